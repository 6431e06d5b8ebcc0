"""Host tests (no device) for the f32 implicit-GEMM PatchGAN convolutions: the cases of tests/test_conv4x4_f32_exact_gpu.py are exactly
summable, the index arithmetic of the kernels (tests/conv4x4_f32_inputs.py spells it out in float64) agrees with the host models of
tests/conv4x4_bf16_inputs.py and with torch, the library's host-side decisions (pack size, weight-gradient plan, the supported query)
agree with their mirrors, and ops.conv4x4 dispatches on ops.DISC_F32_IMPLICIT.
On the parent commit these fail: the entry points and the switch do not exist."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import conv4x4_bf16_inputs as M
import conv4x4_f32_inputs as C
import gan_lpips_inputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


def plan_of(L, stride, n, hi, wi, cin, cout):
    out = (ctypes.c_int * 8)()
    assert L.odvae_conv4x4_wgrad_plan(stride, n, hi, wi, cin, cout, out) == 0, L.odvae_last_error()
    return dict(zip(C.PLAN_FIELDS, out))


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.EXTRA_CASES + list(C.WGRAD_SPLIT_CASES.values()), ids=C.case_id)
def test_added_cases_are_exactly_summable(case):
    s = G.assert_exactly_summable4x4(G.make_conv_case(*case))
    print(C.case_id(case), s)
    assert s["worst"] < 2.0 ** 20       # far from the limit: 1.6e5 units is the worst of them


def test_the_cases_of_gan_lpips_inputs_are_exactly_summable():
    """(all 288 in one test: each is a few small float64 convolutions)"""
    worst = max(G.assert_exactly_summable4x4(G.make_conv_case(*c))["worst"] for c in G.CONV_CASES)
    assert worst < G.LIMIT


def test_weight_gradient_split_cases_are_within_the_pixel_budget():
    for stride, case in C.WGRAD_SPLIT_CASES.items():
        s, (h, w), cin, cout, bias, n = case
        assert s == stride and n * G.out4x4(h, s) * G.out4x4(w, s) <= 40000


# ------------------------------------------------------------------------------------------------------------------------------
# the tap and parity algebra of the kernels against the host models and torch, float64
# ------------------------------------------------------------------------------------------------------------------------------
ALGEBRA = [(2, (9, 7), 5, 6, 2), (2, (10, 12), 5, 6, 1), (2, (17, 33), 3, 4, 1), (2, (2, 2), 3, 1, 1), (2, (3, 2), 2, 3, 1),
           (1, (4, 4), 5, 6, 2), (1, (9, 7), 3, 4, 1), (1, (2, 2), 3, 1, 1), (1, (10, 19), 2, 3, 1)]


@pytest.mark.parametrize("stride,hw,cin,cout,n", ALGEBRA)
def test_kernel_index_arithmetic_agrees_with_the_host_models(stride, hw, cin, cout, n):
    c = G.make_conv_case(stride, hw, cin, cout, True, n, seed=4)
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    r = G.conv_references(c)
    y = C.forward_by_pack(x, w, b, stride)
    assert torch.equal(y, M.forward_model(x, w, b, stride)) and torch.equal(y, r["y"])
    dx = C.dgrad_by_pack(dy, w, x.shape, stride)
    assert torch.equal(dx, M.dgrad_model(dy, w, x.shape, stride)) and torch.equal(dx, r["dx"])
    dw = C.wgrad_by_halves(x, dy, stride)
    assert torch.equal(dw, M.wgrad_model(x, dy, stride)) and torch.equal(dw, r["dw"])


def test_the_data_gradient_pack_is_the_flipped_transposed_weight():
    w = G.distinct_integers((3, 2, 4, 4)).double()
    wf = M.flipped_transposed(w)                       # [ci][co][kh][kw] = w[co][ci][3 - kh][3 - kw]
    p1 = C.pack_dgrad_model(w, 1)                      # [t][co][ci]
    assert torch.equal(p1, wf.reshape(2, 3, 16).permute(2, 1, 0))
    p2 = C.pack_dgrad_model(w, 2)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        for a in range(2):
            for b in range(2):      # dgrad_s2_model: class (py, px) takes taps (py + 2a, px + 2b) of the flipped weights
                assert torch.equal(p2[cls * 4 + 2 * a + b], wf[:, :, py + 2 * a, px + 2 * b].t())
    assert sorted(p2.reshape(16, -1)[:, 0].tolist()) == sorted(p1.reshape(16, -1)[:, 0].tolist())      # a permutation of the 16 taps


# ------------------------------------------------------------------------------------------------------------------------------
# what the library decides on the host
# ------------------------------------------------------------------------------------------------------------------------------
def test_pack_floats_matches_its_formula(lib):
    L = lib.load()
    for cr, co in ((3, 64), (64, 3), (1, 512), (512, 1), (64, 128), (130, 72), (72, 130), (33, 32), (32, 33), (256, 512)):
        assert L.odvae_conv4x4_pack_floats(cr, co) == C.pack_floats(cr, co) == 16 * L.odvae_conv3x3_pack_reduce_pad(cr) * L.odvae_conv3x3_pack_out_pad(co)


def test_weight_gradient_plan_agrees_with_its_host_mirror(lib):
    L = lib.load()
    for stride, case in C.WGRAD_SPLIT_CASES.items():
        s, (h, w), cin, cout, bias, n = case
        plan = plan_of(L, s, n, h, w, cin, cout)
        print(stride, plan)
        assert plan == C.wgrad_plan_model(s, n, h, w, cin, cout)
        for k, v in C.WGRAD_SPLIT_PLAN.items():
            assert plan[k] == v, (k, plan)
        last = plan["ntiles"] - (plan["nsplit"] - 1) * plan["tiles_per_split"]
        assert plan["nsplit"] >= 3 and 0 < last < plan["tiles_per_split"] and plan["ci_tiles"] > 1 and plan["co_tiles"] > 1
        ho, wo = G.out4x4(h, s), G.out4x4(w, s)
        assert L.odvae_conv4x4_wgrad_workspace_bytes(s, n, ho, wo, cin, cout) == C.wgrad_workspace_bytes(s, n, h, w, cin, cout)
    for case in C.ALL_CASES[::7] + C.EXTRA_CASES + [(2, (256, 256), 3, 64, True, 32), (1, (31, 31), 512, 1, True, 32)]:
        s, (h, w), cin, cout, bias, n = case
        assert plan_of(L, s, n, h, w, cin, cout) == C.wgrad_plan_model(s, n, h, w, cin, cout), case


def test_plan_and_supported_queries_refuse_what_the_launchers_refuse(lib):
    L = lib.load()
    out = (ctypes.c_int * 8)(*([-7] * 8))
    for args in ((3, 1, 8, 16, 64, 64), (0, 1, 8, 16, 64, 64), (1, 0, 8, 16, 64, 64), (2, 1, 1, 16, 64, 64), (1, 1, 8, 16, 0, 64)):
        assert L.odvae_conv4x4_wgrad_plan(*args, out) == 1
        assert L.odvae_last_error()
        assert list(out) == [-7] * 8
        assert L.odvae_conv4x4_f32_supported(*args) == 0
    assert L.odvae_conv4x4_wgrad_plan(1, 1, 8, 16, 64, 64, None) == 1
    assert L.odvae_conv4x4_f32_supported(2, 32, 256, 256, 3, 64) == 1 and L.odvae_conv4x4_f32_supported(1, 32, 31, 31, 512, 1) == 1
    assert L.odvae_conv4x4_f32_supported(1, 1, 2, 2, 1, 1) == 1
    assert L.odvae_conv4x4_f32_supported(1, 1, 4096, 4096, 32, 4) == 0      # a 2 GiB input image
    assert L.odvae_conv4x4_f32_supported(1, 1, 4097, 4097, 4, 32) == 0      # ... output image (4096 x 4096 x 32)


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_switch_exists_and_is_off_without_the_environment_variable():
    code = "from odvae_amd import ops; print(ops.DISC_F32_IMPLICIT)"
    for value, want in ((None, "False"), ("0", "False"), ("1", "True")):
        env = {k: v for k, v in os.environ.items() if k != "ODVAE_DISC_F32_IMPLICIT"}
        if value is not None:
            env["ODVAE_DISC_F32_IMPLICIT"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])


def test_conv4x4_takes_the_implicit_function_only_when_switched_on_and_supported(lib, monkeypatch):
    from odvae_amd import ops
    L = lib.load()
    taken = []
    monkeypatch.setattr(ops._Conv4x4, "apply", staticmethod(lambda x, w, b, s: (taken.append("im2col"), torch.zeros(x.shape[0], w.shape[0], 1, 1))[1]))
    monkeypatch.setattr(ops._Conv4x4I, "apply", staticmethod(lambda x, w, b, s: (taken.append("implicit"), torch.zeros(x.shape[0], w.shape[0], 1, 1))[1]))
    x, w, w1 = torch.zeros(1, 8, 6, 6), torch.zeros(4, 8, 4, 4), torch.zeros(1, 8, 4, 4)
    monkeypatch.setattr(ops, "DISC_F32_IMPLICIT", False)
    ops.conv4x4(x, w, None, 2)
    assert ops.conv4x4(x, w1, None, 1).shape[1] == 1        # the Cout = 1 -> 4 padding of the im2col route
    monkeypatch.setattr(ops, "DISC_F32_IMPLICIT", True)
    ops.conv4x4(x, w, None, 2)
    assert ops.conv4x4(x, w1, None, 1).shape[1] == 1        # no padding round trip
    monkeypatch.setattr(L, "odvae_conv4x4_f32_supported", lambda *a: 0)
    ops.conv4x4(x, w, None, 2)
    assert taken == ["im2col", "im2col", "implicit", "implicit", "im2col"]
    with pytest.raises(ValueError):
        ops.conv4x4(x, w, None, 3)


@pytest.mark.parametrize("kind", ["c4x4s1", "c4x4s2"])
def test_the_pack_kind_is_tagged_per_weight(kind):
    from odvae_amd import ops
    cache = ops._PackCache()
    w, other = torch.nn.Parameter(torch.zeros(4, 3, 4, 4)), torch.nn.Parameter(torch.zeros(4, 3, 4, 4))
    assert kind in ops._PER_WEIGHT_KINDS
    t0 = cache._tag(w, kind)
    assert t0 == cache.weight_tag(w) == cache._tag(w, "bf16v")
    cache.bump(stepped=[other])                 # the generator's optimizer step: this weight's packs stay valid
    assert cache._tag(w, kind) == t0
    assert cache._tag(w, "direct") != ops._PackCache()._tag(w, "direct")        # ... where an epoch-tagged kind goes stale
    cache.bump(stepped=[w])
    t1 = cache._tag(w, kind)
    assert t1 != t0
    cache.bump()                                # a load_state_dict: any parameter may have changed
    assert cache._tag(w, kind) not in (t0, t1)
