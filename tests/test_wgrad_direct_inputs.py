"""tests/wgrad_direct_inputs.py against autograd, and its cases against the plan the library reports.  Host only: the plan query
(odvae_conv3x3_wgrad_plan) launches nothing and needs no device."""
import pytest
import torch

import wgrad_direct_inputs as W


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


def ref_conv(mode, x, w, b):
    from test_ops_gpu import ref_conv as rc        # the three definitions every conv test of the suite compares against
    return rc(mode, x, w, b)


@pytest.mark.parametrize("mode,n,cin,cout,hi,wi", [(0, 2, 5, 7, 6, 9), (0, 1, 3, 4, 1, 1), (1, 2, 5, 7, 6, 10), (1, 1, 2, 3, 2, 2),
                                                   (2, 2, 5, 7, 3, 5), (2, 1, 4, 2, 1, 2)])
def test_wgrad_f64_is_float64_autograd_of_the_reference_conv(mode, n, cin, cout, hi, wi):
    g = torch.Generator().manual_seed(100 * mode + hi)
    x = torch.randn(n, cin, hi, wi, generator=g, dtype=torch.float64)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = ref_conv(mode, x, w, b)
    assert tuple(y.shape[2:]) == W.out_hw(mode, hi, wi)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    for m in ((mode, 5) if mode == 2 else (mode,)):
        dw, db = W.wgrad_f64(m, x, dy)
        assert (dw - w.grad).abs().max().item() <= 1e-13 * w.grad.abs().max().item()
        assert (db - b.grad).abs().max().item() <= 1e-13 * b.grad.abs().max().item()


def test_wgrad_f64_is_exact_on_the_exact_operands():
    """on make_exact's operands autograd and the nine products agree to the last bit: both are sums of whole numbers"""
    for mode, shape in ((0, (2, 5, 7, 6, 9)), (1, (2, 5, 7, 6, 10)), (2, (2, 5, 7, 3, 5))):
        x, dy = W.make_exact(mode, *shape, seed=mode)
        assert set(x.abs().unique().tolist()) <= set(range(1, W.MAGNITUDE + 1)) and (x == x.round()).all()
        w = torch.zeros(shape[2], shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(shape[2], dtype=torch.float64, requires_grad=True)
        ref_conv(mode, x, w, b).backward(dy)
        dw, db = W.wgrad_f64(mode, x, dy)
        assert torch.equal(dw, w.grad) and torch.equal(db, b.grad)


def test_make_exact_refuses_sums_that_could_round():
    """7 * 7 * 342 393 pixels reach 2^24: a 586 x 586 image of sevens has more, a 585 x 585 one has fewer; 800 x 800 pixels of mean
    magnitude 4 against a largest magnitude of 7 are over it too"""
    x = torch.full((1, 1, 586, 586), 7.0)
    assert W.exact_bound(x, x) >= W.EXACT_LIMIT > W.exact_bound(x[:, :, :585, :585], x[:, :, :585, :585])
    with pytest.raises(AssertionError):
        W.make_exact(0, 1, 1, 1, 800, 800, seed=0)
    W.make_exact(0, 1, 1, 1, 500, 500, seed=0)


@pytest.mark.parametrize("name", list(W.CASES))
def test_every_case_reaches_the_path_it_is_named_after(lib, name):
    mode, n, cin, cout, hi, wi, expect = W.CASES[name]
    plan = lib.conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout)
    print(name, plan)
    got = W.plan_properties(plan, n, hi)
    expect = dict(expect)
    if plan["kind"] == "thin":
        assert expect.pop("Cs") == min(cin, cout) <= 3
    assert {k: got[k] for k in expect} == expect, "%s: the library plans %s" % (name, plan)


def test_the_cases_cover_every_path_between_them(lib):
    """what the case list as a whole has to hold, stated on the reported plans and not on the case names"""
    plans = {}
    for name, (mode, n, cin, cout, hi, wi, _) in W.CASES.items():
        plan = lib.conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout)
        plans[name] = dict(W.plan_properties(plan, n, hi), n=n, mode=mode, cs=min(cin, cout), thin_in=cin <= 3, w=wi)
    for kind in ("v2", "up"):                         # the double-buffered kernels: both buffers reused, and an odd count per block
        of = [p for p in plans.values() if p["kind"] == kind]
        assert any(p["tiles_per_split"] >= 3 for p in of), kind
        assert any(p["tiles_per_split"] % 2 == 1 for p in of), kind
    for kind in ("v1", "v2", "up"):
        of = [p for p in plans.values() if p["kind"] == kind]
        assert all(p["tiles_per_split"] >= 2 for p in of), kind
        assert any(p["last"] < p["tiles_per_split"] for p in of), kind + ": no short last split"
        assert any(p["crosses_images"] for p in of), kind + ": no split spans two images"
        assert any(p["n"] >= 2 for p in of), kind
    assert {p["effective_mode"] for p in plans.values() if p["kind"] == "v1"} == {0, 1, 2}
    assert {p["effective_mode"] for p in plans.values() if p["kind"] == "v2"} == {0, 1, 2}
    assert any(p["kind"] == "v1" and p["mode"] == 5 for p in plans.values())            # the mode 5 -> 2 fallback
    thin = [p for p in plans.values() if p["kind"] == "thin"]
    for thin_in in (True, False):
        of = [p for p in thin if p["thin_in"] == thin_in]
        assert {p["cs"] for p in of} == {1, 2, 3}
        assert any(p["rows_per_wave_max"] >= 2 and p["n"] >= 2 for p in of)
        assert any(p["blocks"] < 32 for p in of)
        assert any(p["waves"] >= 128 and p["waves"] % 128 != 0 for p in of)
    assert {p["w"] for p in thin if p["rows_per_wave_max"] >= 2} >= {16, 48}


def test_plan_query_refuses_what_the_launcher_refuses(lib):
    import ctypes
    L = lib.load()
    out = (ctypes.c_int * 8)(*([-7] * 8))
    for args in ((3, 1, 8, 16, 64, 64), (1, 1, 7, 16, 64, 64), (0, 0, 8, 16, 64, 64)):
        assert L.odvae_conv3x3_wgrad_plan(*args, out) == 1
        assert L.odvae_last_error()
        assert list(out) == [-7] * 8
    assert L.odvae_conv3x3_wgrad_plan(0, 1, 8, 16, 64, 64, None) == 1
    # one split's slab of the parity kernel, 16 * CinP * CoutP * 4 bytes: 2^31 at 4096 x 8192 channels, one channel tile less below it
    assert L.odvae_conv3x3_wgrad_plan(5, 1, 1, 1, 4096, 8192, out) == 1
    assert "slab" in L.odvae_last_error().decode() and list(out) == [-7] * 8
    assert L.odvae_conv3x3_wgrad_plan(5, 1, 1, 1, 4096, 8128, out) == 0
    assert list(out)[0] == 3
