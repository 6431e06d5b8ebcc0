"""The thin 3x3 kernels at FOUR thin channels (an RGBA reconstruction: image_mask_key with ddconfig.out_ch 4), bit for bit against float64
on exactly summable operands -- the builders and the launch helpers of tests/test_conv3x3_f32_exact_gpu.py and
tests/test_wgrad_direct_exact_gpu.py, by import.

  thin-out   conv3x3_thin_out_kernel<128, 4>: 128 -> 4, 36 tap columns in two column tiles
  thin-in    conv3x3_thin_in_kernel<4>: Cin = 4, eighteen MFMA steps, a tap's channels one 16-byte load
  thin wgrad conv3x3_wgrad_thin_kernel<2>: a 4-channel thin side either way, the bias column on the conv_in side, thin_colsum on the other
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_f32_exact_inputs as C  # noqa: E402
import exact_inputs as E  # noqa: E402
import test_conv3x3_f32_exact_gpu as TC  # noqa: E402
import test_wgrad_direct_exact_gpu as TW  # noqa: E402
import wgrad_direct_inputs as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def conv_case(route, n, cin, cout, h, w):
    name = "%s-n%d-%dto%d-%dx%d" % (route, n, cin, cout, h, w)
    c = E.make_case("A", 0, n, cin, cout, h, w, seed=C.case_seed(name) % 1000)
    c.update(route=route, mode=0, n=n, cin=cin, cout=cout, hi=h, wi=w, abi=0, name=name)
    C.assert_exactly_summable(c)
    return c


@pytest.mark.parametrize("n,h,w", [(1, 8, 32), (2, 9, 33), (1, 3, 5), (1, 16, 64)])
def test_thin_output_kernel_at_four_channels(hip_lib, n, h, w):
    """128 -> 4 with and without bias (thin-out), with residual + ReLU (the generic kernel, as at 3 channels), and its data gradient
    (Cin' = 4: the thin-in kernel where W % 32 == 0, the generic one elsewhere)."""
    c = conv_case("thin_out", n, 128, 4, h, w)
    r = TC.Run(hip_lib)
    fwd, dgr = TC.direct_packs(r, c)
    TC.run_direct_forward(r, c, fwd, {"bias": (True, False, 0), "no bias": (False, False, 0), "generic kernel: bias + residual + ReLU": (True, True, 1)})
    TC.run_direct_dgrad(r, c, dgr)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h", [1, 2, 5])
@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("cout", [128, 130])
def test_thin_input_kernel_at_four_channels(hip_lib, cout, w, h, n):
    """Cin = 4: one and two co blocks (130: the second two channels wide), one and two segments per row, with bias + residual + ReLU and bare."""
    c = conv_case("thin_in", n, 4, cout, h, w)
    r = TC.Run(hip_lib)
    fwd, dgr = TC.direct_packs(r, c)
    TC.run_direct_forward(r, c, fwd, TC.FULL_AND_NONE)
    TC.run_direct_dgrad(r, c, dgr)


def wgrad_plan(n, hi, wi, cin, cout):
    from odvae_amd import lib
    return lib.conv3x3_wgrad_plan(0, n, hi, wi, cin, cout)


def check_wgrad(hip_lib, n, cin, cout, h, w):
    plan = wgrad_plan(n, h, w, cin, cout)
    groups = -(-max(cin, cout) // 128)                                   # the launcher's rule: channel groups of 128 on the wide side,
    blocks = max(1, min(1024 // groups, -(-(n * h) // 4)))               # four waves (image rows in flight) per block
    assert plan["kind"] == "thin", plan
    assert W.plan_properties(plan, n, h) == dict(kind="thin", blocks=blocks, waves=4 * blocks, groups=groups,
                                                 rows_per_wave_max=-(-(n * h) // (4 * blocks))), plan
    x, dy = W.make_exact(0, n, cin, cout, h, w, 1000 * cin + 10 * h + w + n)
    dw64, db64 = W.wgrad_f64(0, x, dy)
    run = TW.Launch(hip_lib, 0, x, dy)
    dw, db = run.run()
    assert not torch.isnan(dw).any().item() and not torch.isnan(db).any().item(), "an output element was never written"
    assert torch.equal(dw.double(), dw64), "dw: " + TW.mismatch(dw, dw64)
    assert torch.equal(db.double(), db64), "db: " + TW.mismatch(db, db64)
    dw3, db3 = run.run(bias=False)                         # dbias = NULL: the same dw, and nothing else written
    assert torch.equal(dw3, dw) and torch.isnan(db3).all().item()
    return plan


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h", [1, 3, 8])
@pytest.mark.parametrize("w", [16, 32, 48])
@pytest.mark.parametrize("cin,cout", [(4, 128), (128, 4), (4, 36), (32, 4)])
def test_thin_weight_gradient_at_four_channels(hip_lib, cin, cout, w, h, n):
    check_wgrad(hip_lib, n, cin, cout, h, w)


@pytest.mark.parametrize("cin,cout", [(4, 128), (128, 4)])
def test_thin_weight_gradient_wave_with_rows_of_two_images(hip_lib, cin, cout):
    """4098 rows over the grid cap's 4096 waves: waves 0 and 1 own a row of the first image and one of the third."""
    plan = check_wgrad(hip_lib, 3, cin, cout, 1366, 16)
    assert plan["nsplit"] == 4096 and plan["nsplit"] < 3 * 1366 <= 2 * plan["nsplit"]


def test_a_workspace_one_byte_short_is_refused(hip_lib):
    x, dy = W.make_exact(0, 1, 128, 4, 3, 16, 5)
    run = TW.Launch(hip_lib, 0, x, dy)
    assert run.need >= 4 * 128 * 64 * 4      # two column tiles: 64 slab columns per wide channel and wave
    run.outputs()
    assert run.raw(ws_bytes=run.need - 1) == TW.ERR_WORKSPACE
    run.assert_untouched()


def test_autograd_conv_out_at_four_channels(hip_lib):
    """ops.conv3x3 128 -> 4 at 16 x 32: y from the thin-out kernel, dx from the thin-in kernel, dw and db from the thin weight gradient."""
    from odvae_amd import ops
    c = conv_case("thin_out", 1, 128, 4, 16, 32)
    assert ops._conv3x3_route(0, 16, 32, 128, 4, False) == "direct"
    assert wgrad_plan(1, 16, 32, 128, 4)["kind"] == "thin"
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    xd = x.float().to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True)
    y = ops.conv3x3(xd, wd, bd)
    y.backward(dy.float().to(DEV))
    dw64, db64 = W.wgrad_f64(0, x, dy)
    assert W.exact_bound(x, dy) < 2 ** 24
    for what, got, want in (("y", y.detach(), C.conv_ref(0, x, w, b)), ("dx", xd.grad, C.dgrad_ref(0, dy, w, x.shape)), ("dw", wd.grad, dw64),
                            ("db", bd.grad, db64)):
        got = got.cpu().contiguous()
        assert torch.equal(got.double(), want), "%s: %s" % (what, TC.mismatch(got, want))
