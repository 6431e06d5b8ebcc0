"""The bf16-split main loop of the Winograd-domain weight gradient (conv3x3_wgrad_wino_f32.hip) through the C ABI, against the f32 loop of the
same library (odvae_conv3x3_wgrad_wino_select(0)) and the float64 gradient on the CPU.

Accuracy, the project's criterion for a split product (tests/test_gemm_split_gpu.py): with e(form) = max |dw - dw64| and
sbar = max entry of |G|^T (sum over tiles |V| |dM|) |G| (float64), e(split) <= e(f32) + 2^-22 sbar: the three dropped products are below
2^-22 of sum |a| |b|, everything kept is accumulated in f32 as the f32 loop does.  Each case prints its figures before it asserts;
profiles/wgrad_wino_split.md records them.  That bound would hide a dropped lo . hi product, so the exact recipes of
tests/wgrad_wino_math.py pin the loop bit for bit (tests/test_wgrad_wino_split.py shows that they detect such a loop).

The split loop needs whole chunks of 16 tiles inside a tile row (W / 2 a multiple of 16), so it never meets a ragged last chunk or a
chunk that spans two images; those shapes are covered where they belong, among the shapes that keep the f32 loop bit for bit.  Splits of
unequal length, tile rows of several chunks, single tile rows and image borders inside a split are covered on the split loop.
tests/test_wgrad_wino_exact_gpu.py pins both loops and the reduction bit for bit at the edges of the plan: several chunks per split, a short
last split, the XCD block mapping, ragged chunks on the f32 loop."""
import math

import pytest
import torch
import torch.nn.functional as F

import wgrad_wino_math as wm

pytestmark = pytest.mark.gpu
BWD_TOL = 5e-4      # as tests/test_ops_gpu.py


def dev():
    return torch.device("cuda:0")


def run(hip_lib, x, dy, form, bias=True):
    """x, dy: float64 / f32 NCHW on the host -> dw [Cout][Cin][3][3], dbias [Cout] (device tensors)"""
    from odvae_amd import lib as _lib, ops
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    xd = x.float().to(dev()).permute(0, 2, 3, 1).contiguous()
    dyd = dy.float().to(dev()).permute(0, 2, 3, 1).contiguous()
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=dev())
    db = torch.full((cout,), float("nan"), device=dev())
    assert hip_lib.odvae_conv3x3_wgrad_wino_supported(n, h, w, cin, cout) == 1
    wp, wn = ops._ws(hip_lib.odvae_conv3x3_wgrad_wino_workspace_bytes(n, h, w, cin, cout), xd)
    prev = hip_lib.odvae_conv3x3_wgrad_wino_select(form)
    try:
        _lib.check(hip_lib.odvae_conv3x3_wgrad_wino_f32(xd.data_ptr(), dyd.data_ptr(), n, h, w, cin, cout, dw.data_ptr(),
                                                        db.data_ptr() if bias else None, wp, wn, _lib.stream_ptr()), "wgrad_wino")
    finally:
        hip_lib.odvae_conv3x3_wgrad_wino_select(prev)
    torch.cuda.synchronize()
    return dw, db


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def random_case(kind, n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    dy = torch.randn(n, cout, h, w, generator=g)
    if kind == "mean3":
        x = x + 3.0
    elif kind == "x100":
        x = x * 100.0
    return x.double(), dy.double()


ACCURACY_CASES = [
    # kind, N, Cin, Cout, H, W
    ("normal", 4, 128, 128, 32, 32),     # the narrowest map the gate admits (16 tiles per row), full 128-channel blocks
    ("normal", 2, 256, 256, 32, 32),     # 256 channels: 2 x 2 channel blocks
    ("mean3", 4, 128, 128, 32, 32),
    ("x100", 2, 128, 128, 32, 32),
    ("normal", 1, 384, 128, 2, 32),      # a single tile row, three channel blocks
    ("mean3", 3, 128, 256, 6, 96),       # three chunks per tile row, image borders inside the splits
    ("normal", 5, 128, 128, 14, 64),     # 70 tile rows of two chunks over 64 splits: splits of unequal length
]


@pytest.mark.parametrize("kind,n,cin,cout,h,w", ACCURACY_CASES)
def test_split_loop_is_as_close_to_float64_as_the_f32_loop(hip_lib, kind, n, cin, cout, h, w):
    x, dy = random_case(kind, n, cin, cout, h, w, seed=n * 1000 + cin + h)
    ref, bref = wm.wgrad_f64(x, dy)
    s = wm.sbar(x, dy)
    d0, b0 = run(hip_lib, x, dy, 0)
    d1, b1 = run(hip_lib, x, dy, 1)
    dd, bd = run(hip_lib, x, dy, -1)
    e0 = (d0.cpu().double() - ref).abs().max().item()
    e1 = (d1.cpu().double() - ref).abs().max().item()
    print("%s N%d %d->%d %dx%d: e(f32) %.3e e(split) %.3e sbar %.3e max|dw| %.3e  e(split)/sbar %.3e  bound - e(split) %.3e"
          % (kind, n, cin, cout, h, w, e0, e1, s, ref.abs().max().item(), e1 / s, e0 + 2.0 ** -22 * s - e1))
    assert e1 <= e0 + 2.0 ** -22 * s
    assert bits_equal(b0, b1), "dbias is summed from the unsplit dM in the f32 loop's order"
    assert not bits_equal(d0, d1), "selector 1 ran the f32 loop"
    assert bits_equal(dd, d1) and bits_equal(bd, b1), "the gate admits this shape: the default is the split loop"
    assert (bd.cpu().double() - bref).abs().max().item() <= 1e-5 * max(1.0, bref.abs().max().item())


EXACT_SHAPES = [(2, 128, 128, 4, 32), (1, 256, 256, 4, 32), (1, 384, 128, 2, 32), (2, 128, 256, 6, 64)]


@pytest.mark.parametrize("recipe", ["x3", "dy3", "22"])
@pytest.mark.parametrize("n,cin,cout,h,w", EXACT_SHAPES)
def test_split_loop_is_exact_on_exactly_summable_operands(hip_lib, recipe, n, cin, cout, h, w):
    x, dy = wm.make_exact(recipe, n, cin, cout, h, w, seed=3)
    ref, bref = wm.wgrad_f64(x, dy)
    assert torch.equal(ref.float().double(), ref) and torch.equal(bref.float().double(), bref)
    dw, db = run(hip_lib, x, dy, 1)
    assert bits_equal(dw.cpu(), ref.float()), "dw differs from the float64 gradient in %d entries" % (dw.cpu() != ref.float()).sum().item()
    assert bits_equal(db.cpu(), bref.float())
    dd, _ = run(hip_lib, x, dy, -1)
    assert bits_equal(dd, dw)


BELOW_THE_GATE = [
    (2, 128, 128, 16, 16),      # 8 tiles per row: the narrow-map variant of the f32 loop
    (1, 128, 128, 6, 20),       # 10 tiles per row: chunks span tile rows, ragged last chunk
    (3, 256, 128, 6, 10),       # chunks span images
    (2, 128, 128, 2, 2),
    (1, 128, 256, 4, 48),       # 24 tiles per row: wide enough for the wide f32 variant, not a multiple of 16
]


@pytest.mark.parametrize("n,cin,cout,h,w", BELOW_THE_GATE)
def test_shapes_below_the_gate_keep_the_f32_loop_bit_for_bit(hip_lib, n, cin, cout, h, w):
    x, dy = random_case("mean3", n, cin, cout, h, w, seed=cin + h + w)
    d0, b0 = run(hip_lib, x, dy, 0)
    for form in (-1, 1):
        d, b = run(hip_lib, x, dy, form)
        assert bits_equal(d, d0) and bits_equal(b, b0), "form %d" % form
    ref, _ = wm.wgrad_f64(x, dy)
    assert (d0.cpu().double() - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


def test_selector_returns_the_previous_setting_and_clamps(hip_lib):
    first = hip_lib.odvae_conv3x3_wgrad_wino_select(1)
    try:
        assert first == -1, "the default is the shape rule"
        assert hip_lib.odvae_conv3x3_wgrad_wino_select(0) == 1
        assert hip_lib.odvae_conv3x3_wgrad_wino_select(7) == 0
        assert hip_lib.odvae_conv3x3_wgrad_wino_select(-5) == 1
        assert hip_lib.odvae_conv3x3_wgrad_wino_select(-1) == -1
    finally:
        hip_lib.odvae_conv3x3_wgrad_wino_select(first)


def test_two_launches_agree_bit_for_bit_and_dbias_is_optional(hip_lib):
    x, dy = random_case("normal", 4, 128, 256, 8, 64, seed=11)
    d1, b1 = run(hip_lib, x, dy, 1)
    d2, b2 = run(hip_lib, x, dy, 1)
    assert bits_equal(d1, d2) and bits_equal(b1, b2)
    d3, b3 = run(hip_lib, x, dy, 1, bias=False)
    assert bits_equal(d1, d3) and torch.isnan(b3).all(), "a null dbias is left alone"


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("side", ["x", "dy"])
def test_non_finite_inputs_stay_non_finite(hip_lib, side, value):
    n, cin, cout, h, w = 2, 128, 128, 8, 32
    x, dy = random_case("normal", n, cin, cout, h, w, seed=5)
    ch = 37
    (x if side == "x" else dy)[1, ch, 3, 17] = value      # an interior pixel: it meets all nine taps
    dw, db = run(hip_lib, x, dy, 1)
    dw0, _ = run(hip_lib, x, dy, 0)
    bad = ~torch.isfinite(dw.cpu())
    want = torch.zeros_like(bad)
    if side == "x":
        want[:, ch] = True
        assert torch.isfinite(db).all()
    else:
        want[ch] = True
        assert not torch.isfinite(db[ch]) and torch.isfinite(db.cpu()[torch.arange(cout) != ch]).all()
    assert torch.equal(bad, want), "%d entries non-finite, %d expected" % (bad.sum().item(), want.sum().item())
    assert torch.equal(~torch.isfinite(dw0.cpu()), want), "the f32 loop marks the same entries"


def test_unsupported_shapes_are_still_refused(hip_lib):
    from odvae_amd import lib as _lib, ops
    L = hip_lib
    assert L.odvae_conv3x3_wgrad_wino_supported(2, 33, 32, 128, 128) == 0
    assert L.odvae_conv3x3_wgrad_wino_supported(2, 32, 32, 132, 128) == 0
    x = torch.zeros(2, 32, 32, 132, device=dev())
    dy = torch.zeros(2, 32, 32, 128, device=dev())
    dw = torch.zeros(128, 132, 3, 3, device=dev())
    wp, wn = ops._ws(1 << 20, x)
    prev = L.odvae_conv3x3_wgrad_wino_select(1)
    try:
        rc = L.odvae_conv3x3_wgrad_wino_f32(x.data_ptr(), dy.data_ptr(), 2, 32, 32, 132, 128, dw.data_ptr(), None, wp, wn, _lib.stream_ptr())
        assert rc != 0 and b"unsupported shape" in L.odvae_last_error()
        rc = L.odvae_conv3x3_wgrad_wino_f32(x.data_ptr(), dy.data_ptr(), 2, 32, 32, 128, 128, dw.data_ptr(), None, wp, 16, _lib.stream_ptr())
        assert rc != 0 and b"workspace" in L.odvae_last_error()
    finally:
        L.odvae_conv3x3_wgrad_wino_select(prev)


def test_resnet_block_sized_layer_end_to_end(hip_lib):
    """ops.conv3x3 forward and backward of one 128 -> 128 layer at 64 x 64 (the gate opens: 32 tiles per row) against torch on the CPU"""
    from odvae_amd import ops
    n, cin, cout, h, w = 2, 128, 128, 64, 64
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    gy = torch.randn(n, cout, h, w, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.conv2d(xr, wr, br, padding=1).backward(gy)
    xd, wd, bd = x.to(dev()).requires_grad_(True), wt.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    ops.conv3x3(xd, wd, bd, None, 0).backward(gy.to(dev()))

    def close(a, ref, tol, what):
        err = (a.detach().cpu().double() - ref.double()).abs().max().item()
        scale = max(1.0, ref.abs().max().item())
        assert err <= tol * scale, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, scale)
    close(xd.grad, xr.grad, BWD_TOL, "dx")
    close(wd.grad, wr.grad, BWD_TOL * math.sqrt(n * h * w / 64), "dw")
    close(bd.grad, br.grad, BWD_TOL * math.sqrt(n * h * w / 64), "db")
