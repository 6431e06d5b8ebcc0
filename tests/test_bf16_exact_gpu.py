"""The bf16 convolution kernels, bit for bit, on exactly summable inputs (tests/exact_inputs.py).

conv_bf16.hip / conv_wgrad_bf16.hip multiply bf16 numbers and add in f32 only.  On operands whose every partial sum is a whole number
of units below 2^24 no f32 addition rounds, so an f32 output must EQUAL the float64 reference and a bf16 output must equal it rounded
once to nearest-even -- whatever the summation order.  Every assertion on a device output here is bit equality
(`exact_inputs.assert_bits_equal`); every test first asserts the precondition on the tensors it uses (`assert_exactly_summable`).
tests/test_exact_inputs.py shows on the host that the checker rejects a dropped term, a wrong rounding mode, a lost operand bit, ...
The random-input tests (test_bf16_gpu.py, test_bf16_fullsize_gpu.py) keep guarding scale and dynamic range.

Instantiations and the cases that reach them (`kernel_of` / `wgrad_kernel_of` below mirror launch_by_cout, conv_bf16_impl and make_plan;
test_case_list_reaches_every_instantiation asserts the table).  conv_bf16_kernel<MODE, KC, WCT, WPT, WAVES_CO, WAVES_PX, 8>; the output-width
class W (Cout > 64) = <2,2,2,2>, M (33..64) = <2,1,1,4>, S (<= 32) = <1,1,1,4>.  "dx of" = the data-gradient launch of that case
(reduce = Cout, out = Cin).  Cases are (mode, N, Cin, Cout, H, W) of CONV_CASES / FWD_ONLY_CASES.

  conv_bf16_kernel        reached by            (the reduction pads to 32, or stays if a multiple of 64: 40 -> 64, 72 -> 96, 104 -> 128, 136 -> 160)
  0 KC64 W                fwd (0,1,40,72,9,17), (0,1,64,136,9,17); dx of (0,1,136,40,9,17) [reduce 40, out 136]
  0 KC64 M                fwd (0,3,64,40,16,16), (0,1,40,64,9,17); dx of (0,3,64,40,16,16)
  0 KC64 S                fwd (0,1,128,24,7,9); dx of every (0,*,24,40,*,*) of the spatial grid [reduce 40, out 24]
  0 KC32 W                fwd (0,1,8,136,9,17), (0,3,136,136,33,33); dx of (0,1,72,24,9,17) [reduce 24, out 72]; forward-only Cout 68, 100, 260
  0 KC32 M                fwd (0,*,24,40,*,*), the spatial grid
  0 KC32 S                fwd (0,1,72,24,9,17); dx of (0,1,8,136,9,17); forward-only (0,1,8,4,9,17)
  1 KC16 W / M / S        fwd (1,1,40,72,18,34) / (1,*,24,40,*,*) grid / (1,1,40,24,*,*) grid
  2 KC32 W / M / S        fwd (2,1,40,72,9,17) / (2,*,24,40,*,*) grid / (2,1,72,24,9,17)
  3 KC32 W / M / S        dx of (1,1,72,24,18,34) [out 72] / dx of (1,1,40,24,*,*) grid [out 40] / dx of (1,*,24,40,*,*) grid [out 24]
  4 KC64 W / M / S        fwd (4,1,40,72,9,17) / (4,3,64,40,3,5) / dx of (4,*,24,40,*,*) grid [reduce 40, out 24]
  4 KC32 W / M / S        fwd (4,1,8,136,9,17), (4,3,1088,1024,9,17) / (4,*,24,40,*,*) grid / (4,1,72,24,9,17)
  0 KC64 W STATS          test_stats_epilogue (1,64,256,9,16), (1,64,128,16,32); (1,64,384,9,17) through the C ABI
  0 KC32 W STATS          test_stats_epilogue (2,8,128,17,33), (1,8,512,7,9), (3,8,256,33,17); (2,8,384,8,16) through the C ABI

  conv_wgrad_bf16_kernel<MODE, TH, COT, CIT>   (4,2) for Cout > 32, (1,4) for Cout <= 32
  0 (4,2) / (1,4)         every mode-0 case of CONV_CASES with Cout > 32 / <= 32
  1 (4,2) / (1,4)         (1,1,40,72,18,34) / (1,1,72,24,18,34)
  2 (4,2) / (1,4)         (2,1,40,72,9,17) / (2,1,72,24,9,17)
  4 (4,2) / (1,4)         (4,1,40,72,9,17) / (4,1,72,24,9,17)
  splits == ntiles: all the small maps.  splits < ntiles, uneven shares: (0,3,136,136,33,33) [6 block pairs -> 42 splits, 45 tiles],
  (0,3,136,24,33,130) [2 pairs -> 128 splits, 135 tiles].  256 / pairs == 1: (4,*,1088,1024,..) [136 pairs; (9,17) x 3: one block walks 58 tiles].
"""

import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CL = torch.channels_last


def dev_cl(t, dtype=BF):
    """host float64 NCHW -> device tensor of dtype in NHWC memory (exact: the precondition says every value is representable)"""
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------------------------------------------
# NaN-filled surroundings for outputs handed to the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
GUARD = 512


def guarded(numel, dtype, fill=float("nan")):
    """a view of numel elements in the middle of a NaN-filled buffer (GUARD elements on either side; 16-byte aligned for bf16 and f32)"""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def assert_guards_intact(buf, view, what):
    n = view.numel()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), what + ": wrote outside its output"


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch, mirrored (launch_by_cout / conv_bf16_impl / make_plan)
# ------------------------------------------------------------------------------------------------------------------------------
def reduce_pad(c):
    return c if c % 64 == 0 else (c + 31) // 32 * 32


def kernel_of(mode, reduce_c, out_c, stats=False):
    kc = {0: 64 if reduce_pad(reduce_c) % 64 == 0 else 32, 1: 16, 2: 32, 3: 32, 4: 64 if reduce_pad(reduce_c) % 64 == 0 else 32}[mode]
    if stats:
        return (0, kc, "W", "STATS")
    return (mode, kc, "W" if out_c > 64 else ("M" if out_c > 32 else "S"))


def kernels_of_case(mode, cin, cout, backward=True):
    ks = {kernel_of(mode, cin, cout)}
    if backward:
        ks.add(kernel_of({0: 0, 1: 3, 2: 0, 4: 4}[mode], cout, cin))
    return ks


def wgrad_kernel_of(mode, cout):
    return (mode, "4x2" if cout > 32 else "1x4")


def wgrad_plan(mode, n, ho, wo, cin, cout):
    th = 4 if mode == 1 else 8
    cot, cit = (4, 2) if cout > 32 else (1, 4)
    coutp, cinp = -(-cout // (cot * 32)) * cot * 32, -(-cin // (cit * 32)) * cit * 32
    ntiles = n * -(-wo // 16) * -(-ho // th)
    pairs = (coutp // (cot * 32)) * (cinp // (cit * 32))
    return {"pairs": pairs, "splits": min(max(1, 256 // pairs), ntiles), "ntiles": ntiles}


ALL_CONV_KERNELS = ({(m, kc, c) for m, kcs in ((0, (64, 32)), (1, (16,)), (2, (32,)), (3, (32,)), (4, (64, 32))) for kc in kcs for c in "WMS"}
                    | {(0, 64, "W", "STATS"), (0, 32, "W", "STATS")})
ALL_WGRAD_KERNELS = {(m, l) for m in (0, 1, 2, 4) for l in ("4x2", "1x4")}

# ------------------------------------------------------------------------------------------------------------------------------
# the case lists: (recipe, mode, N, Cin, Cout, H, W)
# ------------------------------------------------------------------------------------------------------------------------------
# spatial edges: tiles of 8 x 16 (4 x 16 in the Downsample weight gradient) whole, ragged by one, over by one, a single row / column --
# every pair (H, W) of the output sizes below, N alternating between 1 and 3
EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 33)
HW_STRIDE1 = [(h, w) for h in EDGES for w in EDGES]                    # 3x3, 1x1 and the Upsample conv's input (its output: 2 .. 66)
HW_DOWN = [(2 * h, 2 * w) for h in EDGES for w in EDGES]               # even inputs of the Downsample conv: outputs 1 .. 33

CONV_CASES = []
for i, (h, w) in enumerate(HW_STRIDE1):
    CONV_CASES.append(("A", 0, 1 + 2 * (i % 2), 24, 40, h, w))
    CONV_CASES.append(("A", 4, 1 + 2 * ((i + 1) % 2), 24, 40, h, w))
    CONV_CASES.append(("A", 2, 1 + 2 * (i % 2), 24, 40, h, w))
for i, (h, w) in enumerate(HW_DOWN):
    CONV_CASES.append(("A", 1, 1 + 2 * (i % 2), 24, 40, h, w))
    if (h // 2 + w // 2) % 2:
        CONV_CASES.append(("A", 1, 1, 40, 24, h, w))
# channel edges (ragged Cin 8 .. 136, the three output-width classes, both chunk widths) at one ragged map per mode
for mode, (h, w) in ((0, (9, 17)), (1, (18, 34)), (2, (9, 17)), (4, (9, 17))):
    for cin, cout in ((40, 72), (72, 24), (104, 8), (136, 40), (8, 136), (24, 264)):
        CONV_CASES.append(("A", mode, 1, cin, cout, h, w))
CONV_CASES += [
    ("A", 0, 1, 64, 136, 9, 17), ("A", 0, 3, 64, 40, 16, 16), ("A", 0, 1, 128, 24, 7, 9), ("A", 0, 1, 72, 128, 15, 15), ("A", 0, 1, 40, 64, 9, 17),
    ("A", 0, 1, 24, 128, 33, 2), ("A", 4, 1, 64, 136, 9, 17), ("A", 4, 3, 64, 40, 3, 5), ("A", 4, 1, 128, 24, 7, 9), ("A", 4, 1, 40, 64, 9, 17),
    ("A", 1, 1, 64, 64, 16, 32), ("A", 2, 1, 64, 64, 8, 16), ("A", 1, 1, 512, 128, 18, 32), ("A", 0, 1, 512, 128, 9, 16),
    # weight-gradient plans: a block walks several tiles with uneven shares; 136 block pairs -> one split
    ("A", 0, 3, 136, 136, 33, 33), ("A", 0, 3, 136, 24, 33, 130), ("A", 4, 1, 1088, 1024, 2, 7), ("A", 4, 3, 1088, 1024, 9, 17),
    # recipe B: all eight significand bits of x and w in use (K = taps * Cin <= 258)
    ("B", 0, 2, 8, 24, 9, 17), ("B", 0, 1, 8, 72, 17, 33), ("B", 0, 1, 24, 40, 9, 17), ("B", 0, 3, 8, 8, 16, 16), ("B", 1, 1, 8, 40, 18, 34),
    ("B", 1, 3, 24, 8, 16, 32), ("B", 2, 1, 8, 40, 9, 17), ("B", 2, 1, 24, 72, 8, 16), ("B", 4, 2, 136, 136, 3, 5), ("B", 4, 1, 256, 72, 8, 16),
    ("B", 4, 3, 8, 8, 7, 9), ("B", 4, 1, 64, 24, 9, 17),
]
# Cout % 8 == 4: the bf16 store handles runs of four channels, the backward kernels want 16-byte vectors (forward only; the refusal is pinned)
FWD_ONLY_CASES = [("A", mode, n, cin, cout, h, w) for mode, h, w in ((0, 9, 17), (1, 18, 34), (2, 9, 17), (4, 9, 17))
                  for n, cin, cout in ((1, 8, 4), (3, 40, 36), (1, 72, 68), (1, 104, 100), (1, 64, 132), (1, 136, 260))]
FWD_ONLY_CASES += [("B", 0, 2, 8, 36, 9, 17), ("B", 4, 1, 136, 132, 7, 9), ("A", 0, 1, 8, 4, 1, 7)]
STATS_CASES = [(2, 8, 128, 17, 33), (1, 8, 512, 7, 9), (3, 8, 256, 33, 17), (1, 64, 256, 9, 16), (1, 64, 128, 16, 32)]      # (N, Cin, Cout, H, W), groups = 32
STATS_ABI_CASES = [(1, 64, 384, 9, 17, 48), (2, 8, 384, 8, 16, 96)]      # ... , groups: three 128-channel blocks (8 and 4 channels per group)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def test_case_list_reaches_every_instantiation():
    """all 23 conv_bf16_kernel and all 8 conv_wgrad_bf16_kernel instantiations have a case; the weight-gradient plans named in the
    docstring are the ones the case list produces"""
    conv, wgrad = set(), set()
    for _, mode, n, cin, cout, h, w in CONV_CASES:
        conv |= kernels_of_case(mode, cin, cout)
        wgrad.add(wgrad_kernel_of(mode, cout))
    for _, mode, n, cin, cout, h, w in FWD_ONLY_CASES:
        conv |= kernels_of_case(mode, cin, cout, backward=False)
    for n, cin, cout, h, w in STATS_CASES:
        conv.add(kernel_of(0, cin, cout, stats=True))
    assert conv == ALL_CONV_KERNELS, sorted(ALL_CONV_KERNELS - conv)
    assert len(ALL_CONV_KERNELS) == 23
    assert wgrad == ALL_WGRAD_KERNELS and len(wgrad) == 8
    p = wgrad_plan(0, 3, 33, 33, 136, 136)
    assert (p["pairs"], p["splits"], p["ntiles"]) == (6, 42, 45)
    p = wgrad_plan(0, 3, 33, 130, 136, 24)
    assert (p["pairs"], p["splits"], p["ntiles"]) == (2, 128, 135)
    p = wgrad_plan(4, 1, 3 * 9 * 17, 1, 1088, 1024)
    assert (p["pairs"], p["splits"], p["ntiles"]) == (136, 1, 58)
    for mode in (0, 1, 2, 4):      # each mode of the weight gradient also runs with splits == ntiles in both layouts
        small = [c for c in CONV_CASES if c[1] == mode]
        for layout in ("4x2", "1x4"):
            assert any(wgrad_kernel_of(mode, c[4]) == (mode, layout) and
                       (lambda q: q["splits"] == q["ntiles"])(wgrad_plan(mode, c[2], *E.out_hw(mode, c[5], c[6]), c[3], c[4])) for c in small)


# ------------------------------------------------------------------------------------------------------------------------------
# ops.conv3x3 / ops.conv1x1: forward, dx, dw, db, dresidual
# ------------------------------------------------------------------------------------------------------------------------------
def run_ops(ops, c, out_f32=False, dy_f32=None, backward=True, want_dx=True):
    mode = c["mode"]
    xd = dev_cl(c["x"]).requires_grad_(backward and want_dx)
    wd = c["w"].float().to(DEV).requires_grad_(backward)
    bd = c["b"].float().to(DEV).requires_grad_(backward) if c["b"] is not None else None
    rd = dev_cl(c["res"]).requires_grad_(backward) if c["res"] is not None else None
    if mode == 4:
        assert not out_f32
        y = ops.conv1x1(xd, wd, bd, rd)
    else:
        y = ops.conv3x3(xd, wd, bd, rd, mode, out_f32=out_f32)
    got = {"y": y.detach()}
    if backward:
        y.backward(dev_cl(dy_f32, torch.float32) if dy_f32 is not None else dev_cl(c["dy"]))
        got.update(dx=xd.grad, dw=wd.grad, db=bd.grad if bd is not None else None, dres=rd.grad if rd is not None else None)
    return got


def check_case(ops, recipe, mode, n, cin, cout, h, w, bias, residual, backward=True):
    c = E.make_case(recipe, mode, n, cin, cout, h, w, bias, residual)
    E.assert_exactly_summable(c)
    ref = E.references(c)
    got = run_ops(ops, c, backward=backward)
    what = "%s mode %d N%d %d->%d %dx%d" % (recipe, mode, n, cin, cout, h, w)
    E.assert_bits_equal(got["y"], ref["y"], what + " y")
    if backward:
        E.assert_bits_equal(got["dx"], ref["dx"], what + " dx")
        E.assert_bits_equal(got["dw"], ref["dw"], what + " dw")
        if bias:
            E.assert_bits_equal(got["db"], ref["db"], what + " db")
        if residual:
            E.assert_bits_equal(got["dres"], ref["dres"], what + " dresidual", summed=False)


@pytest.mark.parametrize("recipe,mode,n,cin,cout,h,w", CONV_CASES, ids=_ids(CONV_CASES))
def test_conv_bf16_exact(hip_lib, recipe, mode, n, cin, cout, h, w):
    from odvae_amd import ops
    check_case(ops, recipe, mode, n, cin, cout, h, w, True, True)


NOBIAS_CASES = [c for c in CONV_CASES if c[5:] in ((9, 17), (18, 34), (17, 33), (34, 66)) or c[0] == "B"]


@pytest.mark.parametrize("bias,residual", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("recipe,mode,n,cin,cout,h,w", NOBIAS_CASES, ids=_ids(NOBIAS_CASES))
def test_conv_bf16_exact_without_bias_or_residual(hip_lib, recipe, mode, n, cin, cout, h, w, bias, residual):
    """the bias / residual descriptors of the kernel are EMPTY when the operand is absent: the accumulators must start at exactly zero"""
    from odvae_amd import ops
    check_case(ops, recipe, mode, n, cin, cout, h, w, bias, residual)


@pytest.mark.parametrize("recipe,mode,n,cin,cout,h,w", FWD_ONLY_CASES, ids=_ids(FWD_ONLY_CASES))
def test_conv_bf16_exact_cout_4_mod_8(hip_lib, recipe, mode, n, cin, cout, h, w):
    """Cout % 8 == 4: the forward is exact; the backward (16-byte channel vectors of dy) refuses -- an error, not a wrong answer"""
    from odvae_amd import lib, ops
    assert cout % 8 == 4
    check_case(ops, recipe, mode, n, cin, cout, h, w, True, True, backward=False)
    c = E.make_case(recipe, mode, n, cin, cout, h, w, True, False)
    xd, wd = dev_cl(c["x"]).requires_grad_(True), c["w"].float().to(DEV).requires_grad_(True)
    y = ops.conv1x1(xd, wd) if mode == 4 else ops.conv3x3(xd, wd, None, None, mode)
    with pytest.raises(lib.HipLibraryError, match="multiple"):
        y.backward(dev_cl(c["dy"]))
    xd2 = dev_cl(c["x"])
    y = ops.conv1x1(xd2, wd) if mode == 4 else ops.conv3x3(xd2, wd, None, None, mode)
    with pytest.raises(lib.HipLibraryError, match="multiples of 8"):      # the weight gradient on its own
        y.backward(dev_cl(c["dy"]))


@pytest.mark.parametrize("h,w", [(7, 9), (17, 33), (9, 16), (3, 3)])
def test_downsample_odd_sizes(hip_lib, h, w):
    """Downsample at odd input sizes: forward, dw and db are exact (pad (0,1,0,1): the last row / column is read by the centre taps only);
    the data gradient is refused -- its kernel writes 2 Ho x 2 Wo pixels, one row / column short of the input."""
    from odvae_amd import ops
    c = E.make_case("A", 1, 2, 40, 72, h, w, True, True)
    E.assert_exactly_summable(c)
    ref = E.references(c)
    got = run_ops(ops, c, want_dx=False)
    E.assert_bits_equal(got["y"], ref["y"], "y")
    E.assert_bits_equal(got["dw"], ref["dw"], "dw")
    E.assert_bits_equal(got["db"], ref["db"], "db")
    with pytest.raises(RuntimeError):
        run_ops(ops, c, want_dx=True)


def test_degenerate_sizes_are_refused(hip_lib):
    """a 1 x 1 input has no Downsample output: an error, not an empty launch"""
    from odvae_amd import ops
    c = E.make_case("A", 1, 1, 8, 8, 2, 2)
    with pytest.raises(RuntimeError):
        ops.conv3x3(dev_cl(c["x"][:, :, :1, :1]), c["w"].float().to(DEV), None, None, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# the f32 ends as the model uses them
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cout,h,w", [(2, 36, 9, 17), (1, 136, 17, 33), (3, 8, 16, 16)])
def test_conv_in_from_padded_image(hip_lib, n, cout, h, w):
    """the 3-channel f32 image through to_bf16(pad_channels_to=8) into conv_in: cx = 8 != cin = 3, dw cut back to 3 channels"""
    from odvae_amd import ops
    backward = cout % 8 == 0
    c = E.make_case("A", 0, n, 3, cout, h, w, True, False, cx=8)
    E.assert_exactly_summable(c)
    ref = E.references(c)
    img = dev_cl(c["x"][:, :3], torch.float32)
    xb = ops.to_bf16(img, pad_channels_to=8)
    assert tuple(xb.shape) == (n, 8, h, w) and xb.dtype == BF
    E.assert_bits_equal(xb, E.rne(c["x"]), "padded image", summed=False)
    wd, bd = c["w"].float().to(DEV).requires_grad_(backward), c["b"].float().to(DEV).requires_grad_(backward)
    y = ops.conv3x3(xb, wd, bd, None, 0)
    E.assert_bits_equal(y.detach(), ref["y"], "conv_in y")
    if backward:
        y.backward(dev_cl(c["dy"]))
        assert tuple(wd.grad.shape) == (cout, 3, 3, 3)
        E.assert_bits_equal(wd.grad, ref["dw"], "conv_in dw")
        E.assert_bits_equal(bd.grad, ref["db"], "conv_in db")


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 64, 3, 9, 17), (1, 40, 3, 17, 33), (1, 128, 8, 8, 16), (2, 136, 6, 7, 9)])
def test_conv_out_f32_with_f32_gradient(hip_lib, n, cin, cout, h, w):
    """conv_out / the encoder's moments: out_f32 (no rounding, any Cout), an f32 upstream gradient (cast + channel pad to 8 first; db sums
    the f32 values themselves, dw / dx see the cast ones)"""
    from odvae_amd import ops
    c = E.make_case("A", 0, n, cin, cout, h, w, True, False)
    dyf, u = E.f32_gradient(c["dy"].shape)
    E.assert_exactly_summable(c, dyf, u)
    ref = E.references(c, out_f32=True, dy_f32=dyf)
    got = run_ops(ops, c, out_f32=True, dy_f32=dyf)
    assert got["y"].dtype == torch.float32
    for k in ("y", "dx", "dw", "db"):
        E.assert_bits_equal(got[k], ref[k], "conv_out " + k)


# ------------------------------------------------------------------------------------------------------------------------------
# STATS epilogue: y and the per-tile GroupNorm partial sums, slot by slot
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,h,w", STATS_CASES, ids=_ids(STATS_CASES))
@pytest.mark.parametrize("residual", [True, False])
def test_stats_epilogue(hip_lib, n, cin, cout, h, w, residual):
    from odvae_amd import ops
    c = E.make_case("C", 0, n, cin, cout, h, w, True, residual)
    E.assert_exactly_summable(c, stats_groups=32)
    ref = E.references(c, stats_groups=32)
    y = ops.conv3x3(dev_cl(c["x"]), c["w"].float().to(DEV), c["b"].float().to(DEV), dev_cl(c["res"]) if residual else None, 0, gn_stats=True)
    E.assert_bits_equal(y, ref["y"], "y")
    assert getattr(y, "_gn_partials", None) is not None, "the conv left no statistics"
    E.assert_bits_equal(y._gn_partials[0], ref["partials"], "partials [N][tiles][32][2]")


@pytest.mark.parametrize("n,cin,cout,h,w,groups", STATS_ABI_CASES, ids=_ids(STATS_ABI_CASES))
def test_stats_epilogue_three_channel_blocks(hip_lib, n, cin, cout, h, w, groups):
    """Cout = 384 (three 128-channel blocks) through the C ABI; y and the partials sit inside NaN-filled buffers that must stay NaN"""
    L = hip_lib
    from odvae_amd import lib
    c = E.make_case("C", 0, n, cin, cout, h, w, True, True)
    E.assert_exactly_summable(c, stats_groups=groups)
    ref = E.references(c, stats_groups=groups)
    assert L.odvae_conv_bf16_stats_supported(cout, groups) == 1
    xd, rd, wd, bd = dev_cl(c["x"]), dev_cl(c["res"]), c["w"].float().to(DEV).contiguous(), c["b"].float().to(DEV)
    pack = torch.empty(L.odvae_conv_bf16_pack_elems(cin, cout, 9), dtype=BF, device=DEV)
    lib.check(L.odvae_conv_pack_bf16(wd.data_ptr(), cout, cin, 9, pack.data_ptr(), None, lib.stream_ptr()), "pack")
    tiles = L.odvae_conv_bf16_stats_chunks(h, w)
    ybuf, yv = guarded(n * h * w * cout, BF)
    pbuf, pv = guarded(n * tiles * groups * 2, torch.float32)
    lib.check(L.odvae_conv_bf16_stats(xd.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, bd.data_ptr(), rd.data_ptr(), yv.data_ptr(),
                                      pv.data_ptr(), groups, lib.stream_ptr()), "conv_bf16_stats")
    E.assert_bits_equal(yv.view(n, h, w, cout).permute(0, 3, 1, 2), ref["y"], "y")
    E.assert_bits_equal(pv.view(n, tiles, groups, 2), ref["partials"], "partials")
    assert_guards_intact(ybuf, yv, "y")
    assert_guards_intact(pbuf, pv, "partials")


@pytest.mark.parametrize("mode,n,cin,cout,h,w,out_f32", [(0, 1, 40, 68, 9, 17, 0), (0, 2, 64, 3, 7, 9, 1), (1, 1, 24, 36, 18, 34, 0), (2, 1, 72, 24, 7, 9, 0),
                                                          (4, 3, 136, 132, 3, 5, 0), (4, 1, 64, 5, 9, 17, 1), (0, 1, 8, 4, 1, 1, 0)])
def test_conv_abi_writes_only_its_output(hip_lib, mode, n, cin, cout, h, w, out_f32):
    """odvae_conv_bf16 through the C ABI with y inside a NaN-filled buffer: y exact, the surroundings untouched (ragged tiles and channel
    tails end exactly at the last element)"""
    L = hip_lib
    from odvae_amd import lib
    c = E.make_case("A", mode, n, cin, cout, h, w, True, not out_f32)
    E.assert_exactly_summable(c)
    ref = E.references(c, out_f32=bool(out_f32))
    taps = 1 if mode == 4 else 9
    ho, wo = E.out_hw(mode, h, w)
    xd, wd, bd = dev_cl(c["x"]), c["w"].float().to(DEV).contiguous(), c["b"].float().to(DEV)
    rd = dev_cl(c["res"]) if c["res"] is not None else None
    pack = torch.empty(L.odvae_conv_bf16_pack_elems(cin, cout, taps), dtype=BF, device=DEV)
    lib.check(L.odvae_conv_pack_bf16(wd.data_ptr(), cout, cin, taps, pack.data_ptr(), None, lib.stream_ptr()), "pack")
    ybuf, yv = guarded(n * ho * wo * cout, torch.float32 if out_f32 else BF)
    lib.check(L.odvae_conv_bf16(mode, xd.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, bd.data_ptr(), lib.ptr(rd), yv.data_ptr(), ho, wo,
                                out_f32, lib.stream_ptr()), "conv_bf16")
    E.assert_bits_equal(yv.view(n, ho, wo, cout).permute(0, 3, 1, 2), ref["y"], "y")
    assert_guards_intact(ybuf, yv, "y")


@pytest.mark.parametrize("mode,n,cin,cout,h,w", [(0, 1, 40, 72, 9, 17), (1, 2, 24, 8, 18, 34), (2, 1, 72, 24, 7, 9), (4, 3, 136, 136, 3, 5), (0, 3, 136, 24, 33, 130)])
def test_wgrad_abi_writes_only_its_output(hip_lib, mode, n, cin, cout, h, w):
    L = hip_lib
    from odvae_amd import lib
    c = E.make_case("A", mode, n, cin, cout, h, w, True, False)
    E.assert_exactly_summable(c)
    ref = E.references(c)
    ho, wo = E.out_hw(mode, h, w)
    xd, dyd = dev_cl(c["x"]), dev_cl(c["dy"])
    wbuf, wv = guarded(c["w"].numel(), torch.float32)
    bbuf, bv = guarded(cout, torch.float32)
    need = L.odvae_conv_wgrad_bf16_workspace_bytes(mode, n, ho, wo, cin, cout)
    ws = torch.full((need // 4 + 4,), float("nan"), dtype=torch.float32, device=DEV)      # a dirty workspace: every slab entry read must have been written
    lib.check(L.odvae_conv_wgrad_bf16(mode, xd.data_ptr(), dyd.data_ptr(), n, h, w, cin, ho, wo, cout, wv.data_ptr(), bv.data_ptr(), ws.data_ptr(),
                                      need, lib.stream_ptr()), "conv_wgrad_bf16")
    E.assert_bits_equal(wv.view(c["w"].shape), ref["dw"], "dw")
    E.assert_bits_equal(bv, ref["db"], "db")
    assert_guards_intact(wbuf, wv, "dw")
    assert_guards_intact(bbuf, bv, "db")
    assert torch.isnan(ws[need // 4:]).all(), "wrote past the workspace it asked for"


# ------------------------------------------------------------------------------------------------------------------------------
# the image-group loop of the 1x1 forward / data gradient
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8, 8), (3, 5), (2, 6), (1, 1)])      # pixels of a two-image group: 128 (w16 = 16), 30 (2), 24 (8), 2; last group 15 (1), 12 (4)
@pytest.mark.parametrize("recipe,cin,cout", [("A", 72, 40), ("B", 136, 136)])
def test_conv1x1_image_groups(hip_lib, monkeypatch, recipe, cin, cout, h, w):
    """CONV_1X1_GROUP = 2 at N = 5 (groups of 2, 2, 1 images, as inputs past 2 GiB would be split): forward with bias and residual and the
    data gradient equal the one-launch result bit for bit, and the reference"""
    from odvae_amd import ops
    c = E.make_case(recipe, 4, 5, cin, cout, h, w, True, True)
    E.assert_exactly_summable(c)
    ref = E.references(c)
    monkeypatch.setattr(ops, "CONV_1X1_GROUP", 0)
    one = run_ops(ops, c)
    monkeypatch.setattr(ops, "CONV_1X1_GROUP", 2)
    grouped = run_ops(ops, c)
    for k in ("y", "dx", "dw", "db"):
        E.assert_bits_equal(grouped[k], one[k], "grouped vs one launch: " + k)
        E.assert_bits_equal(grouped[k], ref[k], "grouped vs reference: " + k)


def test_conv1x1_image_groups_out_f32(hip_lib, monkeypatch):
    """the same with an f32 output (the group offset of y counts 4-byte elements)"""
    from odvae_amd import ops
    c = E.make_case("A", 4, 5, 72, 6, 3, 5, True, False)
    E.assert_exactly_summable(c)
    ref = E.references(c, out_f32=True)
    xd, wd, bd = dev_cl(c["x"]), c["w"].float().to(DEV), c["b"].float().to(DEV)
    fwd_pack, _ = ops.pack_conv3x3(wd, True, False, "bf16")
    outs = {}
    for grp in (0, 2):
        monkeypatch.setattr(ops, "CONV_1X1_GROUP", grp)
        outs[grp] = ops._conv_b_raw(4, xd, fwd_pack, 6, bd, None, True)
    E.assert_bits_equal(outs[2], outs[0], "grouped vs one launch")
    E.assert_bits_equal(outs[2], ref["y"], "grouped vs reference")


# ------------------------------------------------------------------------------------------------------------------------------
# the small kernels the conv backward leans on, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 8), (3, 7, 9, 40), (2, 8, 16, 136), (1, 17, 33, 24)])
def test_upsample2x_bwd_bf16_exact(hip_lib, n, h, w, c):
    """dx = rne(2x2 sums of du): du holds 8-bit integers times powers of two, so ties and roundings occur and the f32 sums are exact"""
    L = hip_lib
    from odvae_amd import lib
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + c)
    du = (torch.randint(-255, 256, (n, c, 2 * h, 2 * w), generator=g) * 2 ** torch.randint(0, 4, (n, c, 2 * h, 2 * w), generator=g)).double()
    assert torch.equal(E.rne(du).double(), du) and E.pool2x2(du.abs()).max().item() < E.LIMIT
    want = E.rne(E.pool2x2(du))
    inexact, _ = E.rounding_profile(E.pool2x2(du))
    assert inexact > 0.2
    dud = dev_cl(du)
    buf, v = guarded(n * h * w * c, BF)
    lib.check(L.odvae_upsample2x_bwd_bf16(dud.data_ptr(), v.data_ptr(), n, h, w, c, lib.stream_ptr()), "upsample2x_bwd_bf16")
    E.assert_bits_equal(v.view(n, h, w, c).permute(0, 3, 1, 2), want, "dx")
    assert_guards_intact(buf, v, "dx")


@pytest.mark.parametrize("rows,c", [(1, 8), (700, 8), (513, 96), (5000, 96), (1025, 512), (77, 512), (300001, 24), (4099, 2048)])
def test_colsum_bf16_exact(hip_lib, rows, c):
    """column sums of a [rows][C] bf16 matrix: C = 96 is 12 vectors (they do not divide the 256 threads), rows are no multiple of the
    block share"""
    L = hip_lib
    from odvae_amd import lib
    g = torch.Generator().manual_seed(rows + c)
    amax = 255 if rows < 50000 else 15       # the column sums stay below 2^24 units of 1/8
    x = torch.randint(-amax, amax + 1, (rows, c), generator=g).double() / 8
    assert torch.equal(E.rne(x).double(), x) and x.abs().sum(0).max().item() * 8 < E.LIMIT
    xd = x.to(BF).to(DEV)
    need = L.odvae_colsum_bf16_workspace_bytes(rows, c)
    ws = torch.full((need // 4 + 4,), float("nan"), dtype=torch.float32, device=DEV)
    buf, v = guarded(c, torch.float32)
    lib.check(L.odvae_colsum_bf16(xd.data_ptr(), rows, c, v.data_ptr(), ws.data_ptr(), need, lib.stream_ptr()), "colsum_bf16")
    E.assert_bits_equal(v, x.sum(0).float(), "column sums")
    assert_guards_intact(buf, v, "column sums")
    assert torch.isnan(ws[need // 4:]).all()


def cast_probe_values():
    """f32 values a cast must get exactly right: bf16 numbers, ties to even and to odd neighbours, just off a tie, +-0, the largest finite
    f32 (rounds to infinity), the largest that stays finite, subnormals, infinities, random bit patterns"""
    bits = [0x00000000, 0x80000000, 0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF,
            0x7F7F7FFF, 0x7F7F8000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x3EAAAAAB, 0x40490FDB]
    g = torch.Generator().manual_seed(3)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=g, dtype=torch.int64)
    t = torch.cat([torch.tensor(bits, dtype=torch.int64), rnd])
    t = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).view(torch.float32)
    return t[~torch.isnan(t)]


@pytest.mark.parametrize("c,cp", [(3, 8), (8, 8), (6, 8), (3, 16), (40, 40)])
def test_cast_pad_bf16_exact(hip_lib, c, cp):
    """f32 -> bf16 with channel padding: a cast is exact or it is wrong (raw comparison, the sign of zero included); padded channels hold +0"""
    L = hip_lib
    from odvae_amd import lib
    v = cast_probe_values()
    rows = v.numel() // c
    x = v[:rows * c].view(rows, c).contiguous()
    want = torch.zeros(rows, cp, dtype=BF)
    want[:, :c] = x.to(BF)
    buf, out = guarded(rows * cp, BF)
    lib.check(L.odvae_cast_pad_bf16(x.to(DEV).data_ptr(), rows, c, cp, out.data_ptr(), lib.stream_ptr()), "cast_pad_bf16")
    E.assert_bits_equal(out.view(rows, cp), want, "cast_pad_bf16", summed=False)
    assert_guards_intact(buf, out, "cast_pad_bf16")


def test_casts_keep_nan(hip_lib):
    L = hip_lib
    from odvae_amd import lib
    x = torch.tensor([[float("nan"), 1.0, -float("nan"), 2.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
    y = torch.zeros(1, 8, dtype=BF, device=DEV)
    lib.check(L.odvae_cast_pad_bf16(x.data_ptr(), 1, 8, 8, y.data_ptr(), lib.stream_ptr()), "cast_pad_bf16")
    assert torch.isnan(y[0, 0]) and torch.isnan(y[0, 2]) and torch.equal(y[0, [1, 3]].float().cpu(), torch.tensor([1.0, 2.0]))
    z = torch.zeros(1, 8, device=DEV)
    lib.check(L.odvae_cast_f32_from_bf16(y.data_ptr(), 8, z.data_ptr(), lib.stream_ptr()), "cast_f32_from_bf16")
    assert torch.isnan(z[0, 0]) and torch.isnan(z[0, 2]) and torch.equal(z[0, [1, 3]].cpu(), torch.tensor([1.0, 2.0]))


@pytest.mark.parametrize("n", [8, 4096, 65536 + 8])
def test_cast_f32_from_bf16_exact(hip_lib, n):
    """every finite / infinite bf16 bit pattern (n = 65536 + 8) widens to exactly itself"""
    L = hip_lib
    from odvae_amd import lib
    bits = (torch.arange(n, dtype=torch.int64) * (1 if n > 65536 else 37)) % 65536
    x = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(BF)
    keep = ~torch.isnan(x.float())
    x = torch.where(keep, x, torch.zeros_like(x))
    buf, out = guarded(n, torch.float32)
    lib.check(L.odvae_cast_f32_from_bf16(x.to(DEV).data_ptr(), n, out.data_ptr(), lib.stream_ptr()), "cast_f32_from_bf16")
    E.assert_bits_equal(out, x.float(), "cast_f32_from_bf16", summed=False)
    assert_guards_intact(buf, out, "cast_f32_from_bf16")


@pytest.mark.parametrize("cout,cin,taps", [(36, 40, 9), (132, 72, 1), (8, 8, 9), (260, 136, 1), (3, 64, 9)])
def test_conv_pack_bf16_layout(hip_lib, cout, cin, taps):
    """forward and flipped packs against the index formula [tap][RP/16][OP/32][lane][8]: lane (r, h) element j = W[row 32 ot + r][k = 16 kt + 8 h + j];
    every padded slot holds +0"""
    L = hip_lib
    from odvae_amd import lib
    g = torch.Generator().manual_seed(cout + cin)
    k = 3 if taps == 9 else 1
    w = (torch.randint(-255, 256, (cout, cin, k, k), generator=g).double() / 128)
    w[w == 0] = 1.0       # no zero weights: a +0 in the pack is then a padded slot
    wd = w.float().to(DEV).contiguous()

    def want(rows, red, get):
        rp, op = L.odvae_conv_bf16_reduce_pad(red), L.odvae_conv_bf16_out_pad(rows)
        full = torch.zeros(taps, op, rp, dtype=torch.float64)      # [tap][row][k], zero where padded
        full[:, :rows, :red] = get
        # [tap][kt][ot][lane = 32 h + r][j]  <-  full[tap][32 ot + r][16 kt + 8 h + j]
        v = full.view(taps, op // 32, 32, rp // 16, 2, 8).permute(0, 3, 1, 4, 2, 5).contiguous()
        return v.view(-1).float().to(BF), rp, op

    wt = w.view(cout, cin, taps)
    fwd_want, rp_f, op_f = want(cout, cin, wt.permute(2, 0, 1))
    dgr_want, rp_d, op_d = want(cin, cout, wt.flip(2).permute(2, 1, 0))
    assert fwd_want.numel() == L.odvae_conv_bf16_pack_elems(cin, cout, taps) and dgr_want.numel() == L.odvae_conv_bf16_pack_elems(cout, cin, taps)
    fbuf, fv = guarded(fwd_want.numel(), BF)
    dbuf, dv = guarded(dgr_want.numel(), BF)
    lib.check(L.odvae_conv_pack_bf16(wd.data_ptr(), cout, cin, taps, fv.data_ptr(), dv.data_ptr(), lib.stream_ptr()), "conv_pack_bf16")
    E.assert_bits_equal(fv, fwd_want, "forward pack", summed=False)
    E.assert_bits_equal(dv, dgr_want, "flipped pack", summed=False)
    assert (fwd_want == 0).sum().item() == taps * (rp_f * op_f - cout * cin)
    assert_guards_intact(fbuf, fv, "forward pack")
    assert_guards_intact(dbuf, dv, "flipped pack")


# ------------------------------------------------------------------------------------------------------------------------------
# the f32 direct kernels on exact inputs (the other side of the full-size comparison), then full size
# ------------------------------------------------------------------------------------------------------------------------------
def direct_f32(monkeypatch, ops):
    """the f32 path on its direct kernels: F(2x2) / F(4x4) Winograd transforms hold 1/4, 1/24 and are not exact"""
    monkeypatch.setattr(ops, "WINOGRAD", False)
    monkeypatch.setattr(ops, "WGRAD_WINOGRAD", False)
    monkeypatch.setattr(ops, "UPCONV_WINOGRAD4", False)


def run_f32(ops, mode, x, w, b, dy):
    xd = x.requires_grad_(True)
    wd, bd = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ops.KERNEL_EVENTS.enable()
    try:
        y = ops.conv3x3(xd, wd, bd, None, mode)
        y.backward(dy)
        ran = sorted(ops.KERNEL_EVENTS.rec)
    finally:
        ops.KERNEL_EVENTS.disable()
    assert not [k for k in ran if "wino" in k], "a Winograd kernel ran: %s" % ran
    if mode == 0 and w.shape[0] > 32:
        assert "conv3x3_128x128" in ran, "the direct stride-1 kernel did not run: %s" % ran
    return y.detach(), xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("mode,n,cin,cout,h,w", [(0, 2, 40, 72, 17, 33), (0, 1, 128, 128, 16, 32), (1, 1, 64, 128, 18, 34), (2, 1, 128, 64, 9, 17), (2, 2, 128, 128, 16, 16)])
def test_f32_direct_kernels_exact(hip_lib, monkeypatch, mode, n, cin, cout, h, w):
    """the f32 direct kernels equal float64 on the same integers (no rounding anywhere): the yardstick of the full-size cases is sound"""
    from odvae_amd import ops
    direct_f32(monkeypatch, ops)
    c = E.make_case("A", mode, n, cin, cout, h, w, True, False)
    E.assert_exactly_summable(c)
    y, dx, dw, db = run_f32(ops, mode, dev_cl(c["x"], torch.float32), c["w"].float().to(DEV), c["b"].float().to(DEV), dev_cl(c["dy"], torch.float32))
    du = E.dgrad_f64(mode, c["dy"], c["w"], c["x"].shape)
    E.assert_bits_equal(y, c_y(c).float(), "f32 y")
    E.assert_bits_equal(dx, (E.pool2x2(du) if mode == 2 else du).float(), "f32 dx")
    E.assert_bits_equal(dw, E.wgrad_f64(mode, c["x"], c["dy"], c["w"].shape).float(), "f32 dw")
    E.assert_bits_equal(db, c["dy"].sum((0, 2, 3)).float(), "f32 db")


def c_y(c):
    return E.conv_f64(c["mode"], c["x"], c["w"], c["b"])


def device_ints(shape, lo, hi, seed, scale=1.0):
    """recipe D operands made on the device from a seed: integers in [lo, hi] times scale, NHWC for 4-d shapes (f32; exact in bf16 too)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g, device=DEV, dtype=torch.int8).float()
    if scale != 1.0:
        t *= scale
    return t.contiguous(memory_format=CL) if len(shape) == 4 else t


def bits_equal_on_device(got, want, what):
    """torch.equal on integer views, -0.0 folded into +0.0 (sums); nothing of full size leaves the device"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = torch.int16 if got.dtype == BF else torch.int32
    same = torch.equal((got + 0.0).contiguous().view(view), (want + 0.0).contiguous().view(view))
    if not same:       # name the suspects: the small report of assert_bits_equal on the first image that differs
        for i in range(got.shape[0]):
            E.assert_bits_equal(got[i:i + 1], want[i:i + 1], "%s, image / row block %d" % (what, i))
    assert same, what


def host_anchor(mode, x, w, b, y32, dw32, dy, samples=48, seed=1):
    """the f32 side anchored on the host: int64 recomputation (in units of 1/8) of sampled y elements plus the four corners, and of
    sampled dw entries -- at equality"""
    n, cin, h, wd_ = x.shape
    _, cout, ho, wo = y32.shape
    g = torch.Generator().manual_seed(seed)
    pts = [(0, 0, 0, 0), (n - 1, cout - 1, 0, wo - 1), (0, cout - 1, ho - 1, 0), (n - 1, 0, ho - 1, wo - 1)]
    pts += [tuple(int(torch.randint(0, m, (1,), generator=g)) for m in (n, cout, ho, wo)) for _ in range(samples)]
    w8 = (w.cpu().double() * 4).round().to(torch.int64)                       # w in units of 1/4
    b8 = (b.cpu().double() * 8).round().to(torch.int64)                       # bias in units of 1/8
    for (i, co, oy, ox) in pts:
        acc = int(b8[co])
        for kh in range(3):
            for kw in range(3):
                if mode == 0:
                    iy, ix = oy + kh - 1, ox + kw - 1
                elif mode == 1:
                    iy, ix = 2 * oy + kh, 2 * ox + kw
                else:
                    iy, ix = oy + kh - 1, ox + kw - 1
                    if not (0 <= iy < 2 * h and 0 <= ix < 2 * wd_):
                        continue
                    iy, ix = iy // 2, ix // 2
                if 0 <= iy < h and 0 <= ix < wd_:
                    xv = x[i, :, iy, ix].cpu().to(torch.int64)
                    acc += 2 * int((xv * w8[co, :, kh, kw]).sum())
        got = y32[i, co, oy, ox].item()
        assert got * 8 == acc, "f32 y(%d, %d, %d, %d) = %r, int64 recomputation %r / 8" % (i, co, oy, ox, got, acc)
    if mode == 0:      # dw[co][ci][kh][kw] = sum over images and pixels of dy[co][oy][ox] x[ci][oy + kh - 1][ox + kw - 1]
        for _ in range(6):
            co, ci = (int(torch.randint(0, m, (1,), generator=g)) for m in (cout, cin))
            kh, kw = (int(torch.randint(0, 3, (1,), generator=g)) for _ in range(2))
            xs = torch.zeros(n, h + 2, wd_ + 2, dtype=torch.int64)
            xs[:, 1:-1, 1:-1] = x[:, ci].cpu().to(torch.int64)
            acc = int((dy[:, co].cpu().to(torch.int64) * xs[:, kh:kh + h, kw:kw + wd_]).sum())
            got = dw32[co, ci, kh, kw].item()
            assert got == acc, "f32 dw(%d, %d, %d, %d) = %r, int64 recomputation %r" % (co, ci, kh, kw, got, acc)


FULL = {0: (32, 128, 128, 256, 256), 1: (32, 128, 128, 256, 256), 2: (32, 128, 128, 128, 128)}      # mode -> (N, Cin, Cout, H, W) of the input


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_full_size_against_f32_direct_kernels(hip_lib, monkeypatch, mode):
    """B = 32, 128 -> 128 channels at the model's largest maps (recipe D): the WHOLE y, dx, dw, db of the bf16 kernels against the project's
    own f32 direct kernels on the same integers -- y_bf16 == rne(y_f32), dw equal: two independent kernels agreeing bit for bit on up to
    268 M elements per tensor.  The f32 side is anchored by int64 recomputation of sampled elements on the host.
    dw sums 2^21 pixels of |x dy| <= 4: at most 2^23 units; y: 9 * 128 taps of |x w| <= 4, far below."""
    from odvae_amd import ops
    direct_f32(monkeypatch, ops)
    n, cin, cout, h, w = FULL[mode]
    ho, wo = E.out_hw(mode, h, w)
    assert n * ho * wo * 2 * 2 < E.LIMIT and 9 * cin * 2 * 2 * 8 + 16 < E.LIMIT      # the summability precondition in closed form: |x|, |dy|, |w| <= 2
    x = device_ints((n, cin, h, w), -2, 2, 11 + mode)
    dy = device_ints((n, cout, ho, wo), -2, 2, 21 + mode)
    wt = device_ints((cout, cin, 3, 3), -8, 8, 31 + mode, 0.25).contiguous()
    b = device_ints((cout,), -16, 16, 41 + mode, 0.125)
    for t in (x, dy, wt):
        assert torch.equal(t.to(BF).float(), t)
    assert x.abs().max().item() <= 2 and dy.abs().max().item() <= 2 and wt.abs().max().item() <= 2 and b.abs().max().item() <= 2      # what the closed form assumes
    assert torch.equal(x, x.round()) and torch.equal(dy, dy.round()) and torch.equal(wt * 4, (wt * 4).round()) and torch.equal(b * 8, (b * 8).round())
    y32, dx32, dw32, db32 = run_f32(ops, mode, x.clone(), wt, b, dy)
    host_anchor(mode, x, wt, b, y32, dw32, dy)
    if mode == 2:       # the bf16 path rounds the gradient w.r.t. the upsampled image before its 2x2 sums: take that image from the f32 stride-1 kernel
        z = torch.zeros(n, cin, ho, wo, device=DEV).contiguous(memory_format=CL).requires_grad_(True)
        ops.conv3x3(z, wt.clone().requires_grad_(True), None, None, 0).backward(dy)
        du = z.grad.to(BF).float()
        dx_want = (du[:, :, 0::2, 0::2] + du[:, :, 0::2, 1::2] + du[:, :, 1::2, 0::2] + du[:, :, 1::2, 1::2]).to(BF)
        del z, du
    else:
        dx_want = dx32.to(BF)
    y_want = y32.to(BF)
    del y32, dx32
    xb = x.to(BF).requires_grad_(True)
    wd, bd = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.conv3x3(xb, wd, bd, None, mode)
    y.backward(dy.to(BF))
    bits_equal_on_device(y.detach(), y_want, "y (mode %d)" % mode)
    bits_equal_on_device(xb.grad, dx_want, "dx (mode %d)" % mode)
    bits_equal_on_device(wd.grad, dw32, "dw (mode %d)" % mode)
    bits_equal_on_device(bd.grad, db32, "db (mode %d)" % mode)
