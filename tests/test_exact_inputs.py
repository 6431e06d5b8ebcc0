"""The exact-input checker must be able to fail (CPU only).

torch on the host stands in for the kernels: float32 `F.conv2d` and float32 autograd, which on exactly summable operands give the
exact sums just as the kernels' f32 accumulators must.  The unmutated stand-in passes every reference of `exact_inputs`; each
mutant below plants one of the faults the bit-for-bit GPU tests (tests/test_bf16_exact_gpu.py) exist to catch, and must be REJECTED
by `assert_bits_equal` -- one named "must fail" test per mutant and recipe it applies to.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-in: ops._ConvB's rounding chain in float32 on the host, with switchable faults
# ------------------------------------------------------------------------------------------------------------------------------
def store_bf16(t, how="rne"):
    """f32 -> bf16 as the kernels' store does (rne), or one of the wrong ways"""
    t = t.float().contiguous()
    if how == "rne":
        return t.to(BF)
    bits = t.view(torch.int32)
    if how == "half_away":       # sign-magnitude: adding half an ulp to the magnitude rounds ties away from zero
        bits = bits + 0x8000
    return (bits & -65536).view(torch.float32).to(BF)       # (-65536 = 0xFFFF0000: truncation)


def clear_low_bit(t):
    """the lowest significand bit of every bf16 element cleared (an operand path that loses one bit)"""
    return (t.float().to(BF).view(torch.int16) & -2).view(BF).double()


def standin(c, out_f32=False, dy_f32=None, fault=None, at=None):
    """y, dx, dw, db, dres of case c in float32.  fault: None or the name of one planted fault; at: where (fault-specific)."""
    mode, cin = c["mode"], c["w"].shape[1]
    x, w = c["x"][:, :cin].float(), c["w"].float()
    if fault == "operand_low_bit":
        x = clear_low_bit(c["x"][:, :cin]).float()
    xs = x
    if fault == "wrap_right":       # the tap right of the last column reads the first pixel of the next row instead of zero (mode 0)
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 1:-1, -1] = torch.roll(x[:, :, :, 0], -1, 2)
        s = F.conv2d(xp, w)
    else:
        s = E.conv_f64(mode, xs, w)
    if fault == "drop_term":        # one (tap, channel) term missing at one output pixel (mode 0), every output channel
        n, ci, py, px, kh, kw = at
        s[n, :, py, px] -= x[n, ci, py + kh - 1, px + kw - 1] * w[:, ci, kh, kw]
    if fault == "acc_roundtrip":    # the sum takes a bf16 round trip before bias and residual are added
        s = s.to(BF).float()
    if c["b"] is not None:
        s = s + c["b"].float().view(1, -1, 1, 1)
    if c["res"] is not None:
        s = s + c["res"].float()
    if fault == "nan":
        s[at] = float("nan")
    how = {"truncate": "trunc", "half_away": "half_away"}.get(fault, "rne")
    y = s if out_f32 else store_bf16(s, how)

    dyb = (dy_f32.float().to(BF) if dy_f32 is not None else c["dy"].float().to(BF)).float()
    du = E.dgrad_f64(mode, dyb, w, x.shape)
    if mode == 2:
        du2 = du if fault == "skip_second_rounding" else store_bf16(du, how).float()
        dx = store_bf16(E.pool2x2(du2), how)
    else:
        dx = store_bf16(du, how)
    dyw = dyb
    if fault == "dw_row":           # one pixel row of the upstream gradient left out of the weight gradient
        dyw = dyb.clone()
        dyw[:, :, at] = 0
    dw = E.wgrad_f64(mode, x, dyw, w.shape)
    db = (dy_f32.float() if dy_f32 is not None else dyb).sum((0, 2, 3))
    return {"y": y, "dx": dx, "dw": dw, "db": db, "dres": dyb.to(BF)}


def check_all(got, ref):
    for k in ("y", "dx", "dw", "db", "dres"):
        E.assert_bits_equal(got[k], ref[k], k)


CASES = {       # recipe -> (mode, n, cin, cout, h, w): ragged channels, ragged tiles, a tile seam inside the image
    "A": [(0, 2, 40, 68, 17, 33), (1, 1, 40, 36, 18, 34), (2, 1, 40, 68, 9, 17), (4, 3, 72, 36, 5, 7), (0, 1, 8, 4, 1, 7)],
    "B": [(0, 2, 8, 36, 9, 17), (1, 1, 8, 24, 18, 34), (2, 1, 8, 8, 9, 17), (4, 2, 136, 132, 3, 5)],
    "C": [(0, 2, 8, 128, 17, 33), (0, 1, 64, 256, 9, 16)],
    "D": [(0, 1, 128, 128, 16, 32)],
}
ALL = [(r,) + s for r, lst in CASES.items() for s in lst]


@pytest.mark.parametrize("recipe,mode,n,cin,cout,h,w", ALL)
@pytest.mark.parametrize("bias,residual", [(True, True), (False, False)])
def test_standin_passes(recipe, mode, n, cin, cout, h, w, bias, residual):
    c = E.make_case(recipe, mode, n, cin, cout, h, w, bias, residual)
    groups = 32 if recipe == "C" else None
    E.assert_exactly_summable(c, stats_groups=groups)
    ref = E.references(c, stats_groups=groups)
    got = standin(c)
    check_all(got, ref)
    if groups:      # the statistics a float32 epilogue would form from the rounded y
        E.assert_bits_equal(E.tile_group_sums(got["y"].float(), groups), ref["partials"], "partials")


@pytest.mark.parametrize("mode,n,cin,cout,h,w", [(0, 2, 64, 3, 9, 17), (4, 2, 40, 8, 9, 17), (0, 1, 40, 68, 8, 16)])
def test_standin_passes_f32_ends(mode, n, cin, cout, h, w):
    """out_f32 forward (no rounding) and an f32 upstream gradient (cast first; the bias gradient sums the f32 values)"""
    c = E.make_case("A", mode, n, cin, cout, h, w, True, False)
    dyf, u = E.f32_gradient(c["dy"].shape)
    E.assert_exactly_summable(c, dyf, u)
    ref = E.references(c, out_f32=True, dy_f32=dyf)
    assert ref["y"].dtype == torch.float32 and not torch.equal(E.rne(dyf).double(), dyf)
    check_all(standin(c, out_f32=True, dy_f32=dyf), ref)


def test_standin_passes_padded_image():
    """conv_in: 3 weight channels, an input padded to 8 zero channels"""
    c = E.make_case("A", 0, 2, 3, 36, 9, 17, True, False, cx=8)
    assert tuple(c["x"].shape) == (2, 8, 9, 17)
    E.assert_exactly_summable(c)
    check_all(standin(c), E.references(c))


def test_recipes_exercise_the_rounding():
    """a fair share of recipe A's and B's outputs are no bf16 numbers, and some are exact ties: the store's rounding is on trial"""
    for recipe, spec, tie_min in (("A", CASES["A"][0], 0.1), ("B", CASES["B"][0], 0.005)):
        ref = E.references(E.make_case(recipe, *spec))
        inexact, ties = E.rounding_profile(ref["y_exact"])
        assert inexact > 0.3 and ties > tie_min, (recipe, inexact, ties)


# ------------------------------------------------------------------------------------------------------------------------------
# mutants: every one of these must be rejected
# ------------------------------------------------------------------------------------------------------------------------------
def _case(recipe, i=0, **kw):
    c = E.make_case(recipe, *CASES[recipe][i], **kw)
    E.assert_exactly_summable(c)
    return c, E.references(c)


def _live_channel(c, n, py, px):
    """an input channel whose value at this pixel is not zero (dropping a zero term is no fault)"""
    return int((c["x"][n, :, py, px] != 0).nonzero()[0])


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_truncation_at_the_store_must_fail(recipe):
    c, ref = _case(recipe)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="truncate")["y"], ref["y"], "y")
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="truncate")["dx"], ref["dx"], "dx")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_round_half_away_must_fail(recipe):
    c, ref = _case(recipe)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="half_away")["y"], ref["y"], "y")
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="half_away")["dx"], ref["dx"], "dx")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_bf16_round_trip_of_the_accumulator_must_fail(recipe):
    c, ref = _case(recipe)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="acc_roundtrip")["y"], ref["y"], "y")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_term_dropped_at_a_corner_pixel_must_fail(recipe):
    c, ref = _case(recipe)
    h, w = c["x"].shape[2:]
    at = (0, _live_channel(c, 0, h - 1, w - 1), h - 1, w - 1, 1, 1)
    with pytest.raises(AssertionError, match="on the image border"):
        E.assert_bits_equal(standin(c, fault="drop_term", at=at)["y"], ref["y"], "y")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_term_dropped_at_an_interior_tile_seam_must_fail(recipe):
    c, ref = _case(recipe)
    at = (1, _live_channel(c, 1, 7, 15), 8, 16, 0, 0)       # output (8, 16), the first pixel of a tile, reads input (7, 15) of the tile before
    with pytest.raises(AssertionError, match="[1-9][0-9]* on a tile seam"):
        E.assert_bits_equal(standin(c, fault="drop_term", at=at)["y"], ref["y"], "y")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_term_dropped_in_the_last_channel_of_a_ragged_cin_must_fail(recipe):
    c, ref = _case(recipe)
    cin = c["w"].shape[1]
    assert cin % 32 != 0
    n, py, px = (int(v) for v in (c["x"][:, cin - 1] != 0).nonzero()[3])
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="drop_term", at=(n, cin - 1, py, px, 1, 1))["y"], ref["y"], "y")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_tap_wraps_at_the_right_border_must_fail(recipe):
    c, ref = _case(recipe)
    with pytest.raises(AssertionError, match="on the image border"):
        E.assert_bits_equal(standin(c, fault="wrap_right")["y"], ref["y"], "y")


def test_mutant_operand_loses_its_lowest_significand_bit_must_fail():
    """recipe B's reason to exist; recipe A (integers up to 4: three bits) cannot see this fault"""
    c, ref = _case("B")
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="operand_low_bit")["y"], ref["y"], "y")
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="operand_low_bit")["dw"], ref["dw"], "dw")
    ca, refa = _case("A")
    check_all(standin(ca, fault="operand_low_bit"), refa)


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_second_rounding_of_the_upsample_gradient_omitted_must_fail(recipe):
    c, ref = _case(recipe, 2)
    assert c["mode"] == 2
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="skip_second_rounding")["dx"], ref["dx"], "dx")


@pytest.mark.parametrize("recipe", ["A", "B"])
def test_mutant_pixel_row_left_out_of_dw_must_fail(recipe):
    c, ref = _case(recipe)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(standin(c, fault="dw_row", at=c["dy"].shape[2] - 1)["dw"], ref["dw"], "dw")


@pytest.mark.parametrize("recipe", ["A", "B"])
@pytest.mark.parametrize("out_f32", [False, True])
def test_mutant_nan_in_one_output_element_must_fail(recipe, out_f32):
    c = E.make_case(recipe, *CASES[recipe][0])
    ref = E.references(c, out_f32=out_f32)
    with pytest.raises(AssertionError, match="1 of"):
        E.assert_bits_equal(standin(c, out_f32=out_f32, fault="nan", at=(1, 2, 3, 4))["y"], ref["y"], "y")


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_mutant_cast_that_drops_the_sign_of_zero_must_fail(dtype):
    """casts are compared raw (summed=False); for sums the sign of an exact zero is no fault"""
    want = torch.tensor([1.0, -0.0, 0.0, -2.5], dtype=dtype)
    got = torch.tensor([1.0, 0.0, 0.0, -2.5], dtype=dtype)
    E.assert_bits_equal(want.clone(), want, "cast", summed=False)
    with pytest.raises(AssertionError, match="1 of 4"):
        E.assert_bits_equal(got, want, "cast", summed=False)
    E.assert_bits_equal(got, want, "sum", summed=True)


def test_checker_rejects_dtype_and_shape_mismatch():
    a = torch.zeros(2, 4, dtype=BF)
    with pytest.raises(AssertionError, match="dtype"):
        E.assert_bits_equal(a.float(), a, "t")
    with pytest.raises(AssertionError, match="shape"):
        E.assert_bits_equal(a.reshape(4, 2), a, "t")


# ------------------------------------------------------------------------------------------------------------------------------
# the precondition must be able to fail too
# ------------------------------------------------------------------------------------------------------------------------------
def test_summability_rejects_recipe_b_at_512_channels():
    c = E.make_case("B", 0, 1, 512, 8, 4, 4)
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        E.assert_exactly_summable(c)


def test_summability_rejects_operands_that_are_no_bf16_numbers():
    c = E.make_case("A", 0, 1, 8, 8, 4, 4)
    c["x"][0, 0, 0, 0] = 257.0       # nine significant bits
    with pytest.raises(AssertionError, match="not made of bf16 numbers"):
        E.assert_exactly_summable(c)
    c = E.make_case("A", 0, 1, 8, 8, 4, 4)
    c["w"][0, 0, 0, 0] = 2.0 ** -5   # a bf16 number, but finer than the recipe's unit
    with pytest.raises(AssertionError, match="multiples of"):
        E.assert_exactly_summable(c)


def test_summability_rejects_statistics_that_do_not_fit():
    """recipe A is fine for the conv itself, but the sums of y and y^2 over a tile and group pass 2^24 units"""
    c = E.make_case("A", 0, 1, 512, 128, 8, 16)
    E.assert_exactly_summable(c)
    with pytest.raises(AssertionError, match="stats_sum"):
        E.assert_exactly_summable(c, stats_groups=8)
