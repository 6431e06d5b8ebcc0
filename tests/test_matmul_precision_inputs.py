"""float32_matmul_precision, host side: the level references of tests/matmul_precision_inputs.py (what each recipe must give at each
level, and that the acceptance rule of the GPU tests rejects planted faults), and the public surface -- Python API, environment,
`torch` mode, Trainer, header and binding.  No device."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import gemm_exact_inputs as G
import matmul_precision_inputs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(132, 200, 1024, 2), (132, 200, 1051, 2)]      # M, N, K, batch: the ragged shape of G.SPLIT_CASES, whole and partial last step
_CASES = {}


def case(recipe, shape=SHAPES[1]):
    key = (recipe,) + shape
    if key not in _CASES:
        c = G.make_case(recipe, *shape)
        G.assert_exactly_summable(c)
        if recipe != "A":
            G.assert_planes(c)
        _CASES[key] = c
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------
def test_kept_products_are_suffixes_of_the_kernel_order():
    assert P.KEPT[1] == P.KEPT[0][3:] and P.KEPT[2] == P.KEPT[0][5:]
    assert set(P.KEPT[1]) == {(p, q) for p in (P.HI, P.MID) for q in (P.HI, P.MID)} - {(P.MID, P.MID)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("recipe", G.SPLIT_RECIPES)
def test_kept_partial_sums_stay_below_the_limit(recipe, shape):
    c = case(recipe, shape)
    for level in P.LEVELS:
        assert P.assert_level_summable(c, level) < G.LIMIT
    assert torch.equal(P.level_reference(c, 0), G.reference(c)), "level 0 is the float64 product on every split recipe"


def test_recipe_a_is_the_same_at_every_level():
    c = case("A")
    assert torch.equal(P.level_reference(c, 1), G.reference(c)) and torch.equal(P.level_reference(c, 2), G.reference(c))


def test_recipe_s1_is_exact_at_high_and_hi_a_times_b_at_medium():
    c = case("S1")
    (a_hi, a_mid, a_lo), _ = P.planes(c)
    assert torch.equal(P.level_reference(c, 1), G.reference(c))
    assert torch.equal(P.level_reference(c, 2), torch.matmul(a_hi, c["b"]))
    assert not torch.equal(P.level_reference(c, 2), G.reference(c)) and a_mid.abs().max() > 0 and a_lo.abs().max() == 0


def test_recipe_s2_loses_mid_mid_at_high():
    c = case("S2")
    (a_hi, a_mid, _), (b_hi, b_mid, _) = P.planes(c)
    mm = torch.matmul(a_mid, b_mid)
    assert mm.abs().max() > 0
    assert torch.equal(P.level_reference(c, 1), G.reference(c) - mm)
    assert torch.equal(P.level_reference(c, 2), torch.matmul(a_hi, b_hi))


@pytest.mark.parametrize("recipe", ["S3", "S3T"])
def test_recipes_s3_lose_their_lo_terms_at_both_new_levels(recipe):
    c = case(recipe)
    (a_hi, a_mid, a_lo), (b_hi, b_mid, b_lo) = P.planes(c)
    lo_term = torch.matmul(a_lo, b_hi) if recipe == "S3" else torch.matmul(a_hi, b_lo)
    mid_term = torch.matmul(a_mid, b_hi) if recipe == "S3" else torch.matmul(a_hi, b_mid)
    assert lo_term.abs().max() > 0 and mid_term.abs().max() > 0
    assert torch.equal(P.level_reference(c, 1), G.reference(c) - lo_term)
    assert torch.equal(P.level_reference(c, 2), G.reference(c) - lo_term - mid_term)


# ------------------------------------------------------------------------------------------------------------------------------
# the acceptance rule against planted faults
# ------------------------------------------------------------------------------------------------------------------------------
def _f32(t):
    assert torch.equal(t.float().double(), t), "the planted result is not made of f32 numbers"
    return t.float()


def test_rule_accepts_the_level_reference_and_nothing_from_another_level():
    for recipe in G.SPLIT_RECIPES:
        c = case(recipe)
        refs = [_f32(P.level_reference(c, level)) for level in P.LEVELS]
        for level in P.LEVELS:
            assert P.accepts(refs[level], c, level)
            for other in P.LEVELS:
                same = torch.equal(refs[other], refs[level])
                assert P.accepts(refs[other], c, level) == same
        if recipe != "A":
            assert not P.accepts(refs[0], c, 2), "the highest result passed as medium on recipe %s" % recipe


def test_rule_rejects_mid_mid_kept_at_high():
    c = case("S2")
    pa, pb = P.planes(c)
    assert not P.accepts(_f32(P.sum_of_pairs(pa, pb, P.KEPT[1] + ((P.MID, P.MID),))), c, 1)


def test_rule_rejects_hi_mid_dropped_at_high():
    c = case("S2")
    pa, pb = P.planes(c)
    assert not P.accepts(_f32(P.sum_of_pairs(pa, pb, ((P.MID, P.HI), (P.HI, P.HI)))), c, 1)
    c = case("S1")      # ... and its mirror image, a_mid b_hi dropped
    pa, pb = P.planes(c)
    assert not P.accepts(_f32(P.sum_of_pairs(pa, pb, ((P.HI, P.MID), (P.HI, P.HI)))), c, 1)


def test_rule_rejects_a_truncated_mid():
    """S3 / S3T carry 18-bit odd integers: x - hi has up to ten significant bits, so the mid plane IS rounded (S1 and S2 fit theirs)."""
    for recipe, which in (("S3", "a"), ("S3T", "b")):
        c = case(recipe)
        pa, pb = P.planes(c)
        chopped = P.truncated_mid(c[which])
        assert not torch.equal(chopped, (pa if which == "a" else pb)[P.MID]), "truncation changes nothing on recipe %s" % recipe
        if which == "a":
            pa = (pa[0], chopped, pa[2])
        else:
            pb = (pb[0], chopped, pb[2])
        assert not P.accepts(_f32(P.sum_of_pairs(pa, pb, P.KEPT[1])), c, 1)


def test_rule_rejects_exchanged_planes():
    """The kept sets are symmetric in (A plane, B plane), so handing A's list to B is no fault.  Exchanged planes are: the hi and mid
    planes of one operand taken for each other (a fragment address off by one plane), or the mid plane where medium wants hi."""
    c = case("S2")
    pa, pb = P.planes(c)
    assert not P.accepts(_f32(P.sum_of_pairs((pa[1], pa[0], pa[2]), pb, P.KEPT[1])), c, 1)
    assert not P.accepts(_f32(P.sum_of_pairs(pa, (pb[1], pb[0], pb[2]), P.KEPT[1])), c, 1)
    for recipe in ("S1", "S3T"):      # one operand has a mid plane, the other none: A's planes given to B and B's to A, plane by plane
        c = case(recipe)
        pa, pb = P.planes(c)
        one_sided = ((P.MID, P.HI), (P.HI, P.HI)) if recipe == "S3T" else ((P.HI, P.MID), (P.HI, P.HI))
        assert not P.accepts(_f32(P.sum_of_pairs(pa, pb, one_sided)), c, 1)
        assert not P.accepts(_f32(torch.matmul(pa[P.MID], pb[P.HI]) if recipe == "S1" else torch.matmul(pa[P.HI], pb[P.MID])), c, 2)


def test_error_bounds_follow_from_the_planes():
    b = P.rel_err_bounds()
    assert b[0] == 2.0 ** -22 and b[1] <= 2.0 ** -14 and b[2] <= 2.0 ** -6
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1 << 16, generator=g).double()
    hi, mid, lo = G.split3(x)
    assert (mid.abs() <= 2.0 ** -8 * x.abs()).all() and (lo.abs() <= 2.0 ** -16 * x.abs()).all() and (hi.abs() <= (1 + 2.0 ** -8) * x.abs()).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the public surface
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ops():
    """the op layer with the setting, the pushed level, the library's level and torch's own setting put back afterwards"""
    from odvae_amd import lib, ops
    mode, pushed, torch_mode = ops.FLOAT32_MATMUL_PRECISION, ops._MATMUL_LEVEL_PUSHED, torch.get_float32_matmul_precision()
    level = 0      # what the library holds now (it loads at 0; a test of this process may have loaded it and set something)
    if lib._lib is not None:
        level = lib._lib.odvae_gemm_select_precision(0)
        lib._lib.odvae_gemm_select_precision(level)
    try:
        yield ops
    finally:
        ops.FLOAT32_MATMUL_PRECISION, ops._MATMUL_LEVEL_PUSHED = mode, pushed
        torch.set_float32_matmul_precision(torch_mode)
        if lib._lib is not None:
            lib._lib.odvae_gemm_select_precision(level)


class _Recorder(object):
    """stands in for the library handle: records what the op layer pushes"""

    def __init__(self):
        self.pushed = []

    def odvae_gemm_select_precision(self, level):
        self.pushed.append(level)
        return 0


def test_default_is_highest(ops):
    if "ODVAE_FLOAT32_MATMUL_PRECISION" not in os.environ:
        assert ops.FLOAT32_MATMUL_PRECISION == "highest" and ops._matmul_level() == 0


def test_set_get_round_trip(ops):
    import odvae_amd
    for name in ("high", "medium", "torch", "highest"):
        odvae_amd.set_float32_matmul_precision(name)
        assert odvae_amd.get_float32_matmul_precision() == name == ops.get_float32_matmul_precision() == ops.FLOAT32_MATMUL_PRECISION
    ops.set_float32_matmul_precision(" Medium ")
    assert ops.get_float32_matmul_precision() == "medium" and ops._matmul_level() == 2


@pytest.mark.parametrize("bad", ["tf32", "bf16", "low", "", "highest,high", 1, 2.0, None, ("high",)], ids=repr)
def test_a_bad_name_raises_and_changes_nothing(ops, bad):
    ops.set_float32_matmul_precision("high")
    rec = _Recorder()
    ops._sync_precision(rec)
    with pytest.raises(ValueError, match="float32_matmul_precision"):
        ops.set_float32_matmul_precision(bad)
    assert ops.get_float32_matmul_precision() == "high" and ops._matmul_level() == 1
    ops._sync_precision(rec)
    assert rec.pushed in ([], [1]) and ops._MATMUL_LEVEL_PUSHED == 1


def test_environment_values_parse(ops):
    assert [ops._parse_matmul_precision(v) for v in ("highest", "HIGH", " medium", "Torch\n")] == ["highest", "high", "medium", "torch"]
    assert ops.MATMUL_PRECISION_VALUES == ("highest", "high", "medium", "torch") and ops.MATMUL_PRECISION_LEVELS == {"highest": 0, "high": 1, "medium": 2}
    for bad in ("tf32", "0", "high est", ""):
        with pytest.raises(ValueError):
            ops._parse_matmul_precision(bad)


def test_environment_variable_is_read_at_import():
    """(a fresh interpreter: the switch table is read once, at import)"""
    code = "from odvae_amd import ops; print(ops.FLOAT32_MATMUL_PRECISION, ops._matmul_level())"
    env = dict(os.environ, ODVAE_FLOAT32_MATMUL_PRECISION=" Medium", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.split() == ["medium", "2"], out.stderr[-2000:]
    env["ODVAE_FLOAT32_MATMUL_PRECISION"] = "tf32"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode != 0 and "ODVAE_FLOAT32_MATMUL_PRECISION" in out.stderr and "tf32" in out.stderr


def test_torch_mode_maps_the_three_names_and_tracks_a_change(ops):
    ops.set_float32_matmul_precision("torch")
    rec = _Recorder()
    ops._MATMUL_LEVEL_PUSHED = 0
    want = []
    for name, level in (("medium", 2), ("medium", 2), ("high", 1), ("highest", 0), ("highest", 0), ("medium", 2)):
        torch.set_float32_matmul_precision(name)
        assert ops._matmul_level() == level
        ops._sync_precision(rec)
        ops._sync_precision(rec)      # a second call at the same level tells the library nothing
        if not want or want[-1] != level:
            want.append(level)
        assert rec.pushed == want and ops._MATMUL_LEVEL_PUSHED == level
    assert want == [2, 1, 0, 2]
    # the default does not follow torch
    ops.set_float32_matmul_precision("highest")
    torch.set_float32_matmul_precision("medium")
    assert ops._matmul_level() == 0


def test_a_fixed_level_is_pushed_where_it_changes(ops):
    rec = _Recorder()
    ops.FLOAT32_MATMUL_PRECISION, ops._MATMUL_LEVEL_PUSHED = "highest", 0
    ops._sync_precision(rec)
    assert rec.pushed == []
    ops.FLOAT32_MATMUL_PRECISION = "high"      # set on the package, as a monkeypatch would
    ops._sync_precision(rec)
    ops._sync_precision(rec)
    assert rec.pushed == [1]


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = nn.Linear(4, 4)
        self.learning_rate = 1e-3

    def configure_optimizers(self):
        return [torch.optim.Adam(self.parameters(), lr=self.learning_rate)], []


def test_trainer_none_touches_nothing_and_a_name_sets_it(ops):
    from odvae_amd.trainer import Trainer
    ops.set_float32_matmul_precision("medium")
    pushed = ops._MATMUL_LEVEL_PUSHED
    Trainer(_Tiny(), optimizer_indices=(0,), distributed=False)
    Trainer(_Tiny(), optimizer_indices=(0,), distributed=False, float32_matmul_precision=None)
    assert ops.get_float32_matmul_precision() == "medium" and ops._MATMUL_LEVEL_PUSHED == pushed
    Trainer(_Tiny(), optimizer_indices=(0,), distributed=False, float32_matmul_precision="high")
    assert ops.get_float32_matmul_precision() == "high"      # process-global, like torch's: it outlives the trainer
    with pytest.raises(ValueError, match="float32_matmul_precision"):
        Trainer(_Tiny(), optimizer_indices=(0,), distributed=False, float32_matmul_precision="tf32")
    assert ops.get_float32_matmul_precision() == "high"


def test_runner_takes_the_flag():
    from odvae_amd import run
    assert run.parse([])[0].float32_matmul_precision is None
    assert run.parse(["--float32_matmul_precision", "medium"])[0].float32_matmul_precision == "medium"
    with pytest.raises(SystemExit):
        run.parse(["--float32_matmul_precision", "tf32"])


def test_header_declares_the_entry_point_and_lib_binds_it():
    import ctypes
    from odvae_amd import lib
    assert lib.PROTOTYPES["odvae_gemm_select_precision"] == (ctypes.c_int, [ctypes.c_int])
    assert lib.PROTOTYPES["odvae_gemm_select_precision"] == lib.PROTOTYPES["odvae_gemm_select_staging"]
    assert lib.ABI_VERSION == 4


def test_library_loads_at_level_0_and_clamps():
    """(a fresh interpreter: the level is process-global, and other tests of this process may have loaded the library)"""
    code = ("from odvae_amd import lib; L = lib.load(); s = L.odvae_gemm_select_precision; "
            "print(s(1), s(7), s(-3), s(2), s(0), s(0))")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.split() == ["0", "1", "2", "0", "2", "0"], out.stderr[-2000:]
