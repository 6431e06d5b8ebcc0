"""float32_matmul_precision on the device: the bf16-split kernel (gemm_f32_split.hip) at one, two and three planes.

1. bit for bit: G.SPLIT_CASES x G.SPLIT_RECIPES at every level must EQUAL tests/matmul_precision_inputs.level_reference where the mirror
   of the dispatch says the split kernel runs, and float64 where it says the f32 kernels do (the level must not reach those);
2. the same through the three epilogues (ROWNORM, SMB, EXPB) with the acceptance tests/test_gemm_f32_exact_gpu.py applies to each;
3. the error bound e_L <= e_f32 + b_L on random-normal and softmax-like operands (b_L: matmul_precision_inputs.rel_err_bounds);
4. the level takes effect above the gate, nowhere else, and is deterministic;
5. Inf and NaN operands never come out finite, and touch nothing but their rows and columns;
6. through the op layer: ops.attention_qkv forward and backward, the level set from Python, from C and by a Trainer.
Every test that sets a level puts the previous one back (`precision`, `finally`); `level_is_back` checks it after every test."""
import pytest
import torch
import torch.nn as nn

import gemm_exact_inputs as G
import matmul_precision_inputs as P
import test_gemm_f32_exact_gpu as X      # the poisoned-layout launcher of the exact GEMM tests, as it is
import test_gemm_split_gpu as S          # the packed-operand launcher and the error measure of the split GEMM tests, as they are

pytestmark = pytest.mark.gpu
DEV = X.DEV


class precision(object):
    """odvae_gemm_select_precision(level) for the length of a `with`"""

    def __init__(self, lib, level):
        self.lib, self.level = lib, level

    def __enter__(self):
        self.prev = self.lib.odvae_gemm_select_precision(self.level)

    def __exit__(self, *exc):
        self.lib.odvae_gemm_select_precision(self.prev)


@pytest.fixture(autouse=True)
def level_is_back(hip_lib):
    yield
    from odvae_amd import ops
    left = hip_lib.odvae_gemm_select_precision(0)
    assert left == 0 and ops.FLOAT32_MATMUL_PRECISION == "highest" and ops._MATMUL_LEVEL_PUSHED == 0, "a test left a level behind"


def _refs(c):
    refs = P.level_references(c)
    for r in refs:
        assert torch.equal(r.float().double(), r), "a level reference is not made of f32 numbers"
    return refs


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the plain product
# ------------------------------------------------------------------------------------------------------------------------------
def test_library_level_defaults_to_highest_and_clamps(hip_lib):
    s = hip_lib.odvae_gemm_select_precision
    assert [s(1), s(9), s(-4), s(0)] == [0, 1, 2, 0]


@pytest.mark.parametrize("recipe", G.SPLIT_RECIPES)
@pytest.mark.parametrize("case", G.SPLIT_CASES, ids=X._id)
def test_deep_product_equals_the_level_reference(hip_lib, case, recipe):
    layout, m, n, k, batch, shared = case
    c = G.make_case(recipe, m, n, k, batch, shared_b=shared)
    G.assert_exactly_summable(c)      # all nine plane pairs: an upper bound of every level's kept sum
    if recipe != "A":
        G.assert_planes(c)
    refs = _refs(c)
    assert torch.equal(refs[0], G.reference(c))
    split = ("split", layout, "none") in G.gemm_forms(layout, m, n, k, batch, -1)
    run = X.Launch(hip_lib, layout, c)
    for level in P.LEVELS:
        with precision(hip_lib, level):
            out, before = run.gemm(-1)
            run.check(out, before, refs[level] if split else refs[0], "%s %s level %d (%s)" % (X._id(case), recipe, level, "split" if split else "f32 kernels"))
            if level and split:       # a forced staging mode still means the f32 MFMA kernel
                out, before = run.gemm(1)
                run.check(out, before, refs[0], "%s %s level %d staging 1" % (X._id(case), recipe, level))


def test_the_cases_reach_a_partial_last_step_at_every_layout():
    split = [(l, k, b) for l, m, n, k, b, s in G.SPLIT_CASES if ("split", l, "none") in G.gemm_forms(l, m, n, k, b, -1)]
    assert {(l, k % 32 != 0) for l, k, b in split} == {("NN", False), ("NN", True), ("TN", False), ("TN", True)}


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the epilogues
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.ROWNORM_CASES[1:], ids=X._id)
def test_rownorm_equals_the_level_reference(hip_lib, case):
    """The row sums come from the unsplit f32 values at every level: 1 / l is the same bits, the product is the level's.  The last
    element of every row of A (what makes the row sum a power of two) is wider than a bf16: the levels differ."""
    from odvae_amd import lib as _lib
    m, n, k, batch, shared = case
    c = G.make_rownorm_case(m, n, k, batch, shared_b=shared)
    l = G.assert_rownorm_exact(c)
    refs = [r / l[:, :, None] for r in _refs(c)]
    assert torch.equal(refs[0], torch.matmul(c["a"], c["b"]) / l[:, :, None]) and not torch.equal(refs[2], refs[0])
    split = G.rownorm_forms(m, n, k, batch, -1) == {("split", "NN", "rownorm")}
    run = X.Launch(hip_lib, "NN", c)
    erow = G.Embedded(batch, 1, m)
    for level in P.LEVELS:
        out, before = X.output(run.ec)
        rinv, rinv0 = X.output(erow)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        with precision(hip_lib, level):
            _lib.check(hip_lib.odvae_gemm_rownorm_f32(m, n, k, X.ptr(run.a), run.ea.ld, run.ea.stride, X.ptr(run.b), run.eb.ld, run.eb.stride,
                                                      X.ptr(out), run.ec.ld, run.ec.stride, X.ptr(rinv), erow.stride, flag.data_ptr(), batch,
                                                      _lib.stream_ptr()), "gemm_rownorm")
        torch.cuda.synchronize()
        what = "%s level %d (%s)" % (X._id(case), level, "split" if split else "f32 kernel")
        assert int(flag.item()) == 0, what
        run.check(out, before, refs[level] if split else refs[0], what)
        G.assert_bits_equal(X.logical(erow, rinv), (1.0 / l).float()[:, None, :], what + ": 1 / l", summed=False)
        X.assert_untouched_outside(erow, rinv, rinv0, what + ": 1 / l")


def _smb_case(m, n, k, batch, scaled, wide):
    """G.make_smb_case (recipe A: one plane, every level the same answer), or the same with A made of odd integers up to 1023 -- ten
    bits, a hi and a mid plane: `high` still equals float64, `medium` is hi(a) b."""
    c = G.make_smb_case(m, n, k, batch, scaled)
    if wide:
        c["a"] = G._odd(torch.Generator().manual_seed(77 + k), (batch, m, k), 1023)
    G.assert_smb_exact(c)
    return c


@pytest.mark.parametrize("wide", [False, True], ids=["recipeA", "wideA"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_softmax_backward_tail_equals_the_level_reference(hip_lib, scaled, wide):
    from odvae_amd import lib as _lib
    m, n, k, batch = shape = G.TT_SHAPES[1]
    assert G.smb_forms(m, n, k, batch, -1) == {("split", "NT", "smb")}
    c = _smb_case(m, n, k, batch, scaled, wide)
    refs = [P.smb_level_reference(c, level) for level in P.LEVELS]
    for r in refs:
        assert torch.equal(r.float().double(), r)
    assert torch.equal(refs[0], G.smb_reference(c)) and torch.equal(refs[1], refs[0]) and torch.equal(refs[2], refs[0]) == (not wide)
    run = X.Launch(hip_lib, "NT", c)
    erow = G.Embedded(batch, 1, m)
    rowdot = X.row_vector(erow, c["rowdot"])
    rowmul = X.row_vector(erow, c["rowmul"]) if scaled else None
    for level in P.LEVELS:
        p, p0 = X.output(run.ec, c["p"])
        out, before = X.output(run.ec)
        with precision(hip_lib, level):
            if scaled:
                rc = hip_lib.odvae_gemm_softmax_bwd_scaled_f32(m, n, k, c["alpha"], X.ptr(run.a), run.ea.ld, run.ea.stride, X.ptr(run.b), run.eb.ld,
                                                               run.eb.stride, X.ptr(p), X.ptr(rowdot), X.ptr(rowmul), erow.stride, X.ptr(out), run.ec.ld,
                                                               run.ec.stride, batch, _lib.stream_ptr())
            else:
                rc = hip_lib.odvae_gemm_softmax_bwd_f32(m, n, k, c["alpha"], X.ptr(run.a), run.ea.ld, run.ea.stride, X.ptr(run.b), run.eb.ld, run.eb.stride,
                                                        X.ptr(p), X.ptr(rowdot), erow.stride, X.ptr(out), run.ec.ld, run.ec.stride, batch, _lib.stream_ptr())
        _lib.check(rc, "gemm_softmax_bwd")
        torch.cuda.synchronize()
        what = "%s level %d" % (X._id(shape), level)
        run.check(out, before, refs[level], what)
        X.assert_unchanged(p, p0, what)


def test_exp_bound_tail_at_every_level(hip_lib):
    """Integer scores from one-plane operands: score == bound gives 1.0, far below gives 0.0, and the columns in between the same
    exp2 of the same exact argument at every level."""
    from odvae_amd import lib as _lib
    m, n, k, batch = shape = G.TT_SHAPES[1]
    assert G.expb_forms(m, n, k, batch, -1) == {("split", "NT", "expb")}
    c = G.make_expb_case(m, n, k, batch)
    G.assert_expb_exact(c)
    for name in ("a", "b"):
        assert torch.equal(c[name].float().to(G.BF).double(), c[name])
    run = X.Launch(hip_lib, "NT", c)
    erow = G.Embedded(batch, 1, m)
    bound = X.row_vector(erow, c["bound"])
    cls = c["cls"].to(DEV)
    near = []
    for level in P.LEVELS:
        out, before = X.output(run.ec)
        with precision(hip_lib, level):
            _lib.check(hip_lib.odvae_gemm_exp_bound_f32(m, n, k, c["alpha"], X.ptr(run.a), run.ea.ld, run.ea.stride, X.ptr(run.b), run.eb.ld, run.eb.stride,
                                                        X.ptr(bound), erow.stride, X.ptr(out), run.ec.ld, run.ec.stride, batch, _lib.stream_ptr()),
                       "gemm_exp_bound")
        torch.cuda.synchronize()
        what = "%s level %d" % (X._id(shape), level)
        got = X.logical(run.ec, out)
        one, far = got[:, :, cls == 0], got[:, :, cls == 1]
        G.assert_bits_equal(one, torch.ones_like(one), what + ": score == bound", summed=False)
        G.assert_bits_equal(far, torch.zeros_like(far), what + ": score far below the bound", summed=False)
        near.append(got[:, :, cls == 2])
        assert torch.isfinite(near[-1]).all() and (near[-1] > 0).all()
        X.assert_untouched_outside(run.ec, out, before, what)
    for level in (1, 2):
        G.assert_bits_equal(near[level], near[0], "%s: level %d disagrees with highest on exp of a small difference" % (X._id(shape), level), summed=False)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the bound, 4. the level takes effect and is contained
# ------------------------------------------------------------------------------------------------------------------------------
# (M, N, K) at S.BATCH = 8, small shapes the mirror admits: K = 1024 opens the gate at any tile count (16 tiles x 8 here); past it
# choose_splits must say 1, which 5 x 8 tiles x 8 = 320 do at K = 1052 (512 / 320 = 1) and 5 x 5 x 8 = 200 would not.  The second
# has tails on every axis and K % 32 != 0.
SMALL_FULL = (512, 512, 1024)
SMALL_RAGGED = (600, 904, 1052)
BELOW = (512, 512, 512)


def test_the_bound_shapes_open_the_gate():
    for m, n, k in (SMALL_FULL, SMALL_RAGGED):
        assert G.split_eligible(-1, 0, m, n, k, S.BATCH) and not G.split_eligible(1, 0, m, n, k, S.BATCH)
    assert not G.split_eligible(-1, 0, 600, 904 - 3 * 128, 1052, S.BATCH)
    assert not G.split_eligible(-1, 0, *BELOW, S.BATCH)


def _levels(hip_lib, form, shape, a_d, packed_d, staging=-1, levels=P.LEVELS):
    n = shape[1]
    out = []
    for level in levels:
        with precision(hip_lib, level):
            out.append(S.run_gemm(hip_lib, form, shape, a_d, packed_d, staging)[:, :, n:2 * n])
    return out


@pytest.mark.parametrize("kind", ["normal", "softmax"])
@pytest.mark.parametrize("shape", [SMALL_FULL, SMALL_RAGGED], ids=["full", "ragged"])
@pytest.mark.parametrize("form", ["NN", "TN"])
def test_error_stays_within_the_level_bound(hip_lib, form, shape, kind):
    m, n, k = shape
    a, packed = S.make_case(form, shape, kind, seed=m + 3 * k + (form == "TN") + 7 * (kind == "softmax"))
    a_d, packed_d = a.to(DEV), packed.to(DEV)
    outs = _levels(hip_lib, form, shape, a_d, packed_d)
    out_f32 = S.run_gemm(hip_lib, form, shape, a_d, packed_d, staging=1)[:, :, n:2 * n]
    c64, scale = S.reference(form, shape, a, packed)
    e_f32 = S.rel_err(out_f32, c64, scale)
    e = [S.rel_err(o, c64, scale) for o in outs]
    b = P.rel_err_bounds()
    print("\nmatmul_precision accuracy %s %s M=%d N=%d K=%d batch=%d: e_f32 %.3e  e_highest %.3e  e_high %.3e (bound %.3e)  e_medium %.3e (bound %.3e)"
          % (form, kind, m, n, k, S.BATCH, e_f32, e[0], e[1], e_f32 + b[1], e[2], e_f32 + b[2]))
    for level in P.LEVELS:
        assert torch.isfinite(outs[level]).all()
        assert e[level] <= e_f32 + b[level], "level %d" % level


@pytest.mark.parametrize("form", ["NN", "TN"])
def test_level_takes_effect_above_the_gate_and_nowhere_else(hip_lib, form):
    a, packed = S.make_case(form, SMALL_RAGGED, "normal", seed=31)
    a_d, packed_d = a.to(DEV), packed.to(DEV)
    outs = _levels(hip_lib, form, SMALL_RAGGED, a_d, packed_d)
    again = _levels(hip_lib, form, SMALL_RAGGED, a_d, packed_d)
    for level in P.LEVELS:
        assert torch.equal(outs[level].view(torch.int32), again[level].view(torch.int32)), "two runs at level %d differ" % level
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(outs[i], outs[j]), "levels %d and %d give the same bits above the gate" % (i, j)
    forced = _levels(hip_lib, form, SMALL_RAGGED, a_d, packed_d, staging=1)
    assert torch.equal(forced[0], forced[1]) and torch.equal(forced[0], forced[2]), "the level reached the f32 MFMA kernel (forced staging)"
    assert not torch.equal(forced[0], outs[0])
    a, packed = S.make_case(form, BELOW, "normal", seed=32)
    below = _levels(hip_lib, form, BELOW, a.to(DEV), packed.to(DEV))
    assert torch.equal(below[0], below[1]) and torch.equal(below[0], below[2]), "the level reached a product below the gate (K = 512)"


def test_level_is_contained_below_the_tile_count(hip_lib):
    """K = 1028 at two batches: choose_splits says 2, the f32 kernels and the split-K reduce run -- at every level the same bits."""
    layout, m, n, k, batch = "NN", 132, 200, 1028, 2
    assert ("split", layout, "none") not in G.gemm_forms(layout, m, n, k, batch, -1)
    g = torch.Generator().manual_seed(5)
    c = {"a": torch.randn(batch, m, k, generator=g).double(), "b": torch.randn(batch, k, n, generator=g).double(), "alpha": 1.0}
    run = X.Launch(hip_lib, layout, c)
    got = []
    for level in P.LEVELS:
        with precision(hip_lib, level):
            got.append(X.logical(run.ec, run.gemm(-1)[0]))
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)) and torch.equal(got[0].view(torch.int32), got[2].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. non-finite operands
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", P.LEVELS)
@pytest.mark.parametrize("form", ["NN", "TN"])
def test_non_finite_operands_never_come_out_finite(hip_lib, form, level):
    """In A: the whole row of its batch.  In B: the whole column of its batch.  At highest and high an Inf splits into hi = Inf and
    x - hi = NaN; at medium it stays Inf, and Inf times a finite non-zero number is Inf.  Everything else keeps its bits."""
    shape = SMALL_RAGGED
    m, n, k = shape
    a, packed = S.make_case(form, shape, "normal", seed=41)
    with precision(hip_lib, level):
        clean = S.run_gemm(hip_lib, form, shape, a.to(DEV), packed.to(DEV))[:, :, n:2 * n]
    rows = {"nan": (0, 77, 1000, float("nan")), "inf": (3, m - 1, 31, float("inf")), "-inf": (7, 130, k - 1, float("-inf"))}
    cols = {"nan": (1, 5, 3, float("nan")), "inf": (4, k - 2, n - 1, float("inf")), "-inf": (6, 700, 129, float("-inf"))}
    for b, row, kk, val in rows.values():
        if form == "TN":
            a[b, kk, row] = val
        else:
            a[b, row, kk] = val
    for b, kk, col, val in cols.values():
        packed[b, kk, 2 * n + col] = val
    with precision(hip_lib, level):
        out = S.run_gemm(hip_lib, form, shape, a.to(DEV), packed.to(DEV))[:, :, n:2 * n]
    assert torch.isfinite(clean).all()
    same = out.view(torch.int32) == clean.view(torch.int32)
    finite = torch.isfinite(out)
    for what, (b, row, kk, val) in rows.items():
        assert not finite[b, row].any(), "level %d: %s in A[%d] row %d left finite outputs" % (level, what, b, row)
        same[b, row] = True
    for what, (b, kk, col, val) in cols.items():
        assert not finite[b, :, col].any(), "level %d: %s in B[%d] column %d left finite outputs" % (level, what, b, col)
        same[b, :, col] = True
    assert same.all(), "level %d: a non-finite operand changed entries outside its row / column" % level
    if level == 2:      # no subtraction: an Inf stays an Inf where nothing else is non-finite
        b, row, kk, val = rows["inf"]
        assert torch.isinf(out[b, row]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. through the op layer
# ------------------------------------------------------------------------------------------------------------------------------
ATTN = (8, 64, 32, 32)      # N, C, H, W: T = 1024 tokens


def test_attention_shape_opens_both_gates():
    n, c, h, w = ATTN
    t = h * w
    assert G.split_eligible(-1, 0, t, c, t, n) and G.split_tt_eligible(-1, t, t, c, n)          # P V, dS K, P^T dO, dS^T Q; E and dS
    assert G.workspace_bytes(t, t, c, n) == 0 and G.workspace_bytes(t, c, t, n) == 0            # the folded softmax runs
    assert not G.split_tt_eligible(-1, t, t, c, n - 1) and not G.split_tt_eligible(-1, t, t, c // 2, n)


def _attention(qkv, go):
    from odvae_amd import ops
    q = qkv.clone().requires_grad_(True)
    o = ops.attention_qkv(q)
    o.backward(go)
    torch.cuda.synchronize()
    return o.detach(), q.grad


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = nn.Linear(4, 4)
        self.learning_rate = 1e-3

    def configure_optimizers(self):
        return [torch.optim.Adam(self.parameters(), lr=self.learning_rate)], []


def test_attention_follows_the_level(hip_lib):
    import odvae_amd
    from odvae_amd import ops
    from odvae_amd.trainer import Trainer
    n, c, h, w = ATTN
    g = torch.Generator().manual_seed(61)
    qkv = torch.randn(n, 3 * c, h, w, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    go = torch.randn(n, c, h, w, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)

    def same(x, y):
        return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(x, y))

    assert ops.get_float32_matmul_precision() == "highest"
    default = _attention(qkv, go)
    assert all(torch.isfinite(t).all() for t in default)
    try:
        odvae_amd.set_float32_matmul_precision("highest")
        assert same(_attention(qkv, go), default), "the default is not `highest`"
        by_name = {}
        for name in ("high", "medium"):
            odvae_amd.set_float32_matmul_precision(name)
            by_name[name] = _attention(qkv, go)
            odvae_amd.set_float32_matmul_precision("highest")
            with precision(hip_lib, P.NAMES.index(name)):
                through_c = _attention(qkv, go)
            assert same(by_name[name], through_c), "%s: set from Python and set through the C entry point differ" % name
            for what, got, ref in zip(("forward", "d(qkv)"), by_name[name], default):
                assert not torch.equal(got, ref), "%s: %s has the bits of highest" % (name, what)
        assert not same(by_name["high"], by_name["medium"])
        # `torch` mode follows torch's own setting at call time
        before = torch.get_float32_matmul_precision()
        try:
            odvae_amd.set_float32_matmul_precision("torch")
            torch.set_float32_matmul_precision("medium")
            assert same(_attention(qkv, go), by_name["medium"])
            torch.set_float32_matmul_precision("highest")
            assert same(_attention(qkv, go), default)
        finally:
            torch.set_float32_matmul_precision(before)
        # a Trainer sets it for the process and does not take it back
        odvae_amd.set_float32_matmul_precision("highest")
        Trainer(_Tiny(), optimizer_indices=(0,), distributed=False, float32_matmul_precision="high")
        assert ops.get_float32_matmul_precision() == "high"
        assert same(_attention(qkv, go), by_name["high"])
    finally:
        odvae_amd.set_float32_matmul_precision("highest")
    assert same(_attention(qkv, go), default)
