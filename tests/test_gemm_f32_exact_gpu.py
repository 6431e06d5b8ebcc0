"""The f32 GEMM family (gemm_f32.hip, gemm_f32_split.hip, gemm_f32_tile.h), bit for bit, on exactly summable inputs
(tests/gemm_exact_inputs.py).  On such operands no f32 addition rounds in any order, so every output must EQUAL the float64 reference:
every comparison here is on raw bits (`assert_bits_equal`, `torch.equal` on int32 views).  Every test first asserts the precondition on
the tensors it uses.  Operands live in NaN-filled allocations (leading dimensions, batch strides and the rows behind an operand are
NaN), outputs in NaN-filled rows wider than N with canaries behind them; after a call every element outside the logical output must
still hold the bits it had.  tests/test_gemm_exact_inputs.py asserts on the host that the case lists reach every instantiation.

case (list in gemm_exact_inputs)          kernel form                                   layout        epilogue                  splits
UNSPLIT_CASES x staging -1, 0, 1, 2       reg / dma32 / dma16 (-1: dma32 if TN, TT)      NN NT TN TT   plain, alpha+bias, b+res  1
  (132, 132, 36, 3) TN, staging 0         reg_batched <false,false,false,true>          TN            "                         1
  K = 4, 8, 12 / 1, 33, 37 (TN)           all of the above: K below one step, odd K
SPLITK_CASES x staging -1, 0, 1, 2        the same kernels + gemm_splitk_reduce_kernel   NN NT TN TT   "  (in the reduce)        2, 5, 18
  K = 1028 / 1027                         partial last step of the last split                                                   2
  K = 3000 (batch 1 and 2)                one unrolled pass of the reduce + remainder; slabs [split][batch]                     5
  K = 9220                                four passes + remainder 2; the last split's k range is empty                          18
PRED_CASES                                gemm_f32_pred_kernel                          NN NT TN TT   plain; pred 0 / 1         1
  batch 260                               1040 (tile, batch) pairs on 1024 blocks: 16 blocks walk two pairs
SPLIT_CASES x recipes A S1 S2 S3 S3T      gemm_f32_split_kernel (K = 1024; batch 128)   NN TN         plain                     1
  K = 1028 / 1051 at batch 2              choose_splits says 2: the f32 kernels + reduce                                        2
TT_SHAPES, softmax backward               reg / dma32 / dma16; split at batch 128       NT            EPI_SMB (+ rowmul, alias) 1
TT_SHAPES, exp_bound                      reg; split at batch 128                       NT            EPI_EXPB                  1
ROWNORM_CASES                             reg (K = 100; 1028 at batch 2); split         NN            EPI_ROWNORM               1
CONV1X1_CASES through ops.conv1x1         forward NT reg, dx NN reg, dw TN dma32 (+ reduce at 1152 pixels; split at 1024 pixels)
"""
import pytest
import torch

import canary_buffers as CB
import gemm_exact_inputs as G

pytestmark = pytest.mark.gpu
DEV = CB.DEV


# ------------------------------------------------------------------------------------------------------------------------------
# device side of the poisoned layout
# ------------------------------------------------------------------------------------------------------------------------------
def ptr(buf):
    """the address of logical element (0, 0, 0) of an embedded buffer"""
    return buf.data_ptr() + 4 * G.LEAD


def operand(buf):
    return buf.to(DEV)


def output(e, values=None):
    """(device buffer with canaries behind it, its bits before the call): an Embedded layout, NaN (or `values`) inside"""
    buf, view = CB.out_buf(e.numel)
    view.copy_(e.buffer(values).to(DEV))
    return buf, buf.clone()


def logical(e, buf):
    return buf[e.index.to(DEV)]


def assert_untouched_outside(e, buf, before, what):
    """every element of the allocation outside the logical output -- NaN padding, batch gaps, canaries -- holds its original bits"""
    CB.assert_canary(buf)
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    outside[e.index.reshape(-1).to(DEV)] = False
    assert torch.equal(buf.view(torch.int32)[outside], before.view(torch.int32)[outside]), what + ": wrote outside its logical output"


def assert_unchanged(buf, before, what):
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), what + ": an input was written"


class staging(object):
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.odvae_gemm_select_staging(self.mode)

    def __exit__(self, *exc):
        self.lib.odvae_gemm_select_staging(self.prev)


class Launch(object):
    """One product's device operands, uploaded once and launched under several staging modes."""

    def __init__(self, hip_lib, layout, c, ldc_pad=8):
        self.lib, self.layout, self.c = hip_lib, layout, c
        self.ta, self.tb = G.LAYOUTS[layout]
        self.batch, self.m, self.k = c["a"].shape
        self.n = c["b"].shape[2]
        self.ea, ba, self.eb, bb = G.embed_operands(layout, c)
        self.a, self.b = operand(ba), operand(bb)
        self.ec = G.Embedded(self.batch, self.m, self.n, ld_pad=ldc_pad)
        self.bias = self.res = None
        if c.get("bias") is not None:
            self.ebias = G.Embedded(1, 1, self.n)
            self.bias = operand(self.ebias.buffer(c["bias"].reshape(1, 1, -1)))
        if c.get("res") is not None:
            self.res = operand(self.ec.buffer(c["res"]))
        self.inputs = [(t, t.clone()) for t in (self.a, self.b, self.bias, self.res) if t is not None]

    def gemm(self, mode, expect_splits=None):
        from odvae_amd import lib as _lib
        L = self.lib
        out, before = output(self.ec)
        need = L.odvae_gemm_f32_workspace_bytes(self.m, self.n, self.k, self.batch)
        assert need == G.workspace_bytes(self.m, self.n, self.k, self.batch), "the mirror of choose_splits disagrees with the library"
        if expect_splits is not None:
            assert need == expect_splits * self.batch * self.m * self.n * 4
        ws = CB.workspace(need) if need else None
        with staging(L, mode):
            _lib.check(L.odvae_gemm_f32(self.ta, self.tb, self.m, self.n, self.k, float(self.c["alpha"]), ptr(self.a), self.ea.ld, self.ea.stride,
                                        ptr(self.b), self.eb.ld, self.eb.stride, ptr(out), self.ec.ld, self.ec.stride,
                                        ptr(self.bias) if self.bias is not None else None, ptr(self.res) if self.res is not None else None,
                                        self.batch, ws.data_ptr() if need else None, need, _lib.stream_ptr()), "gemm_f32")
        torch.cuda.synchronize()
        if need:
            CB.assert_workspace_canary(ws)
        return out, before

    def pred(self, flag):
        from odvae_amd import lib as _lib
        L = self.lib
        out, before = output(self.ec)
        p = torch.tensor([flag], dtype=torch.int32, device=DEV)
        _lib.check(L.odvae_gemm_pred_f32(self.ta, self.tb, self.m, self.n, self.k, 1.0, ptr(self.a), self.ea.ld, self.ea.stride,
                                         ptr(self.b), self.eb.ld, self.eb.stride, ptr(out), self.ec.ld, self.ec.stride, self.batch,
                                         p.data_ptr(), _lib.stream_ptr()), "gemm_pred")
        torch.cuda.synchronize()
        assert int(p.item()) == flag
        return out, before

    def check(self, out, before, want64, what):
        G.assert_bits_equal(logical(self.ec, out), want64.float(), what)
        assert_untouched_outside(self.ec, out, before, what)
        for t, t0 in self.inputs:
            assert_unchanged(t, t0, what)


def _id(case):
    return "-".join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. odvae_gemm_f32, unsplit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.UNSPLIT_CASES, ids=_id)
def test_unsplit_product_equals_float64(hip_lib, case):
    layout, recipe, epi, m, n, k, batch = case
    c = G.make_case(recipe, m, n, k, batch, epi)
    G.assert_exactly_summable(c)
    want = G.reference(c)
    run = Launch(hip_lib, layout, c)
    for mode in G.STAGINGS:      # each equals float64, so they equal each other
        out, before = run.gemm(mode, expect_splits=0)
        run.check(out, before, want, "%s staging %d %s" % (_id(case), mode, sorted(G.gemm_forms(layout, m, n, k, batch, mode))))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. split-K
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", G.EPILOGUES)
@pytest.mark.parametrize("case", G.SPLITK_CASES, ids=_id)
def test_split_k_product_equals_float64(hip_lib, case, epi):
    layout, m, n, k, batch, splits = case
    c = G.make_case("A", m, n, k, batch, epi)
    G.assert_exactly_summable(c)
    want = G.reference(c)
    run = Launch(hip_lib, layout, c)
    for mode in G.STAGINGS:
        out, before = run.gemm(mode, expect_splits=splits)
        run.check(out, before, want, "%s %s staging %d" % (_id(case), epi, mode))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. odvae_gemm_pred_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.PRED_CASES, ids=_id)
def test_predicated_product(hip_lib, case):
    layout, m, n, k, batch = case
    c = G.make_case("A", m, n, k, batch)
    G.assert_exactly_summable(c)
    run = Launch(hip_lib, layout, c)
    out, before = run.pred(0)
    assert_unchanged(out, before, _id(case) + " with *pred == 0")
    out, before = run.pred(1)
    run.check(out, before, G.reference(c), _id(case) + " with *pred == 1")


# ------------------------------------------------------------------------------------------------------------------------------
# 9. one NaN inside A: its row of its batch, nothing else
# ------------------------------------------------------------------------------------------------------------------------------
NAN_CASES = [("gemm", "NT", 132, 260, 100, 3, -1), ("gemm", "TN", 132, 260, 100, 3, -1), ("gemm", "NN", 132, 260, 100, 3, 2),
             ("gemm", "NN", 128, 128, 3000, 2, -1), ("gemm", "TN", 128, 128, 9220, 1, -1), ("pred", "NT", 132, 132, 36, 260, -1)]


@pytest.mark.parametrize("case", NAN_CASES, ids=_id)
def test_one_nan_in_a_poisons_exactly_its_row(hip_lib, case):
    kind, layout, m, n, k, batch, mode = case
    c = G.make_case("A", m, n, k, batch)
    G.assert_exactly_summable(c)
    want = G.reference(c).float()
    b_, row, kk = batch - 1, m - 3, k - 2
    c["a"][b_, row, kk] = G.NAN
    run = Launch(hip_lib, layout, c)
    out, before = run.pred(1) if kind == "pred" else run.gemm(mode)
    got = logical(run.ec, out).clone()
    assert torch.isnan(got[b_, row]).all(), "the NaN did not reach every column of its row"
    got[b_, row] = 0.0
    want[b_, row] = 0.0
    G.assert_bits_equal(got, want, _id(case))
    assert_untouched_outside(run.ec, out, before, _id(case))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the bf16-split form
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", G.SPLIT_RECIPES)
@pytest.mark.parametrize("case", G.SPLIT_CASES, ids=_id)
def test_deep_product_planes_equal_float64(hip_lib, case, recipe):
    layout, m, n, k, batch, shared = case
    c = G.make_case(recipe, m, n, k, batch, shared_b=shared)
    G.assert_exactly_summable(c)
    if recipe != "A":
        G.assert_planes(c)
    want = G.reference(c)
    run = Launch(hip_lib, layout, c)
    for mode in (-1, 1):       # the form the gate chooses, and the f32 kernel on the same operands
        out, before = run.gemm(mode)
        run.check(out, before, want, "%s %s staging %d %s" % (_id(case), recipe, mode, sorted(G.gemm_forms(layout, m, n, k, batch, mode))))


@pytest.mark.parametrize("case", G.SPLIT_CASES, ids=_id)
def test_split_gate_opens_where_the_mirror_says(hip_lib, case):
    """Exact inputs cannot show which kernel ran.  Random-normal operands can: the bf16-split kernel rounds differently from the f32
    kernels, which agree with each other to the bit."""
    layout, m, n, k, batch, shared = case
    g = torch.Generator().manual_seed(k + batch)
    c = {"a": torch.randn(batch, m, k, generator=g).double(), "b": torch.randn(1 if shared else batch, k, n, generator=g).double(), "alpha": 1.0}
    run = Launch(hip_lib, layout, c)
    default, forced = (logical(run.ec, run.gemm(mode)[0]) for mode in (-1, 1))
    split = ("split", layout, "none") in G.gemm_forms(layout, m, n, k, batch, -1)
    assert torch.isfinite(default).all() and torch.isfinite(forced).all()
    assert torch.equal(default.view(torch.int32), forced.view(torch.int32)) == (not split), "the gate and its mirror disagree"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. softmax backward in the epilogue
# ------------------------------------------------------------------------------------------------------------------------------
def row_vector(e, values):
    return operand(e.buffer(values[:, None, :]))


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "alias"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("shape", G.TT_SHAPES, ids=_id)
def test_softmax_backward_tail_equals_float64(hip_lib, shape, scaled, alias):
    from odvae_amd import lib as _lib
    m, n, k, batch = shape
    c = G.make_smb_case(m, n, k, batch, scaled)
    G.assert_smb_exact(c)
    want = G.smb_reference(c)
    run = Launch(hip_lib, "NT", c)
    erow = G.Embedded(batch, 1, m)
    rowdot = row_vector(erow, c["rowdot"])
    rowmul = row_vector(erow, c["rowmul"]) if scaled else None
    for mode in G.SMB_STAGINGS[shape]:
        p, p0 = output(run.ec, c["p"])
        out, before = (p, p0) if alias else output(run.ec)
        with staging(hip_lib, mode):
            if scaled:
                rc = hip_lib.odvae_gemm_softmax_bwd_scaled_f32(m, n, k, c["alpha"], ptr(run.a), run.ea.ld, run.ea.stride, ptr(run.b), run.eb.ld, run.eb.stride,
                                                               ptr(p), ptr(rowdot), ptr(rowmul), erow.stride, ptr(out), run.ec.ld, run.ec.stride, batch,
                                                               _lib.stream_ptr())
            else:
                rc = hip_lib.odvae_gemm_softmax_bwd_f32(m, n, k, c["alpha"], ptr(run.a), run.ea.ld, run.ea.stride, ptr(run.b), run.eb.ld, run.eb.stride,
                                                        ptr(p), ptr(rowdot), erow.stride, ptr(out), run.ec.ld, run.ec.stride, batch, _lib.stream_ptr())
        _lib.check(rc, "gemm_softmax_bwd")
        torch.cuda.synchronize()
        what = "%s staging %d %s" % (_id(shape), mode, sorted(G.smb_forms(m, n, k, batch, mode)))
        run.check(out, before, want, what)
        if not alias:
            assert_unchanged(p, p0, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. exponentials against a row bound
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.TT_SHAPES, ids=_id)
def test_exp_bound_tail(hip_lib, shape):
    from odvae_amd import lib as _lib
    m, n, k, batch = shape
    c = G.make_expb_case(m, n, k, batch)
    G.assert_expb_exact(c)
    run = Launch(hip_lib, "NT", c)
    erow = G.Embedded(batch, 1, m)
    bound = row_vector(erow, c["bound"])
    cls = c["cls"].to(DEV)
    near = []
    for mode in G.EXPB_STAGINGS[shape]:
        out, before = output(run.ec)
        with staging(hip_lib, mode):
            _lib.check(hip_lib.odvae_gemm_exp_bound_f32(m, n, k, c["alpha"], ptr(run.a), run.ea.ld, run.ea.stride, ptr(run.b), run.eb.ld, run.eb.stride,
                                                        ptr(bound), erow.stride, ptr(out), run.ec.ld, run.ec.stride, batch, _lib.stream_ptr()),
                       "gemm_exp_bound")
        torch.cuda.synchronize()
        what = "%s staging %d %s" % (_id(shape), mode, sorted(G.expb_forms(m, n, k, batch, mode)))
        got = logical(run.ec, out)
        one, far = got[:, :, cls == 0], got[:, :, cls == 1]
        G.assert_bits_equal(one, torch.ones_like(one), what + ": score == bound", summed=False)
        G.assert_bits_equal(far, torch.zeros_like(far), what + ": score far below the bound", summed=False)
        near.append(got[:, :, cls == 2])
        assert torch.isfinite(near[-1]).all() and (near[-1] > 0).all()
        assert_untouched_outside(run.ec, out, before, what)
    for other in near[1:]:      # the same exp2 of the same exact argument in every form
        G.assert_bits_equal(other, near[0], _id(shape) + ": the forms disagree on exp of a small difference", summed=False)
    if shape[3] >= 128:
        assert G.expb_forms(m, n, k, batch, -1) != G.expb_forms(m, n, k, batch, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. row-normalised product
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.ROWNORM_CASES, ids=_id)
def test_rownorm_equals_float64(hip_lib, case):
    from odvae_amd import lib as _lib
    m, n, k, batch, shared = case
    c = G.make_rownorm_case(m, n, k, batch, shared_b=shared)
    l = G.assert_rownorm_exact(c)
    want = torch.matmul(c["a"], c["b"]) / l[:, :, None]
    run = Launch(hip_lib, "NN", c)
    erow = G.Embedded(batch, 1, m)
    for mode in (-1, 1):
        out, before = output(run.ec)
        rinv, rinv0 = output(erow)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        with staging(hip_lib, mode):
            _lib.check(hip_lib.odvae_gemm_rownorm_f32(m, n, k, ptr(run.a), run.ea.ld, run.ea.stride, ptr(run.b), run.eb.ld, run.eb.stride,
                                                      ptr(out), run.ec.ld, run.ec.stride, ptr(rinv), erow.stride, flag.data_ptr(), batch,
                                                      _lib.stream_ptr()), "gemm_rownorm")
        torch.cuda.synchronize()
        what = "%s staging %d %s" % (_id(case), mode, sorted(G.rownorm_forms(m, n, k, batch, mode)))
        assert int(flag.item()) == 0, what
        run.check(out, before, want, what)
        G.assert_bits_equal(logical(erow, rinv), (1.0 / l).float()[:, None, :], what + ": 1 / l", summed=False)
        assert_untouched_outside(erow, rinv, rinv0, what + ": 1 / l")


# ------------------------------------------------------------------------------------------------------------------------------
# 8. through the op layer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CONV1X1_CASES, ids=_id)
def test_conv1x1_equals_float64(hip_lib, case):
    from odvae_amd import ops
    n, cin, cout, h, w = case
    c = G.make_conv1x1_case(*case)
    G.assert_conv1x1_exactly_summable(c)
    want = G.conv1x1_references(c)
    px = n * h * w
    for (m_, n_, k_) in ((px, cout, cin), (px, cin, cout), (cout, cin, px)):      # the library's split decision against the mirror's
        assert hip_lib.odvae_gemm_f32_workspace_bytes(m_, n_, k_, 1) == G.workspace_bytes(m_, n_, k_, 1)
    forms = G.conv1x1_forms(*case)
    cl = torch.channels_last
    x = c["x"].float().to(DEV).contiguous(memory_format=cl).requires_grad_(True)
    wt = c["w"].float().to(DEV).requires_grad_(True)
    b = c["b"].float().to(DEV).requires_grad_(True)
    res = c["res"].float().to(DEV).contiguous(memory_format=cl)
    y = ops.conv1x1(x, wt, b, res)
    y.backward(c["dy"].float().to(DEV).contiguous(memory_format=cl))
    torch.cuda.synchronize()
    G.assert_bits_equal(y.detach(), want["y"].float(), "%s forward %s" % (_id(case), sorted(forms["forward"])))
    G.assert_bits_equal(x.grad, want["dx"].float(), "%s dx %s" % (_id(case), sorted(forms["dx"])))
    G.assert_bits_equal(wt.grad, want["dw"].float(), "%s dw %s" % (_id(case), sorted(forms["dw"])))
    G.assert_bits_equal(b.grad, want["db"].float(), "%s db" % _id(case))
