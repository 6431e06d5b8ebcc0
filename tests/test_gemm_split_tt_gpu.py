"""The two T x T attention products on the bf16 matrix pipe (gemm_f32_split.hip, NT form): E = exp(alpha (Q K^T - bound)) behind
odvae_gemm_exp_bound_f32 and dS = alpha E rinv (dO V^T - D) behind odvae_gemm_softmax_bwd[_scaled]_f32.  Everything goes through the C ABI.

Reference: float64 on the CPU.  Yardstick: the f32 MFMA kernel on the same inputs in the same test -- the same entry point under
odvae_gemm_select_staging(1).  With S = A B^T and sbar = sum_k |a_k| |b_k| the cross products the split drops are below 2^-22 sbar
(tests/test_gemm_split_gpu.py derives that), everything kept is accumulated in f32 as the f32 kernel does.  Bounds, derived, not tuned:

  EXPB: E = exp(alpha (S - bound)); to first order the dropped terms move E by at most E alpha 2^-22 sbar, so
        max |E - E64| / E64 (over entries whose E64 is a normal f32 number):  split <= f32 + alpha 2^-22 max sbar.
  SMB:  dS = alpha emul rowmul (S - rowsub) is linear in S, so
        max |dS - dS64| / (alpha |emul| rowmul sbar + tiny):  split <= f32 + 2^-22.

Each test prints the two figures before it asserts; profiles/gemm_split_tt.md records them.

The gate (gemm_tile::split_tt_eligible): staging per shape, ceil(M/128) ceil(N/128) batch >= 512, K at or above its lower bound
(<= 256).  The accuracy cases run at batch 8 (32 x 32 x 8 blocks) so that it opens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-4      # as tests/test_ops_gpu.py
BWD_TOL = 5e-4
BATCH = 8
FULL = (4096, 4096, 256)       # M, N, K of the two products at 64 x 64 tokens, C = 256
RAGGED = (4000, 4040, 252)     # tails on every axis, K % 4 == 0, K % 32 != 0; 32 x 32 x 8 blocks
PAD = 8                        # ldc = N + PAD: the output rows are wider than what is written
TINY = 1e-300


def dev():
    return torch.device("cuda:0")


def make_case(shape, seed, batch=BATCH):
    """A [batch][M][K], B [batch][N][K] (both k-contiguous), rowsub [batch][M], emul [batch][M][N + PAD] (softmax-like, positive),
    rowmul [batch][M] (1 / l-like, positive)."""
    m, n, k = shape
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(batch, m, k, generator=g)
    b = torch.randn(batch, n, k, generator=g)
    rowsub = torch.randn(batch, m, generator=g) * (k ** 0.5) * 0.25
    emul = torch.exp(torch.randn(batch, m, n + PAD, generator=g) * 2.0 - 4.0)
    rowmul = torch.exp(torch.randn(batch, m, generator=g))
    return a, b, rowsub, emul, rowmul


def row_bound(a, b):
    """An upper bound of every row's scores, as f32: the float64 row maximum, rounded up a little."""
    out = torch.empty(a.shape[0], a.shape[1])
    for i in range(a.shape[0]):
        out[i] = (a[i].double() @ b[i].double().t()).max(dim=1).values.float() + 0.125
    return out


def run_expb(hip_lib, shape, alpha, a_d, b_d, bound_d, staging=-1, batch=BATCH):
    """E lands in the first N columns of (N + PAD)-wide rows of NaNs; returns [batch][M][N + PAD]."""
    from odvae_amd import lib as _lib
    m, n, k = shape
    ldc = n + PAD
    out = torch.full((batch, m, ldc), float("nan"), device=dev())
    prev = hip_lib.odvae_gemm_select_staging(staging)
    try:
        _lib.check(hip_lib.odvae_gemm_exp_bound_f32(m, n, k, alpha, a_d.data_ptr(), k, m * k, b_d.data_ptr(), k, n * k, bound_d.data_ptr(), m,
                                                    out.data_ptr(), ldc, m * ldc, batch, _lib.stream_ptr()), "gemm_exp_bound")
    finally:
        hip_lib.odvae_gemm_select_staging(prev)
    torch.cuda.synchronize()
    return out


def run_smb(hip_lib, shape, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d, staging=-1, batch=BATCH, alias=False):
    """dS in (N + PAD)-wide rows of NaNs (alias: written over a copy of emul, as the attention backward may do)."""
    from odvae_amd import lib as _lib
    m, n, k = shape
    ldc = n + PAD
    if alias:
        out = emul_d.clone()
        e_ptr = out.data_ptr()
    else:
        out = torch.full((batch, m, ldc), float("nan"), device=dev())
        e_ptr = emul_d.data_ptr()
    prev = hip_lib.odvae_gemm_select_staging(staging)
    try:
        if rowmul_d is None:
            _lib.check(hip_lib.odvae_gemm_softmax_bwd_f32(m, n, k, alpha, a_d.data_ptr(), k, m * k, b_d.data_ptr(), k, n * k, e_ptr,
                                                          rowsub_d.data_ptr(), m, out.data_ptr(), ldc, m * ldc, batch, _lib.stream_ptr()),
                       "gemm_softmax_bwd")
        else:
            _lib.check(hip_lib.odvae_gemm_softmax_bwd_scaled_f32(m, n, k, alpha, a_d.data_ptr(), k, m * k, b_d.data_ptr(), k, n * k, e_ptr,
                                                                 rowsub_d.data_ptr(), rowmul_d.data_ptr(), m, out.data_ptr(), ldc, m * ldc,
                                                                 batch, _lib.stream_ptr()), "gemm_softmax_bwd_scaled")
    finally:
        hip_lib.odvae_gemm_select_staging(prev)
    torch.cuda.synchronize()
    return out


def expb_errors(outs, alpha, a, b, bound, n):
    """(max relative error of E against float64 for every output in `outs`, max sbar), one image at a time."""
    errs, sbar_max = [0.0] * len(outs), 0.0
    for i in range(a.shape[0]):
        a64, b64 = a[i].double(), b[i].double()
        e64 = torch.exp(alpha * (a64 @ b64.t() - bound[i].double()[:, None]))
        sbar_max = max(sbar_max, (a64.abs() @ b64.abs().t()).max().item())
        normal = e64 >= 2.0 ** -126
        for j, o in enumerate(outs):
            rel = (o[i, :, :n].cpu().double() - e64).abs() / e64
            errs[j] = max(errs[j], rel[normal].max().item())
    return errs, sbar_max


def smb_errors(outs, alpha, a, b, rowsub, emul, rowmul, n):
    errs = [0.0] * len(outs)
    for i in range(a.shape[0]):
        a64, b64 = a[i].double(), b[i].double()
        f64 = alpha * emul[i, :, :n].double() * (rowmul[i].double()[:, None] if rowmul is not None else 1.0)
        ds64 = f64 * (a64 @ b64.t() - rowsub[i].double()[:, None])
        scale = f64.abs() * (a64.abs() @ b64.abs().t()) + TINY
        for j, o in enumerate(outs):
            errs[j] = max(errs[j], ((o[i, :, :n].cpu().double() - ds64).abs() / scale).max().item())
    return errs


@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["full", "ragged"])
def test_exp_bound_is_as_accurate_as_the_f32_kernel(hip_lib, shape):
    m, n, k = shape
    alpha = float(k) ** -0.5
    a, b, _, _, _ = make_case(shape, seed=m + 3 * k)
    bound = row_bound(a, b)
    a_d, b_d, bound_d = a.to(dev()), b.to(dev()), bound.to(dev())
    out = run_expb(hip_lib, shape, alpha, a_d, b_d, bound_d)
    out_f32 = run_expb(hip_lib, shape, alpha, a_d, b_d, bound_d, staging=1)
    out_again = run_expb(hip_lib, shape, alpha, a_d, b_d, bound_d)
    (e_split, e_f32), sbar_max = expb_errors([out, out_f32], alpha, a, b, bound, n)
    allowed = e_f32 + alpha * 2.0 ** -22 * sbar_max
    print("\ngemm_split_tt EXPB M=%d N=%d K=%d batch=%d: rel(E) split %.3e  f32 %.3e  bound %.3e  (alpha 2^-22 max sbar %.3e)"
          % (m, n, k, BATCH, e_split, e_f32, allowed, alpha * 2.0 ** -22 * sbar_max))
    assert torch.isnan(out[:, :, n:]).all(), "wrote outside its columns"
    assert torch.isfinite(out[:, :, :n]).all()
    assert not torch.equal(out[:, :, :n], out_f32[:, :, :n]), "the gate did not open: the f32 MFMA kernel ran"
    assert torch.equal(out[:, :, :n], out_again[:, :, :n]), "two launches differ"
    assert e_split <= allowed


@pytest.mark.parametrize("with_rowmul", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["full", "ragged"])
def test_softmax_bwd_is_as_accurate_as_the_f32_kernel(hip_lib, shape, with_rowmul):
    m, n, k = shape
    alpha = float(k) ** -0.5
    a, b, rowsub, emul, rowmul = make_case(shape, seed=m + 5 * k + with_rowmul)
    if not with_rowmul:
        rowmul = None
    a_d, b_d, rowsub_d, emul_d = a.to(dev()), b.to(dev()), rowsub.to(dev()), emul.to(dev())
    rowmul_d = rowmul.to(dev()) if with_rowmul else None
    out = run_smb(hip_lib, shape, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d)
    out_f32 = run_smb(hip_lib, shape, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d, staging=1)
    out_again = run_smb(hip_lib, shape, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d)
    out_alias = run_smb(hip_lib, shape, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d, alias=True)
    e_split, e_f32 = smb_errors([out, out_f32], alpha, a, b, rowsub, emul, rowmul, n)
    print("\ngemm_split_tt SMB %s M=%d N=%d K=%d batch=%d: e_split %.3e  e_f32 %.3e  bound %.3e"
          % ("scaled" if with_rowmul else "plain", m, n, k, BATCH, e_split, e_f32, e_f32 + 2.0 ** -22))
    assert torch.isnan(out[:, :, n:]).all(), "wrote outside its columns"
    assert torch.isfinite(out[:, :, :n]).all()
    assert not torch.equal(out[:, :, :n], out_f32[:, :, :n]), "the gate did not open: the f32 MFMA kernel ran"
    assert torch.equal(out[:, :, :n], out_again[:, :, :n]), "two launches differ"
    assert torch.equal(out_alias[:, :, :n], out[:, :, :n]), "dS written over P differs from the separate output"
    assert torch.equal(out_alias[:, :, n:], emul_d[:, :, n:]), "the aliased call wrote outside its columns"
    assert e_split <= e_f32 + 2.0 ** -22


def test_gate_keeps_small_launches_and_forced_staging_on_the_f32_kernel(hip_lib):
    """Below the block threshold (batch 1 at T = 1024: 64 blocks) the same calls are the f32 MFMA kernel, bit for bit; a forced staging
    mode means the f32 kernel at every shape."""
    small = (1024, 1024, 256)
    m, n, k = small
    alpha = float(k) ** -0.5
    a, b, rowsub, emul, rowmul = make_case(small, seed=41, batch=1)
    bound = row_bound(a, b)
    a_d, b_d, rowsub_d, emul_d, rowmul_d, bound_d = (x.to(dev()) for x in (a, b, rowsub, emul, rowmul, bound))
    for staging in (0, 1):
        assert torch.equal(run_expb(hip_lib, small, alpha, a_d, b_d, bound_d, batch=1)[:, :, :n],
                           run_expb(hip_lib, small, alpha, a_d, b_d, bound_d, staging=staging, batch=1)[:, :, :n])
        for rm in (None, rowmul_d):
            assert torch.equal(run_smb(hip_lib, small, alpha, a_d, b_d, rowsub_d, emul_d, rm, batch=1)[:, :, :n],
                               run_smb(hip_lib, small, alpha, a_d, b_d, rowsub_d, emul_d, rm, staging=staging, batch=1)[:, :, :n])
    m, n, k = FULL
    a, b, rowsub, emul, rowmul = make_case(FULL, seed=42)
    bound = row_bound(a, b)
    a_d, b_d, rowsub_d, emul_d, rowmul_d, bound_d = (x.to(dev()) for x in (a, b, rowsub, emul, rowmul, bound))
    forced = [run_expb(hip_lib, FULL, alpha, a_d, b_d, bound_d, staging=s)[:, :, :n] for s in (0, 1, 2)]
    assert torch.equal(forced[0], forced[1]) and torch.equal(forced[1], forced[2])
    assert not torch.equal(run_expb(hip_lib, FULL, alpha, a_d, b_d, bound_d)[:, :, :n], forced[1])
    forced = [run_smb(hip_lib, FULL, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d, staging=s)[:, :, :n] for s in (0, 1, 2)]
    assert torch.equal(forced[0], forced[1]) and torch.equal(forced[1], forced[2])
    assert not torch.equal(run_smb(hip_lib, FULL, alpha, a_d, b_d, rowsub_d, emul_d, rowmul_d)[:, :, :n], forced[1])


@pytest.mark.parametrize("epi", ["expb", "smb", "smb_scaled"])
def test_nan_and_inf_operands_stay_visible(hip_lib, epi):
    """x = +-Inf splits into hi = Inf, x - hi = NaN: an Inf in q / dO gives NaN where the f32 kernel gives Inf, 0 or NaN.  Never a finite
    number, and never outside the operand's own output row."""
    m, n, k = FULL
    alpha = float(k) ** -0.5
    a, b, rowsub, emul, rowmul = make_case(FULL, seed=43)
    bound = row_bound(a, b)
    spots = {"nan": (0, 77, 123, float("nan")), "inf": (3, 4001, 31, float("inf")), "-inf": (7, 130, 255, float("-inf"))}
    for bi, row, kk, val in spots.values():
        a[bi, row, kk] = val
    a_d, b_d = a.to(dev()), b.to(dev())
    if epi == "expb":
        out = run_expb(hip_lib, FULL, alpha, a_d, b_d, bound.to(dev()))[:, :, :n]
    else:
        out = run_smb(hip_lib, FULL, alpha, a_d, b_d, rowsub.to(dev()), emul.to(dev()), rowmul.to(dev()) if epi == "smb_scaled" else None)[:, :, :n]
    finite = torch.isfinite(out)
    for what, (bi, row, kk, val) in spots.items():
        assert not finite[bi, row].any(), "%s in A[%d] row %d left finite outputs" % (what, bi, row)
        finite[bi, row] = True
    assert finite.all(), "a non-finite operand spread beyond its row"


def test_attention_at_full_token_count_matches_float64(hip_lib):
    """attention_qkv at n = 8, C = 256, 64 x 64 tokens -- all six products above their gates -- against float64 attention on the CPU,
    forward and d(qkv), at the tolerances of test_ops_gpu.py's test_attention; the folded softmax must not have fallen back."""
    from odvae_amd import ops
    n, c, h, w = 8, 256, 64, 64
    t = h * w
    g = torch.Generator().manual_seed(31)
    qkv = torch.randn(n, 3 * c, h, w, generator=g)
    go = torch.randn(n, c, h, w, generator=g)
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr[:, :c], qr[:, c:2 * c], qr[:, 2 * c:]
    p = torch.softmax(torch.bmm(q.reshape(n, c, t).permute(0, 2, 1), k.reshape(n, c, t)) * (c ** -0.5), dim=2)
    o_ref = torch.bmm(v.reshape(n, c, t), p.permute(0, 2, 1)).reshape(n, c, h, w)
    o_ref.backward(go.double())
    qd = qkv.to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    o = ops.attention_qkv(qd)
    o.backward(go.to(dev()))
    torch.cuda.synchronize()
    assert ops._ATTN_LAST_FLAG is not None and int(ops._ATTN_LAST_FLAG.item()) == 0, "the folded softmax fell back"

    def check(a, b, tol, what):
        a, b = a.detach().cpu().double(), b.detach()
        err, ref = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
        print("\ngemm_split_tt attention %s: max err %.3e, allowed %.1e * %.3e" % (what, err, tol, ref))
        assert err <= tol * ref, what

    check(o, o_ref, FWD_TOL, "forward")
    check(qd.grad, qr.grad, BWD_TOL, "d(qkv)")
