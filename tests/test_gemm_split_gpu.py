"""The T-deep attention products on the bf16 matrix pipe (gemm_f32_split.hip): an f32 operand is split exactly into three bf16
numbers and six of the nine cross products are summed in f32.  Everything goes through the C ABI.

Reference: the float64 product on the CPU.  Error measure: e = max over the output of |C - C64| / sum_k |a_k| |b_k|.
Bound (derived, not tuned): with round-to-nearest splits |mid| <= 2^-8 |x| and |lo| <= 2^-16 |x|, so the three dropped products
(mid lo, lo mid, lo lo) are below 2 * 2^-24 + 2^-32 < 2^-22 of sum |a| |b|; everything kept is accumulated in f32 like the f32
MFMA kernel does.  So e_split <= e_f32 + 2^-22, e_f32 being the error of the f32 MFMA kernel (odvae_gemm_select_staging(1)) on the
same inputs in the same test.  Each test prints the two figures before it asserts; profiles/gemm_split.md records them.

The gate (gemm_tile::split_eligible): staging per shape, no split-K (tiles x batch >= 512), B row-contiguous, K >= 1024, no bias, no
residual.  All cases run at batch 8 so that it opens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-4      # as tests/test_ops_gpu.py
BWD_TOL = 5e-4
BATCH = 8
FULL = (4096, 256, 4096)       # M, N, K of the attention products at 64 x 64 tokens, C = 256
RAGGED = (4000, 200, 4072)     # tails on every axis, K % 32 != 0; 32 x 2 tiles x 8 = 512


def dev():
    return torch.device("cuda:0")


def make_a(kind, rows, cols, g):
    """The stored A matrix [BATCH][rows][cols] (contiguous axis = the softmax axis of P / dS in both forms)."""
    if kind == "normal":
        return torch.randn(BATCH, rows, cols, generator=g)
    s = torch.randn(BATCH, rows, cols, generator=g) * 3.0      # softmax-like: exponentials relative to the row maximum ...
    a = torch.exp(s - s.max(dim=2, keepdim=True).values)
    a[:, 5::97] *= 1e-30                                        # ... some rows scaled down to 1e-30
    return a


def make_case(form, shape, kind, seed):
    """Operands laid out as the attention has them: A with lda = its contiguous extent, B inside a three times wider row (q | k | v)."""
    m, n, k = shape
    g = torch.Generator().manual_seed(seed)
    a = make_a(kind, *((k, m) if form == "TN" else (m, k)), g)
    packed = torch.randn(BATCH, k, 3 * n, generator=g)
    return a, packed


def run_gemm(hip_lib, form, shape, a_d, packed_d, staging=-1):
    """C lands in the middle third of a 3N-wide row of NaNs, as dK does; returns [BATCH][M][3N]."""
    from odvae_amd import ops
    m, n, k = shape
    ta = 1 if form == "TN" else 0
    out = torch.full((BATCH, m, 3 * n), float("nan"), device=dev())
    b_view = packed_d.as_strided((1,), (1,), packed_d.storage_offset() + 2 * n)
    c_view = out.as_strided((1,), (1,), n)
    prev = hip_lib.odvae_gemm_select_staging(staging)
    try:
        ops.gemm(ta, 0, m, n, k, 1.0, a_d, a_d.shape[2], a_d.shape[1] * a_d.shape[2], b_view, 3 * n, k * 3 * n, c_view, 3 * n, m * 3 * n,
                 None, None, BATCH)
    finally:
        hip_lib.odvae_gemm_select_staging(prev)
    torch.cuda.synchronize()
    return out


def reference(form, shape, a, packed):
    m, n, k = shape
    a64 = (a.transpose(1, 2) if form == "TN" else a).double()
    b64 = packed[:, :, 2 * n:].double()
    return torch.bmm(a64, b64), torch.bmm(a64.abs(), b64.abs())


def rel_err(c, c64, scale):
    return ((c.cpu().double() - c64).abs() / scale).max().item()


@pytest.mark.parametrize("kind", ["normal", "softmax"])
@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["full", "ragged"])
@pytest.mark.parametrize("form", ["NN", "TN"])
def test_split_product_is_as_accurate_as_the_f32_kernel(hip_lib, form, shape, kind):
    m, n, k = shape
    a, packed = make_case(form, shape, kind, seed=m + 3 * k + (form == "TN") + 7 * (kind == "softmax"))
    a_d, packed_d = a.to(dev()), packed.to(dev())
    out = run_gemm(hip_lib, form, shape, a_d, packed_d)
    out_f32 = run_gemm(hip_lib, form, shape, a_d, packed_d, staging=1)
    out_again = run_gemm(hip_lib, form, shape, a_d, packed_d)
    c64, scale = reference(form, shape, a, packed)
    e_split = rel_err(out[:, :, n:2 * n], c64, scale)
    e_f32 = rel_err(out_f32[:, :, n:2 * n], c64, scale)
    print("\ngemm_split accuracy %s %s M=%d N=%d K=%d batch=%d: e_split %.3e  e_f32 %.3e  bound %.3e"
          % (form, kind, m, n, k, BATCH, e_split, e_f32, e_f32 + 2.0 ** -22))
    assert torch.isnan(out[:, :, :n]).all() and torch.isnan(out[:, :, 2 * n:]).all(), "wrote outside its columns"
    assert torch.isfinite(out[:, :, n:2 * n]).all()
    assert not torch.equal(out[:, :, n:2 * n], out_f32[:, :, n:2 * n]), "the gate did not open: the f32 MFMA kernel ran"
    assert torch.equal(out[:, :, n:2 * n], out_again[:, :, n:2 * n]), "two launches differ"
    assert e_split <= e_f32 + 2.0 ** -22


@pytest.mark.parametrize("form", ["NN", "TN"])
def test_gate_keeps_shallow_products_on_the_f32_kernel(hip_lib, form):
    """K = 512 < 1024: the same call is the f32 MFMA kernel, bit for bit; forcing a staging mode means the f32 kernel at any depth."""
    shape = (4096, 256, 512)
    a, packed = make_case(form, shape, "normal", seed=11)
    a_d, packed_d = a.to(dev()), packed.to(dev())
    n = shape[1]
    default = run_gemm(hip_lib, form, shape, a_d, packed_d)[:, :, n:2 * n]
    forced = run_gemm(hip_lib, form, shape, a_d, packed_d, staging=1)[:, :, n:2 * n]
    assert torch.equal(default, forced)
    deep = (4096, 256, 4096)
    a, packed = make_case(form, deep, "normal", seed=12)
    a_d, packed_d = a.to(dev()), packed.to(dev())
    forced = [run_gemm(hip_lib, form, deep, a_d, packed_d, staging=s)[:, :, n:2 * n] for s in (0, 1)]
    assert torch.equal(forced[0], forced[1])
    assert not torch.equal(run_gemm(hip_lib, form, deep, a_d, packed_d)[:, :, n:2 * n], forced[1])


@pytest.mark.parametrize("form", ["NN", "TN"])
def test_nan_and_inf_operands_stay_visible(hip_lib, form):
    """x = +-Inf splits into hi = Inf, x - hi = NaN: an Inf operand gives NaN where the f32 kernel gives Inf or NaN.  Never finite."""
    shape = FULL
    m, n, k = shape
    a, packed = make_case(form, shape, "normal", seed=13)
    spots = {"nan": (0, 77, 1234, float("nan")), "inf": (3, 4001, 31, float("inf")), "-inf": (7, 130, 4095, float("-inf"))}
    for b, row, kk, val in spots.values():
        if form == "TN":
            a[b, kk, row] = val
        else:
            a[b, row, kk] = val
    out = run_gemm(hip_lib, form, shape, a.to(dev()), packed.to(dev()))[:, :, n:2 * n]
    finite = torch.isfinite(out)
    for what, (b, row, kk, val) in spots.items():
        assert not finite[b, row].any(), "%s in A[%d] row %d left finite outputs" % (what, b, row)
        finite[b, row] = True
    assert finite.all(), "a non-finite operand spread beyond its row"


def run_rownorm(hip_lib, e_d, packed_d, shape, staging=-1):
    from odvae_amd import lib as _lib
    m, n, k = shape
    out = torch.full((BATCH, m, n), float("nan"), device=dev())
    rinv = torch.full((BATCH, m), float("nan"), device=dev())
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    prev = hip_lib.odvae_gemm_select_staging(staging)
    try:
        _lib.check(hip_lib.odvae_gemm_rownorm_f32(m, n, k, e_d.data_ptr(), k, m * k, packed_d.data_ptr() + 4 * 2 * n, 3 * n, k * 3 * n,
                                                  out.data_ptr(), n, m * n, rinv.data_ptr(), m, flag.data_ptr(), BATCH, _lib.stream_ptr()),
                   "gemm_rownorm")
    finally:
        hip_lib.odvae_gemm_select_staging(prev)
    torch.cuda.synchronize()
    return out, rinv, int(flag.item())


@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["full", "ragged"])
def test_rownorm_above_the_gate(hip_lib, shape):
    """O = (E V) / l with l = the row sums of E, taken from the unsplit f32 values.  1 / l against float64 row sums: a sum of K
    non-negative f32 terms in any order is within K * 2^-24 of the exact one, relatively.  The flag: 0 on ordinary rows (rows of 1e-30
    scale included: their sums stay above 1e-30 because the largest term of a row is 1e-30 itself), 1 when a row underflows entirely."""
    m, n, k = shape
    e, packed = make_case("NN", shape, "softmax", seed=17 + m)
    e_d, packed_d = e.to(dev()), packed.to(dev())
    out, rinv, flag = run_rownorm(hip_lib, e_d, packed_d, shape)
    out_f32, rinv_f32, flag_f32 = run_rownorm(hip_lib, e_d, packed_d, shape, staging=1)
    out2, rinv2, _ = run_rownorm(hip_lib, e_d, packed_d, shape)
    assert flag == 0 and flag_f32 == 0
    assert torch.equal(out, out2) and torch.equal(rinv, rinv2)
    assert not torch.equal(out, out_f32), "the gate did not open"
    l64 = e.double().sum(dim=2)
    err_rinv = ((rinv.cpu().double() * l64) - 1.0).abs().max().item()
    c64, scale = reference("NN", shape, e, packed)
    # |O - C64 / l64| * l64 / sum|e||v|: the product's measure, the row sum's own error (<= K 2^-24 of |O|, and |C64| <= scale) beside it
    e_split = ((out.cpu().double() - c64 / l64[:, :, None]).abs() * l64[:, :, None] / scale).max().item()
    e_f32 = ((out_f32.cpu().double() - c64 / l64[:, :, None]).abs() * l64[:, :, None] / scale).max().item()
    err_rinv_f32 = ((rinv_f32.cpu().double() * l64) - 1.0).abs().max().item()
    print("\ngemm_split rownorm M=%d N=%d K=%d batch=%d: e_split %.3e  e_f32 %.3e  bound %.3e  |rinv * l64 - 1| split %.3e f32 %.3e (bound %.3e)"
          % (m, n, k, BATCH, e_split, e_f32, e_f32 + 2.0 ** -22 + err_rinv + err_rinv_f32, err_rinv, err_rinv_f32, k * 2.0 ** -24))
    assert err_rinv <= k * 2.0 ** -24
    # each kernel's O carries its own row sum's relative error (|C64| <= scale), the two sums run in different orders
    assert e_split <= e_f32 + 2.0 ** -22 + err_rinv + err_rinv_f32
    # one row underflows entirely: the flag goes up (the caller's predicated fallback would then redo the block), as in the f32 kernel
    e_d[2, 1000] = 0.0
    _, _, flag = run_rownorm(hip_lib, e_d, packed_d, shape)
    _, _, flag_f32 = run_rownorm(hip_lib, e_d, packed_d, shape, staging=1)
    assert flag == 1 and flag_f32 == 1


def test_attention_at_full_token_count_matches_float64(hip_lib):
    """attention_qkv at n = 8, C = 256, 64 x 64 tokens -- all four T-deep products above the gate -- against float64 attention on the
    CPU, forward and d(qkv), at the tolerances of test_ops_gpu.py's test_attention."""
    from odvae_amd import ops
    n, c, h, w = 8, 256, 64, 64
    t = h * w
    g = torch.Generator().manual_seed(29)
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

    def check(a, b, tol, what):
        a, b = a.detach().cpu().double(), b.detach()
        err, ref = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
        print("\ngemm_split attention %s: max err %.3e, allowed %.1e * %.3e" % (what, err, tol, ref))
        assert err <= tol * ref, what

    check(o, o_ref, FWD_TOL, "forward")
    check(qd.grad, qr.grad, BWD_TOL, "d(qkv)")
