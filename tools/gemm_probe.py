"""GEMM timings at the attention / 1x1 shapes of the step (B = 32)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odvae_amd import ops, lib as _lib
if os.environ.get("ODVAE_PROBE_LIB"):      # A/B builds of the library (tools/bin/, not shipped)
    _lib.LIB_PATH = os.environ["ODVAE_PROBE_LIB"]

def timeit(fn, iters=30):
    for _ in range(15): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters

dev = torch.device("cuda:0"); B = 32
cases = [("S=QK^T   NT", 4096, 4096, 256, B, 0, 1), ("O=PV     NN", 4096, 256, 4096, B, 0, 0), ("dV=P^TdO TN", 4096, 256, 4096, B, 1, 0),
         ("dP=dOV^T NT", 4096, 4096, 256, B, 0, 1), ("1x1 fwd qkv NT", B * 4096, 768, 256, 1, 0, 1), ("1x1 dgrad NN", B * 4096, 256, 768, 1, 0, 0),
         ("1x1 wgrad TN", 768, 256, B * 4096, 1, 1, 0), ("nin 128->256 @128", B * 16384, 256, 128, 1, 0, 1)]
for name, m, n, k, batch, ta, tb in cases:
    a = torch.randn(batch, (k if ta else m), (m if ta else k), device=dev)
    b = torch.randn(batch, (n if tb else k), (k if tb else n), device=dev)
    c = torch.empty(batch, m, n, device=dev)
    t = timeit(lambda: ops.gemm(ta, tb, m, n, k, 1.0, a, a.shape[2], a.shape[1] * a.shape[2], b, b.shape[2], b.shape[1] * b.shape[2], c, n, m * n, batch=batch))
    print("%-18s M%7d N%5d K%7d b%2d: %8.3f ms  %6.1f TFLOP/s" % (name, m, n, k, batch, t, 2.0 * m * n * k * batch / t / 1e9))

# the two T x T products with their epilogues: default dispatch (the bf16-split kernel at these shapes) against forced staging (f32 MFMA)
L, T, K = _lib.load(), 4096, 256
q, kk = torch.randn(B, T, K, device=dev), torch.randn(B, T, K, device=dev)
bound, drow, rinv = torch.full((B, T), 64.0, device=dev), torch.randn(B, T, device=dev), torch.rand(B, T, device=dev) + 0.5
e, ds = torch.rand(B, T, T, device=dev), torch.empty(B, T, T, device=dev)
tt = [("E=exp(QK^T-b) NT", lambda: _lib.check(L.odvae_gemm_exp_bound_f32(T, T, K, K ** -0.5, q.data_ptr(), K, T * K, kk.data_ptr(), K, T * K, bound.data_ptr(), T,
                                                                          ds.data_ptr(), T, T * T, B, _lib.stream_ptr()), "gemm_exp_bound")),
      ("dS=E(dOV^T-D) NT", lambda: _lib.check(L.odvae_gemm_softmax_bwd_scaled_f32(T, T, K, K ** -0.5, q.data_ptr(), K, T * K, kk.data_ptr(), K, T * K, e.data_ptr(),
                                                                                   drow.data_ptr(), rinv.data_ptr(), T, ds.data_ptr(), T, T * T, B,
                                                                                   _lib.stream_ptr()), "gemm_softmax_bwd_scaled"))]
for name, fn in tt:
    for mode, what in ((-1, "default"), (0, "f32 MFMA")):
        prev = L.odvae_gemm_select_staging(mode)
        t = timeit(fn)
        L.odvae_gemm_select_staging(prev)
        print("%-18s M%7d N%5d K%7d b%2d: %8.3f ms  %6.1f TFLOP/s  (%s)" % (name, T, T, K, B, t, 2.0 * T * T * K * B / t / 1e9, what))
