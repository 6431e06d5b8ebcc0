"""float32_matmul_precision: the six attention products at T = 4 096, C = 256, batch 32 and the TN product of a 1x1 weight gradient
at 65 536 pixels, timed at each level (odvae_gemm_select_precision 0 highest, 1 high, 2 medium) through the C ABI.

Device events around a full queue (ITERS launches back to back), the levels alternating inside every repetition of one process, REPS
repetitions; printed per product and level: the median, the min .. max spread of the repetitions, and the ratio of medians to level 0.
ODVAE_PROBE_LIB=<libodvae_*.so> times another build of the library (tools/ab_build.py, or the parent commit's); a library without
odvae_gemm_select_precision is timed at level 0 only.
usage: python tools/matmul_precision_time.py [--reps 7] [--iters 20]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odvae_amd import lib as _lib  # noqa: E402

LEVELS = (0, 1, 2)
NAMES = ("highest", "high", "medium")
if os.environ.get("ODVAE_PROBE_LIB"):      # A/B builds of the library (tools/bin/, not shipped)
    _lib.LIB_PATH = os.environ["ODVAE_PROBE_LIB"]
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "odvae_gemm_select_precision"):
        del _lib.PROTOTYPES["odvae_gemm_select_precision"]
        LEVELS = (0,)


def products(L, dev, batch=32, t=4096, c=256, pixels=65536, cin=256, cout=768):
    """[(name, M, N, K, batch, what runs, launch)]: operands as the attention lays them out (q | k | v in one 3C-wide row)"""
    st = _lib.stream_ptr()
    qkv = torch.randn(batch, t, 3 * c, device=dev)
    dqkv = torch.empty_like(qkv)
    do, o = torch.randn(batch, t, c, device=dev), torch.empty(batch, t, c, device=dev)
    e, ds = torch.empty(batch, t, t, device=dev), torch.empty(batch, t, t, device=dev)
    bound = torch.full((batch, t), 64.0, device=dev)
    drow, rinv = torch.randn(batch, t, device=dev), torch.rand(batch, t, device=dev) + 0.5
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    q, k, v = (qkv.data_ptr() + 4 * i * c for i in range(3))
    dq, dk, dv = (dqkv.data_ptr() + 4 * i * c for i in range(3))
    c3, sq, scale = 3 * c, t * 3 * c, c ** -0.5
    x, dy = torch.randn(pixels, cin, device=dev), torch.randn(pixels, cout, device=dev)
    dw = torch.empty(cout, cin, device=dev)
    need = L.odvae_gemm_f32_workspace_bytes(cout, cin, pixels, 1)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    keep = (qkv, dqkv, do, o, e, ds, bound, drow, rinv, flag, x, dy, dw, ws)

    def gemm(ta, m, n, kk, a, lda, sa, b, ldb, sb, out, ldc, sc, nb, wp=None, wn=0):
        return lambda: _lib.check(L.odvae_gemm_f32(ta, 0, m, n, kk, 1.0, a, lda, sa, b, ldb, sb, out, ldc, sc, None, None, nb, wp, wn, st), "gemm_f32")

    split_tt = "split, T x T store" if t // 128 * (t // 128) * batch >= 512 and c >= 64 else "f32 MFMA"
    deep = "split" if need == 0 or pixels <= 1024 else "f32 MFMA, split-K: the level does not apply"
    out = [
        ("E = exp(QK^T - b)  NT", t, t, c, batch, split_tt,
         lambda: _lib.check(L.odvae_gemm_exp_bound_f32(t, t, c, scale, q, c3, sq, k, c3, sq, bound.data_ptr(), t, e.data_ptr(), t, t * t, batch, st), "exp_bound")),
        ("O = E V / l        NN", t, c, t, batch, "split",
         lambda: _lib.check(L.odvae_gemm_rownorm_f32(t, c, t, e.data_ptr(), t, t * t, v, c3, sq, o.data_ptr(), c, t * c, rinv.data_ptr(), t, flag.data_ptr(),
                                                     batch, st), "rownorm")),
        ("dV = E^T dO        TN", t, c, t, batch, "split", gemm(1, t, c, t, e.data_ptr(), t, t * t, do.data_ptr(), c, t * c, dv, c3, sq, batch)),
        ("dS = E (dO V^T - D) NT", t, t, c, batch, split_tt,
         lambda: _lib.check(L.odvae_gemm_softmax_bwd_scaled_f32(t, t, c, scale, do.data_ptr(), c, t * c, v, c3, sq, e.data_ptr(), drow.data_ptr(),
                                                                rinv.data_ptr(), t, ds.data_ptr(), t, t * t, batch, st), "softmax_bwd_scaled")),
        ("dQ = dS K          NN", t, c, t, batch, "split", gemm(0, t, c, t, ds.data_ptr(), t, t * t, k, c3, sq, dq, c3, sq, batch)),
        ("dK = dS^T Q        TN", t, c, t, batch, "split", gemm(1, t, c, t, ds.data_ptr(), t, t * t, q, c3, sq, dk, c3, sq, batch)),
        ("1x1 dW = dy^T x    TN", cout, cin, pixels, 1, deep,
         gemm(1, cout, cin, pixels, dy.data_ptr(), cout, 0, x.data_ptr(), cin, 0, dw.data_ptr(), cin, 0, 1, ws.data_ptr() if need else None, need)),
    ]
    return out, keep


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    L = _lib.load()
    dev = torch.device("cuda:0")
    prods, keep = products(L, dev)
    select = getattr(L, "odvae_gemm_select_precision", None) if len(LEVELS) > 1 else None
    print("library %s; %d repetitions of %d launches per product and level, levels alternating" % (_lib.LIB_PATH, args.reps, args.iters))
    print("%-24s %6s %6s %6s %3s  %-8s %9s %19s %8s %9s  %s" % ("product", "M", "N", "K", "b", "level", "median ms", "min .. max ms", "vs lvl 0", "TFLOP/s", "runs on"))
    for name, m, n, k, batch, where, fn in prods:
        ms = {level: [] for level in LEVELS}
        try:
            for _ in range(args.reps):
                for level in LEVELS:
                    if select is not None:
                        select(level)
                    ms[level].append(timed(fn, args.iters))
        finally:
            if select is not None:
                select(0)
        med = {level: sorted(v)[len(v) // 2] for level, v in ms.items()}
        for level in LEVELS:
            print("%-24s %6d %6d %6d %3d  %-8s %9.3f %8.3f .. %7.3f %8.3f %9.1f  %s"
                  % (name, m, n, k, batch, NAMES[level], med[level], min(ms[level]), max(ms[level]), med[level] / med[0],
                     2.0 * m * n * k * batch / med[level] / 1e9, where))
    del keep


if __name__ == "__main__":
    main()
