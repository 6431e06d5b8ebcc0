"""f32 attention block (ops.attention_qkv): the fused kernels (ODVAE_ATTN_F32_FUSED, flash_attn_f32.hip) against today's GEMM path,
forward and backward time from HIP events around launches on a full queue (no per-iteration synchronise), alternating the two paths.
usage: python tools/attn_f32_time.py [N] [C] [H]      (default: the benchmark's block, N = 32, C = 256, 64 x 64 tokens; run under
rocprofv3 --kernel-trace --stats for the per-kernel split)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_PEAK = 157.3   # TFLOP/s, exact-f32 MFMA (MI355X_MICROARCH.md)


def main():
    from odvae_amd import ops
    n, c, h = (int(v) for v in (sys.argv[1:4] if len(sys.argv) > 3 else (32, 256, 64)))
    t = h * h
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(n, 3 * c, h, h, device=dev, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    go = torch.randn(n, c, h, h, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    reps = 4
    for rnd in range(3):
        for fused in (False, True):
            ops.ATTN_F32_FUSED = fused
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
            ev[0].record()
            for i in range(reps):
                o = ops.attention_qkv(qkv)
                ev[2 * i + 1].record()
                o.backward(go)
                ev[2 * i + 2].record()
                qkv.grad = None
            torch.cuda.synchronize()
            tf = sum(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps)) / reps
            tb = sum(ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(reps)) / reps
            if rnd == 0:
                continue   # warm-up round
            issued_f, issued_b = 4.0 * t * t * c * n, (16.0 if c == 512 else 14.0) * t * t * c * n
            if not fused:
                issued_b = 8.0 * t * t * c * n
            print("N=%d C=%d T=%d %s  forward %.3f ms (%.2f of f32 peak)  backward %.3f ms (%.2f of peak on issued work)" % (
                n, c, t, "fused" if fused else "gemm ", tf, issued_f / tf / 1e9 / F32_PEAK, tb, issued_b / tb / 1e9 / F32_PEAK), flush=True)


if __name__ == "__main__":
    main()
