"""Time the two entry points of csrc/patch_u8.hip on nuScenes-shaped work: 32 instances cut from six 1600x900 camera images at
S = 256.  (a) odvae_patch_crop_resize_u8 on 400-px crops, measured twice (a1, a2: the run-to-run spread); (b)
odvae_patch_reduce_resize_u8 on the same staged batch (f = 1); (c) odvae_patch_reduce_resize_u8 on 600-px (f = 2) and 900-px
(f = 3) crops.  The variants alternate inside one loop; each sample brackets 10 launches with HIP events.  Also the host half
(plan + tables + one H2D copy) per batch.  Usage (GPU box): python tools/patch_reduce_time.py [S]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from odvae_amd.patches import GpuPatcher  # noqa: E402

LAUNCHES, SAMPLES = 10, 40


def square_instances(rng, n, side):
    """n objects whose crop is a `side`-px square: extent `side` + 1 on the longer axis (truncates to side or side + 1), centred anywhere in a 1600x900 image."""
    inst = []
    for j in range(n):
        cx, cy = rng.uniform(0, 1600), rng.uniform(0, 900)
        w, h = (side + 1.0, rng.uniform(0.3, 1.0) * side) if j % 2 else (rng.uniform(0.3, 1.0) * side, side + 1.0)
        inst.append((j % 6, [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], [cx, cy]))
    return inst


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rng = np.random.default_rng(0)
    dev = [torch.from_numpy(rng.integers(0, 256, (900, 1600, 3), dtype=np.uint8)).to("cuda:0") for _ in range(6)]
    patcher = GpuPatcher(patch_height=S, box_reduce=True)
    batches = {side: square_instances(rng, 32, side) for side in (400, 600, 900)}
    staged = {side: patcher.stage(dev, inst) for side, inst in batches.items()}
    for side, st in staged.items():
        assert st["n"] == 32 and all(p.size == side for p in st["plans"]), side
    variants = [("a1 crop entry, 400 px", 400, "crop"), ("b  reduce entry, 400 px (f=1)", 400, "reduce"), ("a2 crop entry, 400 px", 400, "crop"),
                ("c  reduce entry, 600 px (f=%d)" % (600 // S), 600, "reduce"), ("c  reduce entry, 900 px (f=%d)" % (900 // S), 900, "reduce")]
    ref = patcher.launch(staged[400], entry="crop")
    got = patcher.launch(staged[400], entry="reduce")
    assert torch.equal(ref.patch, got.patch) and torch.equal(ref.mask, got.mask)
    for _, side, entry in variants:                       # warm-up: code objects, allocator
        for _ in range(LAUNCHES):
            patcher.launch(staged[side], entry=entry)
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(SAMPLES):
        for v, (_, side, entry) in enumerate(variants):
            e0.record()
            for _ in range(LAUNCHES):
                patcher.launch(staged[side], entry=entry)
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    print("S=%d, 32 instances per batch, us per launch over %d samples of %d launches (HIP events; includes launch gaps)" % (S, SAMPLES, LAUNCHES))
    for (name, _, _), t in zip(variants, times):
        t = np.sort(np.asarray(t))
        print("  %-34s min %7.1f  median %7.1f  p90 %7.1f" % (name, t[0], t[len(t) // 2], t[int(len(t) * 0.9)]))
    for side, inst in batches.items():
        reps = 30
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            patcher.stage(dev, inst)
        torch.cuda.synchronize()
        print("  host half (plan + H2D), %d px: %.1f us per batch" % (side, (time.perf_counter() - t0) / reps * 1e6))
    fresh = time.perf_counter()
    GpuPatcher(patch_height=S, box_reduce=True)._table_slot(900, True)
    print("  first use of a crop size (coefficient table 900 -> %d): %.1f us" % (S, (time.perf_counter() - fresh) * 1e6))


if __name__ == "__main__":
    main()
