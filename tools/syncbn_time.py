"""What cutting BatchNorm + LeakyReLU at the exchange costs on one GPU: the split route of synchronised BatchNorm (records -> merge ->
apply; sums -> dx; odvae_batchnorm_sync_* with ONE in-process "rank", no collective) beside the monolithic calls
(odvae_batchnorm_lrelu_fwd / _bwd, train = 1) at the PatchGAN's three BatchNorm layers of BASELINE configs[3] (256 x 256, B = 32):
rows x C = 131072 x 128, 32768 x 256, 30752 x 512, f32 and bf16.  The split route launches one more small kernel forward (record, merge
against finalize) and one more backward (the merge of the sums) and writes / reads a few KB of f64; the tensor passes are the same.
Timing: one HIP event pair around `reps` calls queued back to back through the C ABI on preallocated buffers (no autograd node, no
allocation: the queue stays full), one synchronise per window; the variants' windows alternate; the median over the rounds is reported.
The exchange itself (an RCCL all-reduce of world x C x 24 bytes forward and world x C x 16 backward, per layer) cannot be measured on
one GPU and is not estimated here.
usage: python tools/syncbn_time.py [--reps R] [--rounds K] [--json PATH] [--md PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(131072, 128), (32768, 256), (30752, 512)]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_times(rows, c, bf, reps, rounds):
    from odvae_amd import lib
    L, st = lib.load(), lib.stream_ptr()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if bf else torch.float32
    sfx = "bf16" if bf else "f32"
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(rows, c, device=dev, generator=g) * 0.7 + 0.3).to(dt)
    dy = torch.randn(rows, c, device=dev, generator=g).to(dt)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    f = lambda *s: torch.empty(*s, device=dev)
    gamma, beta, mean, rstd, dgamma, dbeta = torch.ones(c, device=dev), torch.zeros(c, device=dev), f(c), f(c), f(c), f(c)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    record = torch.zeros(1, c, 3, dtype=torch.float64, device=dev)
    sums = torch.zeros(1, 2, c, dtype=torch.float64, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    wp, wn = lib.workspace.get(L.odvae_batchnorm_workspace_bytes(rows, c), dev)
    P = lambda t: t.data_ptr()
    fwd, bwd = getattr(L, "odvae_batchnorm_lrelu_fwd_" + sfx), getattr(L, "odvae_batchnorm_lrelu_bwd_" + sfx)
    rec_fn, sums_fn, dx_fn = (getattr(L, "odvae_batchnorm_sync_%s_%s" % (k, sfx)) for k in ("stats_record", "bwd_sums", "bwd_dx"))

    def mono_fwd():
        lib.check(fwd(P(x), rows, c, P(gamma), P(beta), 1e-5, 0.1, 0.2, 1, P(mean), P(rstd), P(rm), P(rv), P(y), wp, wn, st), "fwd")

    def mono_bwd():
        lib.check(bwd(P(x), P(dy), rows, c, P(gamma), P(beta), P(mean), P(rstd), 0.2, 1, P(dx), P(dgamma), P(dbeta), wp, wn, st), "bwd")

    def split_fwd():
        lib.check(rec_fn(P(x), rows, c, P(record), c * 24, wp, wn, st), "record")
        lib.check(L.odvae_batchnorm_sync_stats_merge(P(record), c * 24, 1, c, 1e-5, 0.1, P(mean), P(rstd), P(rm), P(rv), P(total), st), "merge")
        lib.check(fwd(P(x), rows, c, P(gamma), P(beta), 1e-5, 0.1, 0.2, 0, P(mean), P(rstd), None, None, P(y), None, 0, st), "apply")

    def split_bwd():
        lib.check(sums_fn(P(x), P(dy), rows, c, P(gamma), P(beta), P(mean), P(rstd), 0.2, P(sums), c * 16, P(dgamma), P(dbeta), wp, wn, st), "sums")
        lib.check(dx_fn(P(x), P(dy), rows, c, P(gamma), P(beta), P(mean), P(rstd), 0.2, P(sums), c * 16, 1, P(total), P(dx), wp, wn, st), "dx")

    variants = {"monolithic fwd": mono_fwd, "split fwd": split_fwd, "monolithic bwd": mono_bwd, "split bwd": split_bwd}
    times = {k: [] for k in variants}
    for fn in variants.values():      # warm-up: code objects, the workspace; the forwards leave mean / rstd for the backwards
        window(fn, 3)
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps))
    ms = {k: statistics.median(v) for k, v in times.items()}
    res = {"rows": rows, "C": c, "dtype": sfx, "ms": ms, "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()},
           "split_minus_monolithic_us": {d: 1e3 * (ms["split " + d] - ms["monolithic " + d]) for d in ("fwd", "bwd")}}
    print("%s rows %d C %d" % (sfx, rows, c))
    for k in variants:
        print("  %-16s median %8.4f ms   min %8.4f   max %8.4f" % (k, ms[k], res["ms_min"][k], res["ms_max"][k]), flush=True)
    return res


def markdown(res):
    lines = ["# Synchronised BatchNorm: what the cut at the exchange costs on one GPU", "",
             "Written by `tools/syncbn_time.py` (reps %d, rounds %d; device: %s)." % (res["reps"], res["rounds"], res["device"]), "",
             "`lightning.trainer.sync_batchnorm` runs the PatchGAN's BatchNorm + LeakyReLU as records -> exchange -> merge -> apply and",
             "sums -> exchange -> dx (`odvae_batchnorm_sync_*`) in place of the two monolithic calls.  Below: the split route with ONE in-process",
             "\"rank\" and no collective beside the monolithic calls, through the C ABI on preallocated buffers, at the three BatchNorm layers of",
             "BASELINE configs[3] (256 x 256, B = 32).  One HIP event pair around a window of calls queued back to back, one synchronise per",
             "window, windows alternating between the variants; medians over the rounds, milliseconds per call (min .. max over the rounds).", "",
             "| dtype | rows x C | monolithic fwd | split fwd | split - monolithic | monolithic bwd | split bwd | split - monolithic |",
             "|---|---|---|---|---|---|---|---|"]
    cell = lambda r, k: "%.4f (%.4f .. %.4f)" % (r["ms"][k], r["ms_min"][k], r["ms_max"][k])
    for r in res["layers"]:
        lines.append("| %s | %d x %d | %s | %s | %+.1f us | %s | %s | %+.1f us |" % (
            r["dtype"], r["rows"], r["C"], cell(r, "monolithic fwd"), cell(r, "split fwd"), r["split_minus_monolithic_us"]["fwd"],
            cell(r, "monolithic bwd"), cell(r, "split bwd"), r["split_minus_monolithic_us"]["bwd"]))
    lines += ["",
              "The values are recorded, not held to a threshold.  The split route is taken only when the key is on and the group has more than",
              "one rank; with the key off the monolithic calls run as before.", "",
              "## Not measured", "",
              "The exchange itself: per layer one all-reduce of world x C x 24 bytes in the forward and one of world x C x 16 bytes in the backward",
              "(3 to 12 KB per rank at these widths), latency-bound, three layers, three discriminator forwards and up to three backwards per GAN",
              "batch.  RCCL with more than one rank has never run on the one-GPU lease this project is developed on (the two-rank tests use gloo on",
              "one device, which moves the buffers through the host and says nothing about RCCL), so its cost is **not measured** and no scaling",
              "number is claimed for `sync_batchnorm`."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "syncbn.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("syncbn_time: needs the GPU (a timing taken elsewhere says nothing)")
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "layers": [layer_times(rows, c, bf, a.reps, a.rounds) for bf in (False, True) for rows, c in SHAPES]}
    print(json.dumps(res), flush=True)
    for path, text in ((a.json, json.dumps(res)), (a.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
