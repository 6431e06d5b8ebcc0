"""The perceptual term alone, f32 beside bf16 (LPIPSStyle.set_precision), B = 32 at 256 x 256, in one process:
  * the whole term as a generator step runs it -- both feature forwards (input without a graph, reconstruction with one), the five
    distance taps and the backward to the reconstruction -- in windows that alternate between the two precisions;
  * the bf16 VGG layers one class at a time through the C ABI on preallocated buffers (no autograd node, no allocation): conv + ReLU
    forward (odvae_conv_bf16_relu) and masked data gradient (odvae_conv_bf16_masked), executed TFLOP/s = 2 * 9 * Cin * Cout * N * H * W / time.
Timing: one HIP event pair around `reps` calls queued back to back, one synchronise per window; the median over the rounds is reported,
with the spread (min .. max) beside it.
usage: python tools/lpips_time.py [--reps R] [--rounds K] [--batch B] [--res RES] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def vgg_flop(batch, res):
    """multiply-add FLOP of one feature forward (direct form) and the layer classes (cin, cout, side, count)"""
    from odvae_amd.gan import VGG16_SLICES
    classes, total, side = {}, 0.0, res
    for k, (_, convs) in enumerate(VGG16_SLICES):
        if k > 0:
            side //= 2
        for _, cin, cout in convs:
            classes[(cin, cout, side)] = classes.get((cin, cout, side), 0) + 1
            total += 2.0 * 9 * cin * cout * batch * side * side
    return total, classes


def whole_term(batch, res, reps, rounds):
    import warnings
    from odvae_amd.gan import LPIPSStyle
    dev = torch.device("cuda:0")
    net = LPIPSStyle().to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = (torch.rand(batch, 3, res, res, device=dev, generator=g) * 2 - 1).contiguous(memory_format=torch.channels_last)
    x1 = (x0 + 0.3 * torch.randn(batch, 3, res, res, device=dev, generator=g)).clamp(-1, 1).contiguous(memory_format=torch.channels_last).requires_grad_(True)

    def term():
        net(x0, x1).sum().backward()
        x1.grad = None

    times = {"f32": [], "bf16": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for prec in (32, "bf16"):           # packs, workspaces, allocator pools
            net.set_precision(prec)
            term(); term()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, prec in (("f32", 32), ("bf16", "bf16")):
                net.set_precision(prec)
                times[name].append(window(term, reps))
    flop_fwd, _ = vgg_flop(batch, res)
    out = {}
    for name in times:
        out[name] = med(times[name])
        # two forwards + the data gradients of every layer but the image layer's (its 3-channel gradient is 3/64 of a layer)
        out[name]["algorithmic_tflops"] = 3.0 * flop_fwd / out[name]["median_ms"] / 1e9
    return out


def layer_classes(batch, res, reps, rounds):
    from odvae_amd import lib, ops
    dev = torch.device("cuda:0")
    L, st = lib.load(), lib.stream_ptr()
    _, classes = vgg_flop(batch, res)
    rows = []
    for (cin, cout, side), count in classes.items():
        cx = 8 if cin == 3 else cin
        g = torch.Generator(device=dev).manual_seed(cin + cout)
        w = torch.nn.Parameter(torch.randn(cout, cin, 3, 3, device=dev, generator=g) * (2.0 / (9 * cin)) ** 0.5, requires_grad=False)
        b = torch.zeros(cout, device=dev)
        fwd, dgr = ops.pack_conv3x3(w, True, True, "bf16")
        x = torch.relu(torch.randn(batch, side, side, cx, device=dev, generator=g)).to(BF)
        y = torch.empty(batch, side, side, cout, device=dev, dtype=BF)
        dy = torch.randn(batch, side, side, cout, device=dev, generator=g).to(BF)
        dx = torch.empty(batch, side, side, cx, device=dev, dtype=BF)

        def k_fwd():
            lib.check(L.odvae_conv_bf16_relu(x.data_ptr(), batch, side, side, cx, fwd.data_ptr(), cout, b.data_ptr(), y.data_ptr(), st), "conv_bf16_relu")

        def k_dgrad():
            lib.check(L.odvae_conv_bf16_masked(dy.data_ptr(), batch, side, side, cout, dgr.data_ptr(), cin, x.data_ptr(), dx.data_ptr(), st), "conv_bf16_masked")

        flop = 2.0 * 9 * cin * cout * batch * side * side
        row = {"cin": cin, "cout": cout, "side": side, "layers": count, "gflop": flop / 1e9}
        for name, fn in (("relu_fwd", k_fwd),) + ((("masked_dgrad", k_dgrad),) if cin > 32 else ()):
            fn(); torch.cuda.synchronize()
            t = [window(fn, reps) for _ in range(rounds)]
            row[name] = med(t)
            row[name]["tflops"] = flop / row[name]["median_ms"] / 1e9
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rec = {"batch": a.batch, "res": a.res, "reps": a.reps, "rounds": a.rounds}
    rec["whole_term"] = whole_term(a.batch, a.res, a.reps, a.rounds)
    for name, r in rec["whole_term"].items():
        print("perceptual term %-4s: %8.2f ms (min %.2f .. max %.2f), %6.1f algorithmic TFLOP/s" % (
            name, r["median_ms"], r["min_ms"], r["max_ms"], r["algorithmic_tflops"]), flush=True)
    f, b = rec["whole_term"]["f32"], rec["whole_term"]["bf16"]
    print("bf16 / f32 = %.3f; ranges %s" % (b["median_ms"] / f["median_ms"], "apart" if b["max_ms"] < f["min_ms"] or f["max_ms"] < b["min_ms"] else "OVERLAP"))
    rec["layers"] = layer_classes(a.batch, a.res, max(a.reps, 10), a.rounds)
    print("%-22s %7s %9s | %-28s | %-28s" % ("layer class", "layers", "GFLOP", "conv + ReLU forward", "masked data gradient"))
    for r in rec["layers"]:
        cell = lambda k: ("%7.3f ms %7.1f TFLOP/s" % (r[k]["median_ms"], r[k]["tflops"])) if k in r else "(f32, 3 channels: not timed)"
        print("%4d -> %4d @ %3d x %-3d %7d %9.1f | %-28s | %-28s" % (r["cin"], r["cout"], r["side"], r["side"], r["layers"], r["gflop"],
                                                                   cell("relu_fwd"), cell("masked_dgrad")))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
