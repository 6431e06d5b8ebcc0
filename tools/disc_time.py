"""The PatchGAN discriminator alone, f32 (im2col + GEMM) beside f32 implicit (ops.DISC_F32_IMPLICIT) and bf16
(NLayerDiscriminator.set_precision), B = 32 at 256 x 256, in one process:
  * the discriminator step -- forward on a real and a fake batch, hinge loss, backward to the weights -- and the generator-side pass --
    forward on the reconstruction, backward to the image (no weight gradient) -- in windows that alternate between the three arms;
  * peak device memory of one discriminator step in each arm;
  * the f32 layers one at a time, implicit (odvae_conv4x4_f32 / odvae_conv4x4_wgrad_f32 on preallocated buffers) beside the im2col form
    (reorder + im2col + GEMM | GEMM + col2im | GEMM + reorder, the calls of ops._Conv4x4), windows alternating;
  * the bf16 layers one at a time through the C ABI on preallocated buffers (no autograd node, no allocation): forward, data gradient,
    weight gradient of each 4x4 conv, executed TFLOP/s = 2 * 16 * Cin * Cout * N * Ho * Wo / time, and BatchNorm + LeakyReLU forward /
    backward with their HBM traffic.
Timing: one HIP event pair around `reps` calls queued back to back, one synchronise per window; the median over the rounds is reported,
with the spread (min .. max) beside it.
usage: python tools/disc_time.py [--reps R] [--rounds K] [--batch B] [--res RES] [--json PATH]"""
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
    return {"median_ms": statistics.median(v), "mean_ms": statistics.mean(v), "min_ms": min(v), "max_ms": max(v)}


def layers_of(res):
    """(cin, cout, stride, input side, output side, what follows) of NLayerDiscriminator(3, 64, 3)"""
    out, side = [], res
    for cin, cout, stride, post in ((3, 64, 2, "lrelu"), (64, 128, 2, "bn"), (128, 256, 2, "bn"), (256, 512, 1, "bn"), (512, 1, 1, None)):
        so = (side + 2 - 4) // stride + 1
        out.append((cin, cout, stride, side, so, post))
        side = so
    return out


def whole_net(batch, res, reps, rounds):
    import warnings
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = NLayerDiscriminator().apply(weights_init).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(0)
    real = (torch.rand(batch, 3, res, res, device=dev, generator=g) * 2 - 1).contiguous(memory_format=torch.channels_last)
    fake = (real + 0.3 * torch.randn(batch, 3, res, res, device=dev, generator=g)).clamp(-1, 1).contiguous(memory_format=torch.channels_last)
    rec = fake.clone().requires_grad_(True)
    params = list(net.parameters())
    from odvae_amd import ops
    arms = (("f32", 32, False), ("f32 implicit", 32, True), ("bf16", "bf16", False))

    def disc_step():
        lr, lf = net(real), net(fake)
        loss = 0.5 * (torch.relu(1.0 - lr).mean() + torch.relu(1.0 + lf).mean())
        loss.backward()
        for p in params:
            p.grad = None

    def gen_side():
        for p in params:
            p.requires_grad_(False)
        (-net(rec).mean()).backward()
        rec.grad = None
        for p in params:
            p.requires_grad_(True)

    times = {(n, k): [] for n, _, _ in arms for k in ("disc_step", "gen_side")}
    peak = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, prec, implicit in arms:       # packs, workspaces, allocator pools; then the peak of one step
            net.set_precision(prec)
            ops.DISC_F32_IMPLICIT = implicit
            disc_step(); gen_side(); disc_step()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            disc_step()
            torch.cuda.synchronize()
            peak[name] = {"peak_over_resident_mb": (torch.cuda.max_memory_allocated(dev) - base) / 1e6, "resident_mb": base / 1e6}
        for _ in range(rounds):
            for name, prec, implicit in arms:
                net.set_precision(prec)
                ops.DISC_F32_IMPLICIT = implicit
                times[(name, "disc_step")].append(window(disc_step, reps))
                times[(name, "gen_side")].append(window(gen_side, reps))
    ops.DISC_F32_IMPLICIT = False
    return {"%s %s" % k: med(v) for k, v in times.items()}, peak


def per_layer_f32(batch, res, reps, rounds):
    """each 4x4 conv in f32: the implicit kernels through the C ABI beside the im2col form's calls, alternating windows"""
    from odvae_amd import lib, ops
    dev = torch.device("cuda:0")
    L, st = lib.load(), lib.stream_ptr()
    rows = []
    for cin, cout, stride, si, so, post in layers_of(res):
        g = torch.Generator(device=dev).manual_seed(cin + cout)
        w = torch.randn(cout, cin, 4, 4, device=dev, generator=g) * 0.02
        b = torch.zeros(cout, device=dev)
        fwd, dgr = ops._pack_conv3x3_now(w, True, True, "c4x4s%d" % stride)
        x = torch.randn(batch, si, si, cin, device=dev, generator=g)
        y = torch.empty(batch, so, so, cout, device=dev)
        dy = torch.randn(batch, so, so, cout, device=dev, generator=g)
        dx = torch.empty(batch, si, si, cin, device=dev)
        dw, db = torch.empty(cout, cin, 4, 4, device=dev), torch.empty(cout, device=dev)
        need = L.odvae_conv4x4_wgrad_workspace_bytes(stride, batch, so, so, cin, cout)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        # the im2col form: Cout = 1 runs zero-padded to 4 channels (ops.conv4x4)
        cg = cout if cout % 4 == 0 else cout + 4 - cout % 4
        m, k = batch * so * so, 16 * cin
        wp = torch.zeros(cg, cin, 4, 4, device=dev); wp[:cout] = w
        bp = torch.zeros(cg, device=dev)
        wg, cols, dcols = torch.empty(cg, k, device=dev), torch.empty(m, k, device=dev), torch.empty(m, k, device=dev)
        yg, dyg = torch.empty(m, cg, device=dev), torch.randn(m, cg, device=dev, generator=g)
        dwg, dwo = torch.empty(cg, k, device=dev), torch.empty(cg, cin, 4, 4, device=dev)

        def i_fwd():
            lib.check(L.odvae_conv4x4_f32(stride, 0, x.data_ptr(), batch, si, si, cin, fwd.data_ptr(), cout, b.data_ptr(), y.data_ptr(), so, so, st), "fwd")

        def i_dgrad():
            lib.check(L.odvae_conv4x4_f32(stride, 1, dy.data_ptr(), batch, so, so, cout, dgr.data_ptr(), cin, None, dx.data_ptr(), si, si, st), "dgrad")

        def i_wgrad():
            lib.check(L.odvae_conv4x4_wgrad_f32(stride, x.data_ptr(), dy.data_ptr(), batch, si, si, cin, so, so, cout, dw.data_ptr(), db.data_ptr(),
                                                ws.data_ptr(), need, st), "wgrad")

        def c_fwd():
            lib.check(L.odvae_weight4x4_reorder_f32(wp.data_ptr(), wg.data_ptr(), cg, cin, 1, st), "reorder")
            lib.check(L.odvae_im2col4x4_f32(x.data_ptr(), cols.data_ptr(), batch, si, si, cin, so, so, stride, st), "im2col")
            ops.gemm(0, 1, m, cg, k, 1.0, cols, k, 0, wg, k, 0, yg, cg, 0, bp)

        def c_dgrad():
            ops.gemm(0, 0, m, k, cg, 1.0, dyg, cg, 0, wg, k, 0, dcols, k, 0)
            lib.check(L.odvae_col2im4x4_f32(dcols.data_ptr(), dx.data_ptr(), batch, si, si, cin, so, so, stride, st), "col2im")

        def c_wgrad():
            ops.gemm(1, 0, cg, k, m, 1.0, dyg, cg, 0, cols, k, 0, dwg, k, 0)
            lib.check(L.odvae_weight4x4_reorder_f32(dwg.data_ptr(), dwo.data_ptr(), cg, cin, 0, st), "reorder")
            ops._colsum(dyg, m, cg)
        flop = 2.0 * 16 * cin * cout * batch * so * so
        row = {"cin": cin, "cout": cout, "stride": stride, "in": si, "out": so, "gflop": flop / 1e9}
        for name, fi, fc in (("fwd", i_fwd, c_fwd), ("dgrad", i_dgrad, c_dgrad), ("wgrad", i_wgrad, c_wgrad)):
            fi(); fc(); torch.cuda.synchronize()
            ti, tc = [], []
            for _ in range(rounds):
                ti.append(window(fi, reps)); tc.append(window(fc, reps))
            row[name], row[name + "_im2col"] = med(ti), med(tc)
            row[name]["tflops"] = flop / row[name]["median_ms"] / 1e9
            row[name + "_im2col"]["tflops"] = flop / row[name + "_im2col"]["median_ms"] / 1e9
        rows.append(row)
    return rows


def per_layer(batch, res, reps, rounds):
    from odvae_amd import lib, ops
    dev = torch.device("cuda:0")
    L, st = lib.load(), lib.stream_ptr()
    rows = []
    for cin, cout, stride, si, so, post in layers_of(res):
        cx, cp = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
        out_f32 = cout % 8 != 0
        g = torch.Generator(device=dev).manual_seed(cin + cout)
        w = torch.randn(cout, cin, 4, 4, device=dev, generator=g) * 0.02
        b = torch.zeros(cout, device=dev)
        fwd, dgr = ops._pack_conv3x3_now(w, True, True, "bf16")
        x = torch.randn(batch, si, si, cx, device=dev, generator=g).to(BF)
        y = torch.empty(batch, so, so, cout, device=dev, dtype=torch.float32 if out_f32 else BF)
        dy = torch.randn(batch, so, so, cp, device=dev, generator=g).to(BF)
        dx = torch.empty(batch, si, si, cin, device=dev, dtype=torch.float32 if cin % 8 else BF)
        dw = torch.empty(cp, cx, 4, 4, device=dev)
        db = torch.empty(cp, device=dev)
        mode = 5 if stride == 1 else 6
        need = L.odvae_conv_wgrad_bf16_workspace_bytes(mode, batch, so, so, cx, cp)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        slope = 0.2 if post == "lrelu" else 0.0

        def k_fwd():
            lib.check(L.odvae_conv4x4_bf16(stride, 0, x.data_ptr(), batch, si, si, cx, fwd.data_ptr(), cout, b.data_ptr(), y.data_ptr(), so, so,
                                           int(out_f32), slope, st), "conv4x4 fwd")

        def k_dgrad():
            lib.check(L.odvae_conv4x4_bf16(stride, 1, dy.data_ptr(), batch, so, so, cp, dgr.data_ptr(), cin, None, dx.data_ptr(), si, si,
                                           int(cin % 8 != 0), 0.0, st), "conv4x4 dgrad")

        def k_wgrad():
            lib.check(L.odvae_conv_wgrad_bf16(mode, x.data_ptr(), dy.data_ptr(), batch, si, si, cx, so, so, cp, dw.data_ptr(), db.data_ptr(),
                                              ws.data_ptr(), need, st), "conv4x4 wgrad")
        flop = 2.0 * 16 * cin * cout * batch * so * so
        row = {"cin": cin, "cout": cout, "stride": stride, "in": si, "out": so, "gflop": flop / 1e9}
        for name, fn in (("fwd", k_fwd), ("dgrad", k_dgrad), ("wgrad", k_wgrad)):
            fn(); torch.cuda.synchronize()
            row[name] = med([window(fn, reps) for _ in range(rounds)])
            row[name]["tflops"] = flop / row[name]["median_ms"] / 1e9
        if post == "bn":
            rws = batch * so * so
            yb = torch.randn(rws, cout, device=dev, generator=g).to(BF)
            ob, gb, dxb = torch.empty_like(yb), torch.randn(rws, cout, device=dev, generator=g).to(BF), torch.empty_like(yb)
            gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
            mean, rstd, rm, rv = (torch.zeros(cout, device=dev) for _ in range(4))
            dg, dbt = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
            nb = L.odvae_batchnorm_workspace_bytes(rws, cout)
            wsb = torch.empty(nb, dtype=torch.uint8, device=dev)

            def k_bn_fwd():
                lib.check(L.odvae_batchnorm_lrelu_fwd_bf16(yb.data_ptr(), rws, cout, gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, 0.2, 1, mean.data_ptr(),
                                                           rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ob.data_ptr(), wsb.data_ptr(), nb, st), "bn fwd")

            def k_bn_bwd():
                lib.check(L.odvae_batchnorm_lrelu_bwd_bf16(yb.data_ptr(), gb.data_ptr(), rws, cout, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                                           rstd.data_ptr(), 0.2, 1, dxb.data_ptr(), dg.data_ptr(), dbt.data_ptr(), wsb.data_ptr(), nb, st), "bn bwd")
            for name, fn, passes in (("bn_fwd", k_bn_fwd, 3), ("bn_bwd", k_bn_bwd, 5)):     # tensor passes over HBM: read, read + write | 2 reads, 2 reads + write
                fn(); torch.cuda.synchronize()
                row[name] = med([window(fn, reps) for _ in range(rounds)])
                row[name]["tbytes_per_s"] = passes * 2.0 * rws * cout / row[name]["median_ms"] / 1e9
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
    rec["whole_net"], rec["peak_memory"] = whole_net(a.batch, a.res, a.reps, a.rounds)
    for name, r in rec["whole_net"].items():
        print("%-15s: median %8.3f ms, mean %8.3f (min %.3f .. max %.3f)" % (name, r["median_ms"], r["mean_ms"], r["min_ms"], r["max_ms"]), flush=True)
    for what in ("disc_step", "gen_side"):
        f = rec["whole_net"]["f32 " + what]
        for arm in ("f32 implicit", "bf16"):
            b = rec["whole_net"]["%s %s" % (arm, what)]
            print("%s: %s / f32 = %.3f; ranges %s" % (what, arm, b["median_ms"] / f["median_ms"],
                                                      "apart" if b["max_ms"] < f["min_ms"] or f["max_ms"] < b["min_ms"] else "OVERLAP"))
    for name, r in rec["peak_memory"].items():
        print("peak memory of one discriminator step, %-12s: %9.1f MB over %.1f MB resident" % (name, r["peak_over_resident_mb"], r["resident_mb"]))
    rec["layers_f32"] = per_layer_f32(a.batch, a.res, max(a.reps, 10), a.rounds)
    for r in rec["layers_f32"]:
        line = "f32 %4d -> %4d s%d %3d -> %3d %8.1f GFLOP |" % (r["cin"], r["cout"], r["stride"], r["in"], r["out"], r["gflop"])
        for k in ("fwd", "dgrad", "wgrad"):
            i, c = r[k], r[k + "_im2col"]
            line += " %s implicit %7.3f ms (%.3f .. %.3f) %5.1f TFLOP/s, im2col %7.3f ms (%.3f .. %.3f) |" % (
                k, i["median_ms"], i["min_ms"], i["max_ms"], i["tflops"], c["median_ms"], c["min_ms"], c["max_ms"])
        print(line, flush=True)
    rec["layers"] = per_layer(a.batch, a.res, max(a.reps, 10), a.rounds)
    for r in rec["layers"]:
        line = "%4d -> %4d s%d %3d -> %3d %8.1f GFLOP |" % (r["cin"], r["cout"], r["stride"], r["in"], r["out"], r["gflop"])
        for k in ("fwd", "dgrad", "wgrad"):
            line += " %s %7.3f ms %6.1f TFLOP/s |" % (k, r[k]["median_ms"], r[k]["tflops"])
        for k in ("bn_fwd", "bn_bwd"):
            if k in r:
                line += " %s %7.3f ms %5.2f TB/s |" % (k, r[k]["median_ms"], r[k]["tbytes_per_s"])
        print(line, flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
