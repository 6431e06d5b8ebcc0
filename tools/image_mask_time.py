"""Cost of image_mask_key (RGBA reconstruction: ddconfig.out_ch 4, disc_in_channels 4) on an MI355X.

1. odvae_rgba_terms_f32 and odvae_rgba_terms_bwd_f32 through the C ABI on preallocated buffers (no autograd dispatch, no allocation in the
   queue) against the launches they replace -- l1_masked_sum and three mul_mask forward, l1_masked_bwd and two mul_mask backward; the
   composition's slice copy, torch mask loss and gradient additions are NOT in its rows, which flatters it -- at B x 256 x 256, and
   against their algorithmic bytes at the measured HBM copy rate (6.3 TB/s): forward 36 B read + 40 B written per pixel with the three
   masked copies a generator step asks for, backward 64 B read + 16 B written with every incoming gradient present.
2. The three products of conv_out (forward, data gradient, weight gradient) through the C ABI at 128 -> 4 against 128 -> 3, whose thin
   kernels are the scale; with ODVAE_PROBE_LIB=<the parent commit's libodvae_hip.so> the same calls on that build, where 128 -> 4 takes
   the general kernels.
3. Whole training steps (both optimizers, LPIPS-style and PatchGAN terms on, the benchmark network) with the mask on and off, ALTERNATED
   over `--rounds` rounds of `--steps` steps each after `--warmup`; every figure of both series is written down.

Each row of 1 and 2 is `--iters` calls queued between one pair of events.

    python tools/image_mask_time.py [--iters 50] [--batch 32] [--res 256] [--step-batch 8] [--rounds 3] [--steps 3] [--out profiles/image_mask.md]

Only the tool's own section of the output file (between its two markers) is rewritten.
"""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
DEV = "cuda:0"
HBM_TBS = 6.3
BEGIN, END = "<!-- image_mask_time: begin -->", "<!-- image_mask_time: end -->"


def _queue(fn, iters):
    """fn() queued `iters` times between one event pair: device ms per call."""
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def terms_section(args):
    """The kernels through the C ABI on preallocated buffers: no autograd dispatch, no allocation, nothing but launches in the queue."""
    import torch
    from odvae_amd import lib
    L = lib.load()
    b, r = args.batch, args.res
    n, hw = b, r * r
    g = torch.Generator().manual_seed(3)
    rec, rgb = torch.randn(n, hw, 4, generator=g).to(DEV), (torch.rand(n, hw, 3, generator=g) * 2 - 1).to(DEV)
    alpha = (torch.rand(n, hw, generator=g) < 0.5).float().to(DEV)
    box = torch.ones(n, r, r)
    box[:, : r // 8] = 0.0
    box = box.reshape(n, hw).to(DEV)
    g_rgb, g_rgba, g_n = torch.randn(n, hw, 3, generator=g).to(DEV), torch.randn(n, hw, 4, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    l1, ms, rec_rgb_m, gt_rgb_m, rec_rgba_m, d_rec = new(n), new(n), new(n, hw, 3), new(n, hw, 3), new(n, hw, 4), new(n, hw, 4)
    rec3, d3a, d3b = rec[..., :3].contiguous(), new(n, hw, 3), new(n, hw, 3)
    nbytes = max(L.odvae_rgba_terms_workspace_bytes(n), n * 1024)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = lib.stream_ptr()
    P = lambda t: t.data_ptr()

    def fused_fwd():
        lib.check(L.odvae_rgba_terms_f32(P(rec), P(rgb), P(alpha), P(box), 1, P(l1), P(ms), P(rec_rgb_m), P(gt_rgb_m), P(rec_rgba_m), None, n, hw,
                                         P(ws), nbytes, st), "rgba_terms")

    def fused_bwd():
        lib.check(L.odvae_rgba_terms_bwd_f32(P(rec), P(rgb), P(alpha), P(box), 1, P(g_n), P(g_n), P(g_rgb), P(g_rgba), P(d_rec), n, hw, st), "rgba_terms_bwd")

    def composed_fwd():      # (without the slice copy rec[:, :3] and the mask loss, which the composition runs in torch ops)
        lib.check(L.odvae_l1_masked_sum_f32(P(rgb), P(rec3), P(box), P(l1), n, hw, 3, P(ws), nbytes, st), "l1")
        lib.check(L.odvae_mul_mask_f32(P(rgb), P(box), P(gt_rgb_m), n * hw, 3, st), "mul")
        lib.check(L.odvae_mul_mask_f32(P(rec3), P(box), P(rec_rgb_m), n * hw, 3, st), "mul")
        lib.check(L.odvae_mul_mask_f32(P(rec), P(box), P(rec_rgba_m), n * hw, 4, st), "mul")

    def composed_bwd():      # (without the additions that join the three gradients and the mask loss's backward)
        lib.check(L.odvae_l1_masked_bwd_f32(P(rgb), P(rec3), P(box), P(g_n), P(d3a), n, hw, 3, st), "l1 bwd")
        lib.check(L.odvae_mul_mask_f32(P(g_rgb), P(box), P(d3b), n * hw, 3, st), "mul")
        lib.check(L.odvae_mul_mask_f32(P(g_rgba), P(box), P(d_rec), n * hw, 4, st), "mul")

    npix = n * hw
    floor_f, floor_b = npix * 76 / (HBM_TBS * 1e12) * 1e3, npix * 80 / (HBM_TBS * 1e12) * 1e3
    it = args.iters * 4
    t_f, t_b, c_f, c_b = _queue(fused_fwd, it), _queue(fused_bwd, it), _queue(composed_fwd, it), _queue(composed_bwd, it)
    return ["## odvae_rgba_terms_f32 / _bwd_f32 against the launches they replace, C ABI on preallocated buffers (B = %d, %d x %d, l2, partial box)" % (b, r, r), "",
            "%d calls queued between one event pair per row; nothing but kernel launches in the queue." % it, "",
            "| variant | launches | device ms / call | algorithmic bytes at %.1f TB/s | share of that rate |" % HBM_TBS, "|---|---|---|---|---|",
            "| rgba_terms forward (sums + three masked copies) | 2 | %.4f | %.4f ms | %.0f %% |" % (t_f, floor_f, 100 * floor_f / t_f),
            "| rgba_terms backward (all four gradients) | 1 | %.4f | %.4f ms | %.0f %% |" % (t_b, floor_b, 100 * floor_b / t_b),
            "| l1_masked_sum + 3 x mul_mask, forward (no slice copy, no mask loss) | 5 | %.4f | | %.2f x the fused forward |" % (c_f, c_f / t_f),
            "| l1_masked_bwd + 2 x mul_mask, backward (no gradient additions, no mask-loss backward) | 3 | %.4f | | %.2f x the fused backward |" % (c_b, c_b / t_b),
            ""]


def _bind(path):
    """Another build of the library (the parent commit's, or one of tools/ab_build.py): the conv entry points alone, by the binding's prototypes."""
    import ctypes
    from odvae_amd import lib
    other = ctypes.CDLL(path)
    for name in ("odvae_conv3x3_pack_floats", "odvae_conv3x3_pack_f32", "odvae_conv3x3_f32", "odvae_conv3x3_wgrad_workspace_bytes", "odvae_conv3x3_wgrad_f32"):
        fn = getattr(other, name)
        fn.restype, fn.argtypes = lib.PROTOTYPES[name]
    return other


def conv_section(args):
    """conv_out's forward, data gradient and weight gradient through the C ABI on preallocated buffers, this build and (ODVAE_PROBE_LIB) another."""
    import torch
    from odvae_amd import lib
    b, r = args.batch, args.res
    libs = [("this commit", lib.load())]
    if os.environ.get("ODVAE_PROBE_LIB"):
        libs.append(("ODVAE_PROBE_LIB (the parent commit's build: 128 -> 4 on the general kernels)", _bind(os.environ["ODVAE_PROBE_LIB"])))
    out = ["## conv_out's three products through the C ABI, 128 -> 4 against 128 -> 3 (the thin kernels' scale), B = %d, %d x %d" % (b, r, r), "",
           "%d calls queued between one event pair per figure; two figures per cell, taken one after the other." % args.iters, "",
           "| library | Cout | forward ms | data gradient ms | weight gradient (+ bias) ms |", "|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(4)
    st = lib.stream_ptr()
    x = torch.randn(b, r, r, 128, generator=g).to(DEV)
    dx = torch.empty_like(x)
    for cout in (3, 4):
        w = (torch.randn(cout, 128, 3, 3, generator=g) * 0.05).to(DEV)
        bias, db, dw = torch.zeros(cout, device=DEV), torch.empty(cout, device=DEV), torch.empty(cout, 128, 3, 3, device=DEV)
        dy = torch.randn(b, r, r, cout, generator=g).to(DEV)
        y = torch.empty_like(dy)
        for label, L in libs:
            fwd = torch.empty(L.odvae_conv3x3_pack_floats(128, cout), device=DEV)
            dgr = torch.empty(L.odvae_conv3x3_pack_floats(cout, 128), device=DEV)
            lib.check(L.odvae_conv3x3_pack_f32(w.data_ptr(), cout, 128, fwd.data_ptr(), dgr.data_ptr(), st), "pack")
            nws = L.odvae_conv3x3_wgrad_workspace_bytes(0, b, r, r, 128, cout)
            ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
            calls = (lambda: lib.check(L.odvae_conv3x3_f32(0, x.data_ptr(), b, r, r, 128, fwd.data_ptr(), cout, bias.data_ptr(), None, y.data_ptr(), r, r, 0, st), "fwd"),
                     lambda: lib.check(L.odvae_conv3x3_f32(0, dy.data_ptr(), b, r, r, cout, dgr.data_ptr(), 128, None, None, dx.data_ptr(), r, r, 0, st), "dgrad"),
                     lambda: lib.check(L.odvae_conv3x3_wgrad_f32(0, x.data_ptr(), dy.data_ptr(), b, r, r, 128, r, r, cout, dw.data_ptr(), db.data_ptr(),
                                                                 ws.data_ptr(), nws, st), "wgrad"))
            cells = ["%.3f, %.3f" % (_queue(c, args.iters), _queue(c, args.iters)) for c in calls]
            out.append("| %s | %d | %s |" % (label, cout, " | ".join(cells)))
    return out + [""]


def step_section(args):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    b, r = args.step_batch, args.res

    def build(mask):
        mcfg, _ = synthetic.model_config(YAML, latent_hw=r // 16, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
        p = mcfg.params
        if mask:
            p["image_mask_key"] = "mask"
            p.ddconfig["out_ch"] = 4
            p.lossconfig.params["disc_in_channels"], p.lossconfig.params["mask_weight"] = 4, 0.5
        torch.manual_seed(3)
        model = instantiate_from_config(mcfg)
        model.learning_rate = b * 4.5e-6
        model = model.to(DEV).train()
        model._global_step = 1
        return model, Trainer(model, gradient_clip_val=1.0)

    series = {False: [], True: []}
    runs = {m: build(m) for m in (False, True)}
    batches = {m: synthetic.make_batch(b, r, seed=5, mask_key="mask" if m else None) for m in (False, True)}
    step = 0
    for rnd in range(args.rounds):
        for mask in (False, True):
            model, trainer = runs[mask]
            for i in range(args.warmup if rnd == 0 else 1):
                trainer.training_batch({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batches[mask].items()}, step)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                trainer.training_batch({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batches[mask].items()}, step)
            e1.record()
            torch.cuda.synchronize()
            series[mask].append(e0.elapsed_time(e1) / args.steps)
            step += 1
    fmt = lambda xs: ", ".join("%.1f" % v for v in xs)
    med = {m: statistics.median(series[m]) for m in series}
    return ["## Whole training step, both optimizers, LPIPS-style + PatchGAN terms on (ch = 128, B = %d, %d x %d, f32)" % (b, r, r), "",
            "%d rounds alternating mask off / on, %d steps per figure between one event pair." % (args.rounds, args.steps), "",
            "| image_mask_key | ms / step, every round | median |", "|---|---|---|",
            "| unset (out_ch 3) | %s | %.1f |" % (fmt(series[False]), med[False]),
            "| set (out_ch 4, disc_in_channels 4, mask loss on) | %s | %.1f |" % (fmt(series[True]), med[True]), "",
            "Mask on costs %+.1f %% of a step (spread within a series: %.1f %% and %.1f %%)." % (
                100 * (med[True] / med[False] - 1), 100 * (max(series[False]) / min(series[False]) - 1), 100 * (max(series[True]) / min(series[True]) - 1)), ""]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_mask.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("image_mask_time.py needs an MI355X: nothing here is measured on a CPU")
    warnings.simplefilter("ignore", RuntimeWarning)
    lines = [BEGIN, "", "Measured by `tools/image_mask_time.py --iters %d --batch %d --res %d --step-batch %d --rounds %d --steps %d`." % (
        args.iters, args.batch, args.res, args.step_batch, args.rounds, args.steps), ""]
    lines += terms_section(args) + conv_section(args) + step_section(args) + [END]
    text = open(args.out).read() if os.path.exists(args.out) else "# image_mask_key\n\n"
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + "\n".join(lines) + text[text.index(END) + len(END):]
    else:
        text = text.rstrip("\n") + "\n\n" + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
