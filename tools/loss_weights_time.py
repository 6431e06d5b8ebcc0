"""Cost of the losses' `weights` map and of `cond` (disc_conditional) on an MI355X.

(a) odvae_l1_weighted_sums_f32 / _bwd_f32 against odvae_l1_masked_sum_f32 / _bwd_f32 at the same shape, through the C ABI on preallocated
    buffers, per byte each must move: x 12 B + xr 12 B (16 B where a 4-channel reconstruction is read in place) + box 4 B + weights 4 B
    (12 B per element) per pixel, the backward writes 12 B (16 B) more; the masked pair moves 28 B and 40 B.
(b) odvae_cat_mask_f32 / _bwd_f32 (3 + 2 channels) against the only composition there was: odvae_mul_mask_f32 followed by torch.cat, and
    for the backward a slice copy followed by odvae_mul_mask_f32; and per byte against odvae_mul_mask_f32 alone (16 B read + 12 B written).
(c) Whole training steps (both optimizers, LPIPS-style and PatchGAN terms on, the benchmark network) with cond, with a per-pixel weight
    map, and without either.

Every comparison ALTERNATES its variants over `--rounds` rounds inside this one call; a figure is `--iters` calls (or `--steps` steps)
queued between one event pair after a warm-up; every figure is written down, with the median and the spread (max / min - 1) of a series.
Shares of the HBM rate are against the measured copy rate of MI355X_MICROARCH.md (6.29 TB/s; the 8 TB/s specification beside it).

    python tools/loss_weights_time.py [--iters 100] [--batch 32] [--res 256] [--step-batch 8] [--rounds 5] [--steps 3] [--out profiles/loss_weights_cond.md]

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
HBM_TBS, HBM_SPEC_TBS = 6.29, 8.0
BEGIN, END = "<!-- loss_weights_time: begin -->", "<!-- loss_weights_time: end -->"


def _queue(fn, iters):
    """fn() queued `iters` times between one event pair: device ms per call."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters, rounds):
    """{name: [ms per call, one per round]}: every variant warmed up, then the variants in turn, `rounds` times"""
    import torch
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    series = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            series[k].append(_queue(fn, iters))
    return series


def rows(series, bytes_per_call, base):
    """table rows: every figure, median, spread, achieved TB/s, share of the HBM rate, and time per byte relative to `base`"""
    med = {k: statistics.median(v) for k, v in series.items()}
    per_byte = {k: med[k] / bytes_per_call[k] for k in series}
    out = ["| variant | bytes / call | ms / call, every round | median | spread | TB/s | of %.2f TB/s measured | of %.0f TB/s spec | time per byte vs `%s` |"
           % (HBM_TBS, HBM_SPEC_TBS, base), "|---|---|---|---|---|---|---|---|---|"]
    for k, v in series.items():
        rate = bytes_per_call[k] / (med[k] * 1e-3) / 1e12
        out.append("| %s | %.1f MB | %s | %.4f | %.1f %% | %.2f | %.0f %% | %.0f %% | %.2f x |" % (
            k, bytes_per_call[k] / 1e6, ", ".join("%.4f" % t for t in v), med[k], 100 * (max(v) / min(v) - 1), rate, 100 * rate / HBM_TBS,
            100 * rate / HBM_SPEC_TBS, per_byte[k] / per_byte[base]))
    return out, med, per_byte


def kernel_sections(args):
    import torch
    from odvae_amd import lib
    L = lib.load()
    n, hw = args.batch, args.res * args.res
    g = torch.Generator().manual_seed(3)
    x, xr3 = (torch.rand(n, hw, 3, generator=g) * 2 - 1).to(DEV), torch.randn(n, hw, 3, generator=g).to(DEV)
    xr4 = torch.randn(n, hw, 4, generator=g).to(DEV)
    box = torch.ones(n, args.res, args.res)
    box[:, : args.res // 8] = 0.0
    box = box.reshape(n, hw).to(DEV)
    wpx, wel = torch.rand(n, hw, generator=g).to(DEV), torch.rand(n, hw, 3, generator=g).to(DEV)
    cond, dy5 = torch.rand(n, hw, 2, generator=g).to(DEV), torch.randn(n, hw, 5, generator=g).to(DEV)
    g_n = torch.randn(n, generator=g).to(DEV)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    s0, s1, s2, d3, d4, y3, y5 = new(n), new(n), new(n), new(n, hw, 3), new(n, hw, 4), new(n, hw, 3), new(n, hw, 5)
    nbytes = max(L.odvae_l1_weighted_workspace_bytes(n), n * 1024)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = lib.stream_ptr()
    P = lambda t: t.data_ptr()
    npix = n * hw

    def wsum(xr, cr, wgt, pc):
        return lambda: lib.check(L.odvae_l1_weighted_sums_f32(P(x), P(xr), P(box), P(wgt), pc, P(s0), P(s1), P(s2), n, hw, 3, cr, P(ws), nbytes, st), "l1w")

    def wbwd(xr, cr, wgt, pc, dxr):
        return lambda: lib.check(L.odvae_l1_weighted_bwd_f32(P(x), P(xr), P(box), P(wgt), pc, P(g_n), P(g_n), P(dxr), n, hw, 3, cr, st), "l1w bwd")

    fwd = {"l1_masked_sum": lambda: lib.check(L.odvae_l1_masked_sum_f32(P(x), P(xr3), P(box), P(s0), n, hw, 3, P(ws), nbytes, st), "l1"),
           "l1_weighted_sums, per pixel, Cr 3": wsum(xr3, 3, wpx, 0), "l1_weighted_sums, per pixel, Cr 4 in place": wsum(xr4, 4, wpx, 0),
           "l1_weighted_sums, per element, Cr 3": wsum(xr3, 3, wel, 1)}
    fb = {"l1_masked_sum": 28 * npix, "l1_weighted_sums, per pixel, Cr 3": 32 * npix, "l1_weighted_sums, per pixel, Cr 4 in place": 36 * npix,
          "l1_weighted_sums, per element, Cr 3": 40 * npix}
    bwd = {"l1_masked_bwd": lambda: lib.check(L.odvae_l1_masked_bwd_f32(P(x), P(xr3), P(box), P(g_n), P(d3), n, hw, 3, st), "l1 bwd"),
           "l1_weighted_bwd, per pixel, Cr 3": wbwd(xr3, 3, wpx, 0, d3), "l1_weighted_bwd, per pixel, Cr 4 in place": wbwd(xr4, 4, wpx, 0, d4),
           "l1_weighted_bwd, per element, Cr 3": wbwd(xr3, 3, wel, 1, d3)}
    bb = {"l1_masked_bwd": 40 * npix, "l1_weighted_bwd, per pixel, Cr 3": 44 * npix, "l1_weighted_bwd, per pixel, Cr 4 in place": 52 * npix,
          "l1_weighted_bwd, per element, Cr 3": 52 * npix}

    def composed_fwd():
        lib.check(L.odvae_mul_mask_f32(P(x), P(box), P(y3), npix, 3, st), "mul")
        torch.cat((y3, cond), dim=-1, out=y5)

    def composed_bwd():
        d3.copy_(dy5[..., :3])
        lib.check(L.odvae_mul_mask_f32(P(d3), P(box), P(y3), npix, 3, st), "mul")

    cat = {"mul_mask": lambda: lib.check(L.odvae_mul_mask_f32(P(x), P(box), P(y3), npix, 3, st), "mul"),
           "cat_mask forward (3 + 2)": lambda: lib.check(L.odvae_cat_mask_f32(P(x), P(box), P(cond), P(y5), n, hw, 3, 2, st), "cat"),
           "mul_mask + torch.cat": composed_fwd,
           "cat_mask backward (3 + 2)": lambda: lib.check(L.odvae_cat_mask_bwd_f32(P(dy5), P(box), P(d3), n, hw, 3, 2, st), "cat bwd"),
           "slice copy + mul_mask": composed_bwd}
    cb = {"mul_mask": 28 * npix, "cat_mask forward (3 + 2)": 44 * npix, "mul_mask + torch.cat": 68 * npix, "cat_mask backward (3 + 2)": 28 * npix,
          "slice copy + mul_mask": 52 * npix}
    out, verdict = [], []
    for title, variants, nb, base in (("(a) weighted sums, forward", fwd, fb, "l1_masked_sum"), ("(a) weighted sums, backward", bwd, bb, "l1_masked_bwd"),
                                      ("(b) cat_mask", cat, cb, "mul_mask")):
        series = alternate(variants, args.iters, args.rounds)
        table, med, per_byte = rows(series, nb, base)
        out += ["## %s (B = %d, %d x %d, C = 3, partial box)" % (title, n, args.res, args.res), "",
                "%d calls per figure, %d rounds alternating the variants; bytes are the algorithmic ones (a composition's: every pass counted)."
                % (args.iters, args.rounds), ""] + table + [""]
        for k in series:
            if k != base and ("weighted" in k or k.startswith("cat_mask")):
                r = per_byte[k] / per_byte[base]
                verdict.append("- %s: %.2f x the time per byte of `%s` (bound 1.25): %s" % (k, r, base, "within" if r <= 1.25 else "OVER"))
        if title.startswith("(b)"):
            for ours, comp in (("cat_mask forward (3 + 2)", "mul_mask + torch.cat"), ("cat_mask backward (3 + 2)", "slice copy + mul_mask")):
                verdict.append("- %s: %.4f ms against %.4f ms for `%s`: %s" % (ours, med[ours], med[comp], comp,
                                                                                "not slower" if med[ours] <= med[comp] else "SLOWER"))
    return out + ["## Acceptance", ""] + verdict + [""]


def step_section(args):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    b, r = args.step_batch, args.res
    kinds = {"neither": {}, "cond (2 channels, disc_in_channels 5)": dict(cond_key="cond", cond_channels=2), "per-pixel weights": dict(loss_weights_key="wts")}

    def build(kw):
        torch.manual_seed(3)
        model = synthetic.build_model(YAML, batch_size_for_lr=b, latent_hw=r // 16, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0, **kw)
        model = model.to(DEV).train()
        model._global_step = 1
        batch = synthetic.make_batch(b, r, seed=5, cond_key=kw.get("cond_key"), cond_channels=kw.get("cond_channels", 2), weights_key=kw.get("loss_weights_key"))
        return Trainer(model, gradient_clip_val=1.0), batch

    runs = {k: build(kw) for k, kw in kinds.items()}
    series = {k: [] for k in kinds}
    step = 0
    for rnd in range(args.rounds):
        for k, (trainer, batch) in runs.items():
            fresh = lambda: {a: (v.clone() if torch.is_tensor(v) else v) for a, v in batch.items()}
            for _ in range(args.warmup if rnd == 0 else 1):
                trainer.training_batch(fresh(), step)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                trainer.training_batch(fresh(), step)
            e1.record()
            torch.cuda.synchronize()
            series[k].append(e0.elapsed_time(e1) / args.steps)
            step += 1
    med = {k: statistics.median(v) for k, v in series.items()}
    out = ["## (c) Whole training step, both optimizers, LPIPS-style + PatchGAN terms on (ch = 128, B = %d, %d x %d, f32)" % (b, r, r), "",
           "%d rounds alternating the three models, %d steps per figure between one event pair.  A weighted step takes the three-pass "
           "adaptive weight (the one-pass route is off under weights), so its row holds that difference too." % (args.rounds, args.steps), "",
           "| step | ms / step, every round | median | spread | against neither |", "|---|---|---|---|---|"]
    for k, v in series.items():
        out.append("| %s | %s | %.1f | %.1f %% | %+.1f %% |" % (k, ", ".join("%.1f" % t for t in v), med[k], 100 * (max(v) / min(v) - 1),
                                                               100 * (med[k] / med["neither"] - 1)))
    noise = max(100 * (max(v) / min(v) - 1) for v in series.values())
    out.append("")
    for k in series:
        if k != "neither":
            d = 100 * (med[k] / med["neither"] - 1)
            out.append("- %s: %+.1f %% on the medians, with a spread of up to %.1f %% inside a series: %s." % (
                k, d, noise, "resolved by this run" if abs(d) > noise else "inside the noise of this run, not a measured difference"))
    return out + [""]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true", help="sections (a) and (b) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_weights_cond.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loss_weights_time.py needs an MI355X: nothing here is measured on a CPU")
    warnings.simplefilter("ignore", RuntimeWarning)
    lines = [BEGIN, "", "Measured by `tools/loss_weights_time.py --iters %d --batch %d --res %d --step-batch %d --rounds %d --steps %d%s`." % (
        args.iters, args.batch, args.res, args.step_batch, args.rounds, args.steps, " --no-steps" if args.no_steps else ""), ""]
    lines += kernel_sections(args) + ([] if args.no_steps else step_section(args)) + [END]
    text = open(args.out).read() if os.path.exists(args.out) else "# weights and disc_conditional\n\n"
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
