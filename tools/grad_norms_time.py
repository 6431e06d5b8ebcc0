"""Cost of track_grad_norm and gradient_clip_algorithm: value on the benchmark network.

1. The segmented-norm call (odvae_grad_seg_norms_f32, per-parameter norms and their total) against the global-norm launch pair the clip
   already uses (odvae_grad_norm_f32) on the same gradient arenas: optimizer 0 and optimizer 1 of the headline model.
2. odvae_adam_step_clamp_f32 against odvae_adam_step_f32 on copies of the same arenas.
3. The host time to enqueue one tracked step's log (FusedAdam.grad_norms + the key dict + model.log_dict).
4. Whole optimizer steps of the bench.py configuration (rec+KL f32, B = 32, 256 x 256, gradient_clip_val 1.0) with tracking off, with
   track_grad_norm=2 and with gradient_clip_algorithm=value.

The alternatives of one comparison are alternated round by round inside this one process; a round queues `--iters` calls between ONE pair of
device events after a warm-up call.  Every figure is the median over the rounds with the (min .. max) spread beside it.

    python tools/grad_norms_time.py [--res 256] [--batch 32] [--iters 50] [--rounds 7] [--steps 3] [--warmup 1] [--out profiles/grad_norms.md]

Only the tool's own section of the output file (between its two markers) is rewritten.
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def _round(fn, iters):
    """fn() queued `iters` times between one event pair after one warm-up call: (host ms per call to enqueue, device ms per call)."""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) / iters
    e1.record()
    torch.cuda.synchronize()
    return host * 1e3, e0.elapsed_time(e1) / iters


def _alternate(variants, iters, rounds):
    """{name: fn} -> {name: (host list, device list)}: the variants take turns, round by round."""
    res = {name: ([], []) for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            host, dev = _round(fn, iters)
            res[name][0].append(host)
            res[name][1].append(dev)
    return res


def _fmt(xs, unit=1.0, digits=3):
    f = "%%.%df" % digits
    return (f + " (" + f + " .. " + f + ")") % (statistics.median(xs) * unit, min(xs) * unit, max(xs) * unit)


def _spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def kernel_sections(args, trainer):
    import ctypes
    import torch
    from odvae_amd import lib
    L = lib.load()
    out = []
    norm_rows, adam_rows, host_rows = [], [], []
    for idx, opt in enumerate(trainer.optimizers):
        f = opt.materialize()
        f["g"].normal_(0.0, 1e-3)
        n_par, total = len(f["params"]), f["total"]
        opt._touched.update(range(n_par))
        clip = torch.ones(2, device=f["g"].device)
        wp, wn = lib.workspace.get(1 << 20, f["g"].device)
        stream = lib.stream_ptr()

        def pair():
            lib.check(L.odvae_grad_norm_f32(f["g"].data_ptr(), total, 1.0, clip.data_ptr(), wp, wn, stream), "grad_norm")
        # the entry point itself on tables built once (FusedAdam.grad_norms adds a host walk over the parameters: timed below)
        lens = (ctypes.c_int64 * n_par)(*[q.numel() for q in f["params"]])
        offs = (ctypes.c_int64 * n_par)(*f["offsets"])
        need = int(L.odvae_grad_seg_norms_workspace_bytes(lens, n_par))
        sp, sn = lib.workspace.get(max(need, 1 << 20), f["g"].device)
        wp, wn = sp, sn
        norms = torch.zeros(n_par + 1, device=f["g"].device)

        def seg(kind):
            lib.check(L.odvae_grad_seg_norms_f32(f["g"].data_ptr(), total, offs, lens, None, n_par, kind, 0.0, norms.data_ptr(), sp, sn, stream), "grad_seg_norms")
        r = _alternate({"pair": pair, "seg": lambda: seg(2), "seg_inf": lambda: seg(0), "method": lambda: opt.grad_norms(2)}, args.iters, args.rounds)
        med = {k: statistics.median(v[1]) for k, v in r.items()}
        K = int(L.odvae_grad_seg_norms_segments_per_launch())
        norm_rows.append("| optimizer %d | %d | %d | %d | %s | %s | %s | %.2f | %.2f |"
                         % (idx, n_par, total, -(-n_par // K) + 2, _fmt(r["pair"][1], 1e3, 1), _fmt(r["seg"][1], 1e3, 1), _fmt(r["seg_inf"][1], 1e3, 1),
                            med["seg"] / med["pair"], 4.0 * total / med["seg"] / 1e9))
        host_rows.append("| optimizer %d | %d | %s | %s | %s |" % (idx, n_par, _fmt(r["pair"][0], 1e3, 1), _fmt(r["seg"][0], 1e3, 1), _fmt(r["method"][0], 1e3, 1)))
        # Adam: copies of the arenas, lr as configured; the plain entry point's own run-to-run spread first
        p, m, v = f["p"].clone(), torch.zeros_like(f["p"]), torch.zeros_like(f["p"])

        def plain():
            lib.check(L.odvae_adam_step_f32(p.data_ptr(), f["g"].data_ptr(), m.data_ptr(), v.data_ptr(), total, 1e-5, 0.5, 0.9, 1e-8, 1, None, stream), "adam")

        def clamp():
            lib.check(L.odvae_adam_step_clamp_f32(p.data_ptr(), f["g"].data_ptr(), m.data_ptr(), v.data_ptr(), total, 1e-5, 0.5, 0.9, 1e-8, 1,
                                                  ctypes.c_float(1e-3), stream), "adam_clamp")
        first = _alternate({"plain": plain}, args.iters, args.rounds)["plain"][1]
        r = _alternate({"plain": plain, "clamp": clamp}, args.iters, args.rounds)
        ratio = statistics.median(r["clamp"][1]) / statistics.median(r["plain"][1])
        bound = 1.0 + _spread(first) + 0.03
        adam_rows.append("| optimizer %d | %d | %.1f %% | %s | %s | %.3f | %.3f | %s |"
                         % (idx, total, 100 * _spread(first), _fmt(r["plain"][1], 1e3, 1), _fmt(r["clamp"][1], 1e3, 1), ratio, bound,
                            "yes" if ratio <= bound else "NO"))
        del p, m, v
        opt._touched.clear()
    out += ["## Segmented norms against the global-norm launch pair, same arena", "",
            "%d calls queued per round, %d rounds, alternated; device us per call, median (min .. max).  Expectation: ratio <= 1.5." % (args.iters, args.rounds), "",
            "| arena | segments | floats | launches | odvae_grad_norm_f32 us | odvae_grad_seg_norms_f32 L2 us | max us | L2 / pair | seg L2 read TB/s |",
            "|---|---|---|---|---|---|---|---|---|"] + norm_rows
    out += ["", "Host time to enqueue one call (us, median (min .. max)):", "", "| arena | segments | odvae_grad_norm_f32 | odvae_grad_seg_norms_f32 | FusedAdam.grad_norms(2) |", "|---|---|---|---|---|"] + host_rows
    out += ["", "## Adam with the clamp against the plain step, copies of the same arenas", "",
            "Expectation: clamp / plain <= 1 + the plain entry point's own spread ((max - min) / median over %d rounds by itself, measured first) + 3 %%." % args.rounds, "",
            "| arena | floats | plain spread | odvae_adam_step_f32 us | odvae_adam_step_clamp_f32 us | clamp / plain | bound | within |", "|---|---|---|---|---|---|---|---|"] + adam_rows
    return out


def log_section(args, trainer):
    import torch
    out = ["", "## Host time to enqueue one tracked step's log", "",
           "`Trainer._track_grad_norms`: FusedAdam.grad_norms, the 0-d views, the key dict, model.log_dict.  ms per call, median (min .. max) over %d rounds of %d calls." % (args.rounds, args.iters), "",
           "| optimizer | keys | host ms | device ms |", "|---|---|---|---|"]
    trainer.track_grad_norm = 2.0
    for idx, opt in enumerate(trainer.optimizers):
        n_par = len(opt.materialize()["params"])

        def track():
            opt._touched.update(range(n_par))
            trainer._track_grad_norms(idx, opt)
        r = _alternate({"t": track}, args.iters, args.rounds)["t"]
        out.append("| %d | %d | %s | %s |" % (idx, len(trainer.grad_norms[idx][0]) + 1, _fmt(r[0]), _fmt(r[1])))
        opt._touched.clear()
    trainer.track_grad_norm = None
    torch.cuda.synchronize()
    return out


def step_section(args, model, trainer):
    import torch
    from odvae_amd import synthetic
    batch = synthetic.make_batch(args.batch, args.res, seed=23)
    batch = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in batch.items()}
    variants = {"tracking off, norm clip (the parent's step)": (None, None), "track_grad_norm=2": (2.0, None), "gradient_clip_algorithm=value": (None, "value")}
    times = {k: [] for k in variants}
    count = [0]

    def run(n):
        for _ in range(n):
            mb = dict(batch)
            mb["pose_6d"] = batch["pose_6d"].clone()
            trainer.training_batch(mb, count[0])
            count[0] += 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(args.rounds):
            for name, (track, algo) in variants.items():
                trainer.track_grad_norm, trainer.gradient_clip_algorithm = track, algo
                run(args.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    trainer.track_grad_norm, trainer.gradient_clip_algorithm = None, None
    base = statistics.median(times["tracking off, norm clip (the parent's step)"])
    out = ["", "## Whole optimizer steps, rec+KL f32, B = %d at %d x %d, optimizer 0, gradient_clip_val 1.0" % (args.batch, args.res, args.res), "",
           "%d timed steps after %d warm-up step(s) per round, %d rounds, the three variants alternated on one model; wall ms per step with a device wait at both ends." % (args.steps, args.warmup, args.rounds), "",
           "| variant | ms / step, median (min .. max) | spread | against off |", "|---|---|---|---|"]
    for name, xs in times.items():
        out.append("| %s | %s | %.2f %% | %+.2f %% |" % (name, _fmt(xs, 1e3, 1), 100 * _spread(xs), 100 * (statistics.median(xs) / base - 1)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-steps", action="store_true", help="kernels and host times only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_norms.md"))
    args = ap.parse_args()
    import torch
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=args.res // 16).to("cuda:0").train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
    lines = kernel_sections(args, trainer) + log_section(args, trainer)
    if not args.no_steps:
        lines += step_section(args, model, trainer)
    body = "\n".join(lines) + "\n"
    print(body, flush=True)
    if args.out:
        write_section(args.out, body)


BEGIN, END = "<!-- tools/grad_norms_time.py: begin -->", "<!-- tools/grad_norms_time.py: end -->"


def write_section(path, body):
    """Replace the tool's own section of `path` (between the two markers; appended when absent): the file also holds the notes around the figures."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    text = open(path).read() if os.path.exists(path) else "# track_grad_norm and gradient_clip_algorithm: measurements\n"
    block = "%s\n%s%s\n" % (BEGIN, body, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):].lstrip("\n")
    else:
        text = text.rstrip("\n") + "\n\n" + block
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
