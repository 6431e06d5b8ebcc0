"""Cost of gradient accumulation (Trainer(accumulate_grad_batches=N)) on the benchmark network.

1. The accumulate pass alone, on the headline optimizer-0 parameter list: `FusedAdam.gather_grads(accumulate=True)` (one multi-tensor
   odvae_grad_accumulate_f32 launch per K parameters) against what autograd does when `.grad` stays pointed at the arena over the window -- one in-place
   `add_` per parameter -- and against torch's own multi-tensor `_foreach_add_`.  Each variant is queued `--iters` times between ONE pair of events
   (no synchronisation per iteration); the host time to enqueue the queue is taken separately.  Bytes: 3 x arena (read sum, read gradient, write sum).
2. Whole optimizer steps at the same images per step: (B, N) = (32, 1), (16, 2), (8, 4): ms per optimizer step, peak `max_memory_allocated`,
   accumulate launches per later micro-batch.

    python tools/accum_time.py [--res 256] [--iters 100] [--steps 3] [--warmup 1] [--configs 32x1,16x2,8x4] [--out profiles/grad_accum.md]

Only the tool's own section of the output file (between its two markers) is rewritten.
"""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def _build(res, n_acc, bf16=False):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=res // 16).to("cuda:0").train()
    model._global_step = 1
    return model, Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision="bf16" if bf16 else None, accumulate_grad_batches=n_acc)


def _queue(fn, iters):
    """fn() queued `iters` times between one event pair: (host ms per call to enqueue, device ms per call)."""
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


def kernel_section(args):
    import torch
    model, trainer = _build(args.res, 2)
    opt = trainer.optimizers[0]
    f = opt.materialize()
    params, views = f["params"], f["gviews"]
    fresh = [torch.randn_like(v) * 1e-3 for v in views]
    numel = sum(v.numel() for v in views)
    nbytes = 3 * 4 * numel

    def one_launch():
        for p, g in zip(params, fresh):
            p.grad = g
        opt.gather_grads(accumulate=True)

    def per_parameter():                 # autograd's AccumulateGrad when .grad is the arena view: one in-place add per parameter
        with torch.no_grad():
            for v, g in zip(views, fresh):
                v.add_(g)

    def foreach():
        with torch.no_grad():
            torch._foreach_add_(views, fresh)
    calls = opt.accumulate_calls
    rows = []
    for name, fn in (("odvae_grad_accumulate_f32 via gather_grads(accumulate=True)", one_launch), ("one torch add_ per parameter", per_parameter),
                     ("torch._foreach_add_", foreach)):
        host, dev = _queue(fn, args.iters)
        rows.append((name, host, dev, nbytes / dev / 1e9))
    launches = (opt.accumulate_calls - calls) // (args.iters + 1)
    out = ["## The accumulate pass on the headline optimizer-0 parameter list", "",
           "%d parameters, %.1f M floats; %.0f MB moved per pass (3 x %.0f MB algorithmic); %d launch(es) per pass; %d passes queued between one event pair."
           % (len(params), numel / 1e6, nbytes / 1e6, 4 * numel / 1e6, launches, args.iters), "",
           "| variant | host enqueue ms / pass | device ms / pass | implied HBM TB/s |", "|---|---|---|---|"]
    out += ["| %s | %.3f | %.3f | %.2f |" % r for r in rows]
    del model, trainer
    return out


def step_section(args):
    import torch
    from odvae_amd import synthetic
    out = ["", "## Whole optimizer steps, rec+KL f32 at %d x %d" % (args.res, args.res), "",
           "| B per micro-batch | N | ms / optimizer step | images / s | peak max_memory_allocated GB | accumulate launches / later micro-batch |", "|---|---|---|---|---|---|"]
    for cfg in args.configs.split(","):
        b, n = (int(x) for x in cfg.split("x"))
        torch.cuda.empty_cache()
        model, trainer = _build(args.res, n)
        opt = trainer.optimizers[0]
        batch = synthetic.make_batch(b, args.res, seed=23)
        batch = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in batch.items()}

        def step(i):
            for m in range(n):
                mb = dict(batch)
                mb["pose_6d"] = batch["pose_6d"].clone()
                trainer.training_batch(mb, i * n + m)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            calls = opt.accumulate_calls
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(args.warmup + i)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
        later = args.steps * (n - 1)
        out.append("| %d | %d | %.1f | %.1f | %.1f | %s |" % (b, n, dt * 1e3, b * n / dt, torch.cuda.max_memory_allocated() / 1e9,
                                                              "%.1f" % ((opt.accumulate_calls - calls) / later) if later else "-"))
        del model, trainer, opt
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="32x1,16x2,8x4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum.md"))
    args = ap.parse_args()
    body = "\n".join(kernel_section(args) + step_section(args)) + "\n"
    print(body, flush=True)
    if args.out:
        write_section(args.out, body)


BEGIN, END = "<!-- tools/accum_time.py: begin -->", "<!-- tools/accum_time.py: end -->"


def write_section(path, body):
    """Replace the tool's own section of `path` (between the two markers; appended when absent): the file also holds figures from the tests."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    text = open(path).read() if os.path.exists(path) else "# Gradient accumulation: measurements\n"
    block = "%s\n%s%s\n" % (BEGIN, body, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):].lstrip("\n")
    else:
        text = text.rstrip("\n") + "\n\n" + block
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
