"""Cost of the latent stage with the noise drawn on the host (the default) and on the device (model.params.device_noise).

1. The latent stage alone, forward + backward, at B = 12 and 32 with the 16 x 16 x 16 latent and at B = 12 with 32 x 32 x 16:
     chain, host draws   torch.randn / torch.rand / torch.randn on the host, three uploads through the pinned ring, gaussian_sample and
                         three latent_combine launches, their autograd backward (what PoseAutoencoder.forward does with the option off);
     chain, no draws     the same launches with the three tensors already on the device (the kernels' share of the line above);
     fused               ops.latent_stage: one launch forward, one backward, draws made in registers.
   Each variant is queued `--iters` times between one pair of events; the host time to enqueue is taken separately.
2. Whole training steps (optimizer 0, rec+KL, the benchmark network) with device_noise off and on, ALTERNATED: `--rounds` rounds of
   off then on, `--steps` steps each after `--warmup`; every figure of both series is written down, with each series' spread.

    python tools/latent_time.py [--iters 200] [--batch 12] [--res 256] [--precision 32|bf16] [--rounds 5] [--steps 5] [--out profiles/device_noise.md]

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
DEV = "cuda:0"


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


def stage_section(args):
    import torch
    from odvae_amd import latent_noise as ln
    from odvae_amd import lib, ops
    out = ["## The latent stage alone, forward + backward (p = 0.7, noise on, enc_pose added)", "",
           "%d calls queued between one event pair per row." % args.iters, "",
           "| latent B x H x W x Cz | variant | host enqueue ms / call | device ms / call | launches / call |", "|---|---|---|---|---|"]
    p = 0.7
    for b, hw in ((12, 16), (32, 16), (12, 32)):
        g = torch.Generator().manual_seed(3)
        shape = (b, 16, hw, hw)
        mom = torch.randn(b, 32, hw, hw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        add = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        dz = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        draw = ln.make_draw(1234, 0, 7, True, 0)
        on_dev = [ops.noise_fill(shape, ln.with_stream(draw, s), DEV, kind=k, p=p, nhwc=True) for s, k in ((0, 0), (1, 1), (2, 0))]

        def chain(eps, mask, noise):
            z = ops.gaussian_sample(mom, eps)
            z = ops.latent_combine(z, mask, None)
            z = ops.latent_combine(z, None, noise)
            z = ops.latent_combine(z, None, add)
            z.backward(dz)
            mom.grad = add.grad = None

        def chain_host():
            eps = torch.randn(shape)
            mask = (torch.rand(shape) >= p).float() / (1.0 - p)
            noise = torch.randn(shape)
            chain(lib.upload(eps, DEV), lib.upload(mask, DEV), lib.upload(noise, DEV))

        def chain_dev():
            chain(*on_dev)

        def fused():
            z = ops.latent_stage(mom, draw, add=add, dropout_p=p, noise=True)
            z.backward(dz)
            mom.grad = add.grad = None

        for name, fn, launches in (("chain, host draws", chain_host, "3 copies + 6"), ("chain, no draws", chain_dev, "6"), ("fused", fused, "2")):
            host, dev = _queue(fn, args.iters)
            out.append("| %d x %d x %d x 16 | %s | %.3f | %.3f | %s |" % (b, hw, hw, name, host, dev, launches))
    return out


def _build(args, device_noise):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    mcfg, cfg = synthetic.model_config(YAML, latent_hw=args.res // 16)
    if device_noise is not None:
        mcfg.params["device_noise"] = device_noise
    model = instantiate_from_config(mcfg)
    model.learning_rate = args.batch * cfg.model.base_learning_rate
    model = model.to(DEV).train()
    model._global_step = 1
    return model, Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision=None if args.precision == "32" else args.precision)


def step_section(args):
    import torch
    from odvae_amd import synthetic
    runs = {"off": _build(args, None), "on": _build(args, 1234)}
    batch = synthetic.make_batch(args.batch, args.res, seed=23)      # a host batch, as a loader hands it over
    series = {"off": [], "on": []}

    def steps(trainer, first, count):
        for i in range(count):
            mb = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
            trainer.training_batch(mb, first + i)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("off", "on"):
            steps(runs[name][1], 0, args.warmup)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name in ("off", "on"):
                t0 = time.perf_counter()
                steps(runs[name][1], args.warmup + r * args.steps, args.steps)
                torch.cuda.synchronize()
                series[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = ["", "## Whole training steps, device_noise off and on alternated", "",
           "Optimizer 0, rec+KL, precision %s, B = %d at %d x %d; %d rounds of off then on, %d steps each after %d warm-up steps; ms per step, host clock around synchronised rounds."
           % (args.precision, args.batch, args.res, args.res, args.rounds, args.steps, args.warmup), "",
           "| series | " + " | ".join("round %d" % (r + 1) for r in range(args.rounds)) + " | median | min | max | spread (max - min) |",
           "|---|" + "---|" * (args.rounds + 4)]
    for name in ("off", "on"):
        s = series[name]
        out.append("| %s | " % name + " | ".join("%.2f" % v for v in s) + " | %.2f | %.2f | %.2f | %.2f |" % (statistics.median(s), min(s), max(s), max(s) - min(s)))
    diff = statistics.median(series["on"]) - statistics.median(series["off"])
    spread = max(series["off"]) - min(series["off"])
    out += ["", "on - off, medians: %+.2f ms; the off series' own spread: %.2f ms -> %s." % (diff, spread, "within it" if diff <= spread else "NOT within it")]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--precision", default="32", choices=["32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true", help="the latent stage alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_noise.md"))
    args = ap.parse_args()
    body = "\n".join(stage_section(args) + ([] if args.skip_steps else step_section(args))) + "\n"
    print(body, flush=True)
    if args.out:
        write_section(args.out, body, args.precision)


def write_section(path, body, precision):
    """Replace the tool's own section of `path` for this precision (between its two markers; appended when absent)."""
    begin, end = "<!-- tools/latent_time.py %s: begin -->" % precision, "<!-- tools/latent_time.py %s: end -->" % precision
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    text = open(path).read() if os.path.exists(path) else "# Device-side latent noise: measurements\n"
    block = "%s\n%s%s\n" % (begin, body, end)
    if begin in text and end in text:
        text = text[:text.index(begin)] + block + text[text.index(end) + len(end):].lstrip("\n")
    else:
        text = text.rstrip("\n") + "\n\n" + block
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
