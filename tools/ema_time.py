"""Cost of the weight average (model.params.ema_decay) on the benchmark network.

1. The EMA kernels alone at the headline arena sizes (optimizer 0's 71 M floats, the discriminator's arena): odvae_ema_update_f32 (12 bytes per
   element: read parameter, read and write shadow), odvae_ema_swap_f32 (16 bytes per element) and, as the yardstick, torch's device copy of the same
   arena (8 bytes per element).  Each is queued `--iters` times between ONE pair of events (no synchronisation per iteration); achieved TB/s =
   algorithmic bytes / device time.  Then one whole `model.model_ema(model)` (tick + a launch per arena + one for loss.logvar) and one
   `ema_scope` enter + exit: device time and host time to enqueue.
2. Whole training batches with `ema_decay` unset and set, in one process, alternating, `--repeats` times each: ms per batch (host clock around
   `--steps` batches ending in a device synchronise, after `--warmup` batches).

    python tools/ema_time.py [--res 256] [--batch 32] [--iters 50] [--steps 5] [--warmup 2] [--repeats 3] [--both-optimizers] [--out profiles/ema.md]

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


def _build(res, ema_decay, both):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    kw = dict(perceptual_weight=1.0, disc_factor=1.0) if both else {}
    model_cfg, cfg = synthetic.model_config(YAML, latent_hw=res // 16, **kw)
    if ema_decay is not None:
        model_cfg.params["ema_decay"] = ema_decay
    model = instantiate_from_config(model_cfg)
    model.learning_rate = 12 * cfg.model.base_learning_rate
    model = model.to("cuda:0").train()
    model._global_step = 1
    return model, Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1) if both else (0,))


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
    from odvae_amd import ops
    model, trainer = _build(args.res, 0.9999, args.both_optimizers)
    ema = model.model_ema
    state = torch.tensor([1e-4, 0.9999], device="cuda:0")
    out = ["## The EMA kernels alone at the headline arena sizes", "",
           "%d launches queued between one event pair per row; TB/s = algorithmic bytes / device time." % args.iters, "",
           "| arena | floats | kernel | bytes / element | device ms | achieved TB/s |", "|---|---|---|---|---|---|"]
    for name, (p, s, n) in zip(("optimizer 0 (autoencoder)", "optimizer 1 (discriminator)"), ema.arenas):
        scratch = s.clone()
        for label, per, fn in (("odvae_ema_update_f32", 12, lambda: ops.ema_update(p, s, state, n)),
                               ("odvae_ema_swap_f32", 16, lambda: ops.ema_swap(scratch, s, n)),
                               ("torch copy_ (yardstick)", 8, lambda: scratch.copy_(s))):
            _, dev = _queue(fn, args.iters)
            out.append("| %s | %d | %s | %d | %.4f | %.2f |" % (name, n, label, per, dev, per * n / dev / 1e9))
        del scratch
    host, dev = _queue(lambda: ema(model), args.iters)
    out += ["", "One whole update, `model.model_ema(model)` (one tick, %d arena launches, %d stray parameters): %.4f ms on the device, %.3f ms of host time to enqueue."
            % (len(ema.arenas), len(ema._launches(model)) - len(ema.arenas), dev, host)]

    def scope():
        with model.ema_scope():
            pass
    host, dev = _queue(scope, args.iters)
    out += ["`ema_scope` enter + exit with an empty body (two exchanges of every arena): %.4f ms on the device, %.3f ms of host time." % (dev, host)]
    del model, trainer
    return out


def step_section(args):
    import torch
    from odvae_amd import synthetic
    what = "both optimizers (LPIPS-style net and discriminator on)" if args.both_optimizers else "rec+KL, optimizer 0 only"
    out = ["", "## Whole training batches, f32 at %d x %d, B = %d, %s" % (args.res, args.res, args.batch, what), "",
           "%d timed batches after %d warm-up batches per row; the two settings alternate in one process, the order reversed every repeat "
           "(unset, set, set, unset, ...)." % (args.steps, args.warmup), "",
           "| repeat | ema_decay | ms / batch | images / s |", "|---|---|---|---|"]
    batch = synthetic.make_batch(args.batch, args.res, seed=23)
    batch = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in batch.items()}
    times = {None: [], 0.9999: []}
    for rep in range(args.repeats):
        for decay in ((None, 0.9999) if rep % 2 == 0 else (0.9999, None)):      # unset, set, set, unset, ...: a drift of the clocks over the run cancels
            torch.cuda.empty_cache()
            model, trainer = _build(args.res, decay, args.both_optimizers)

            def step(i):
                mb = dict(batch)
                mb["pose_6d"] = batch["pose_6d"].clone()
                trainer.training_batch(mb, i)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for i in range(args.warmup):
                    step(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    step(args.warmup + i)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.steps
            if decay is not None:
                assert int(model.model_ema.num_updates) == args.warmup + args.steps
            times[decay].append(dt * 1e3)
            out.append("| %d | %s | %.2f | %.1f |" % (rep, "unset" if decay is None else "%g" % decay, dt * 1e3, args.batch / dt))
            del model, trainer
    mean = {k: sum(v) / len(v) for k, v in times.items()}
    out += ["", "Mean over %d repeats: unset %.2f ms (min %.2f, max %.2f), set %.2f ms (min %.2f, max %.2f); difference of the means %+.2f ms."
            % (args.repeats, mean[None], min(times[None]), max(times[None]), mean[0.9999], min(times[0.9999]), max(times[0.9999]), mean[0.9999] - mean[None])]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--both-optimizers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_time.py needs an MI355X: nothing here can be measured on the host")
    body = "\n".join(["Command: `python tools/ema_time.py %s`" % " ".join(sys.argv[1:]), ""] + kernel_section(args) + step_section(args)) + "\n"
    print(body, flush=True)
    if args.out:
        write_section(args.out, body)


BEGIN, END = "<!-- tools/ema_time.py: begin -->", "<!-- tools/ema_time.py: end -->"


def write_section(path, body):
    """Replace the tool's own section of `path` (between the two markers; appended when absent)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    text = open(path).read() if os.path.exists(path) else "# Weight average (ema_decay): measurements\n"
    block = "%s\n%s%s\n" % (BEGIN, body, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):].lstrip("\n")
    else:
        text = text.rstrip("\n") + "\n\n" + block
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
