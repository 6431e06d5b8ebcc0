"""The vector quantiser (ops.vq_quantize, vq_f32.hip) against a torch-on-device restatement of upstream's materialised-distance form
(permute, d[M, K] in f32, argmin, embedding lookup, detach arithmetic, permute; autograd's index_add for the codebook gradient) at the
vq-f4 / vq-f8 / vq-f16 and VQGAN shapes of a 256 x 256, B = 32 batch, forward and forward + backward, with the peak device memory of each;
and a whole VQModel training batch.  Nothing here gates anything: the figures go to profiles/vq.md as measured.
Timing: one HIP event pair around `reps` calls queued back to back, one synchronise per window; windows of the two variants alternate, the
median over the rounds is reported.
usage: python tools/vq_time.py [--shapes f4 f8 f16 vqgan] [--batch B] [--reps R] [--rounds K] [--no-torch] [--json PATH]
       python tools/vq_time.py --step RES BATCH [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (latent side at 256 x 256, n_embed, embed_dim)
SHAPES = {"f4": (64, 8192, 3), "f8": (32, 16384, 4), "f16": (16, 16384, 8), "vqgan": (16, 1024, 256)}


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_quantize(z, weight, beta, legacy=True):
    """VectorQuantizer2.forward on device tensors"""
    zp = z.permute(0, 2, 3, 1).contiguous()
    flat = zp.view(-1, weight.shape[1])
    d = torch.sum(flat ** 2, dim=1, keepdim=True) + torch.sum(weight ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", flat, weight.t())
    idx = torch.argmin(d, dim=1)
    z_q = torch.nn.functional.embedding(idx, weight).view(zp.shape)
    if legacy:
        loss = torch.mean((z_q.detach() - zp) ** 2) + beta * torch.mean((z_q - zp.detach()) ** 2)
    else:
        loss = beta * torch.mean((z_q.detach() - zp) ** 2) + torch.mean((z_q - zp.detach()) ** 2)
    z_q = zp + (z_q - zp).detach()
    return z_q.permute(0, 3, 1, 2).contiguous(), loss, idx


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20


def op_mode(a):
    from odvae_amd import ops
    dev = torch.device("cuda:0")
    out = {"batch": a.batch, "reps": a.reps, "rounds": a.rounds, "shapes": {}}
    for name in a.shapes:
        side, k, d = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(0)
        z = torch.randn(a.batch, d, side, side, device=dev, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        e = torch.randn(k, d, device=dev, generator=g).requires_grad_(True)
        go = torch.randn(a.batch, d, side, side, device=dev, generator=g).contiguous(memory_format=torch.channels_last)

        def run(fn, backward):
            def call():
                if not backward:
                    with torch.no_grad():
                        fn(z, e, 0.25)
                    return
                zq, loss, _ = fn(z, e, 0.25)
                torch.autograd.backward([zq, loss], [go, torch.ones_like(loss)])
                z.grad = None
                e.grad = None
            return call
        variants = {"hip fwd": run(ops.vq_quantize, False), "hip fwd+bwd": run(ops.vq_quantize, True)}
        if not a.no_torch:
            variants["torch fwd"] = run(torch_quantize, False)
            variants["torch fwd+bwd"] = run(torch_quantize, True)
        for fn in variants.values():
            window(fn, 1)
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v, fn in variants.items():
                times[v].append(window(fn, a.reps))
        rec = {"M": a.batch * side * side, "K": k, "D": d, "plan": ops.vq_plan(a.batch * side * side, k, d),
               "ms": {v: statistics.median(t) for v, t in times.items()}, "ms_min": {v: min(t) for v, t in times.items()},
               "peak_mb": {v: peak_of(fn, dev) for v, fn in variants.items()}}
        rec["search_tflops"] = 2.0 * rec["M"] * k * d / (rec["ms"]["hip fwd"] * 1e-3) / 1e12
        if not a.no_torch:
            rec["torch_over_hip_fwd_bwd"] = rec["ms"]["torch fwd+bwd"] / rec["ms"]["hip fwd+bwd"]
            with torch.no_grad():
                same = (ops.vq_quantize(z, e, 0.25)[2] == torch_quantize(z, e, 0.25)[2]).float().mean().item()
            rec["share_of_indices_equal_to_torch"] = same
        out["shapes"][name] = rec
        for v in variants:
            print("%-6s %-14s median %9.3f ms   min %9.3f ms   peak %9.1f MB" % (name, v, rec["ms"][v], rec["ms_min"][v], rec["peak_mb"][v]), flush=True)
        del z, e, go, variants
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def step_mode(a):
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    from odvae_amd.trainer import Trainer
    res_px, batch = a.step
    dev = torch.device("cuda:0")
    # the published vq-f4 geometry (ldm configs/autoencoder vq-f4: ch 128, ch_mult [1, 2, 4], 8192 codes of dimension 3)
    config = Config.merge(Config.load(os.path.join(ROOT, "tests", "golden", "autoencoder_vq_plain.yaml")), Config.from_dotlist(
        ["model.params.n_embed=8192", "model.params.lossconfig.params.n_classes=8192", "model.params.ddconfig.ch=128",
         "model.params.ddconfig.resolution=%d" % res_px]))
    torch.manual_seed(23)
    model = instantiate_from_config(config.model)
    model.learning_rate = batch * 4.5e-6
    model = model.to(dev).train()
    trainer = Trainer(model, gradient_clip_val=1.0)
    data = synthetic.make_image_batch(batch, res_px, seed=23)
    for i in range(a.warmup):
        trainer.training_batch(dict(data), i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.steps):
        losses = trainer.training_batch(dict(data), a.warmup + i)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    out = {"res": res_px, "batch": batch, "steps": a.steps, "warmup": a.warmup, "ms_per_batch": ms, "images_per_s": batch / ms * 1e3,
           "peak_device_memory_gb": torch.cuda.max_memory_allocated(dev) / 1e9, "last_losses": [float(l) for l in losses],
           "perplexity": float(model.logged_metrics.get("train/perplexity", float("nan")))}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2, metavar=("RES", "BATCH"), default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = step_mode(a) if a.step else op_mode(a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
