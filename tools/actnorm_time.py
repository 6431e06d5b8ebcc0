"""ActNorm + LeakyReLU (ops.actnorm_lrelu, the an_* kernels of gan_norm.hip) beside training-mode BatchNorm + LeakyReLU (ops.batchnorm_lrelu)
at the PatchGAN's three normalised layers for 256 x 256 inputs, B = 32, and one generator-plus-discriminator batch of BASELINE configs[3]
(PatchGAN + LPIPS-style loss, both optimizers) with `use_actnorm` on and off -- all in one process.
Bytes alone say ActNorm moves 2 tensor passes forward and 3 backward against BatchNorm's 3 and 5, so at every shape its time should not
exceed the BatchNorm kernels' time measured in the same run.
Timing: one HIP event pair around `reps` calls queued back to back, one synchronise per window; windows of the variants alternate,
the median over the rounds is reported.
usage: python tools/actnorm_time.py [--reps R] [--rounds K] [--no-step] [--steps K] [--warmup W] [--batch B] [--res RES] [--json PATH]"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY = 6.29e12      # bytes/s: what a float4 copy reaches on this chip
SHAPES = [(32, 128, 64, 64), (32, 256, 32, 32), (32, 512, 31, 31)]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_times(shape, reps, rounds):
    from odvae_amd import ops
    from odvae_amd.gan import ActNormLReLU, BatchNormLReLU
    dev = torch.device("cuda:0")
    n, c, h, w = shape
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(n, c, h, w, device=dev, generator=g) * 0.7 + 0.3).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn(n, c, h, w, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    an = ActNormLReLU(c).to(dev).train()
    an(x.detach())                                   # initialises: the timed calls are the steady state
    an_frozen = ActNormLReLU(c).to(dev).train()
    an_frozen.load_state_dict(an.state_dict())
    for p in an_frozen.parameters():
        p.requires_grad_(False)
    bn = BatchNormLReLU(c).to(dev).train()

    def run(fn, backward):
        def call():
            y = fn(x)
            if backward:
                y.backward(dy)
                x.grad = None
        return call

    # the kernels alone, through the C ABI on preallocated buffers: no autograd node, no allocation, ~5 us of host work per call, so the
    # queue stays full and the window holds device time (the op-level variants carry the autograd engine's host time per call, which
    # at these sizes is of the order of the kernels' own time)
    from odvae_amd import lib
    L, st = lib.load(), lib.stream_ptr()
    rows = n * h * w
    xd, y, dx = x.detach(), torch.empty_like(dy), torch.empty_like(dy)
    loc, scale = an.loc.detach(), an.scale.detach()
    dloc, dscale = torch.empty_like(loc), torch.empty_like(scale)
    gamma, beta, mean, rstd = bn.weight.detach(), bn.bias.detach(), torch.empty(c, device=dev), torch.empty(c, device=dev)
    dgamma, dbeta = torch.empty(c, device=dev), torch.empty(c, device=dev)
    wp, wn = lib.workspace.get(max(L.odvae_actnorm_workspace_bytes(rows, c), L.odvae_batchnorm_workspace_bytes(rows, c)), dev)

    def k_an_fwd():
        lib.check(L.odvae_actnorm_lrelu_fwd_f32(xd.data_ptr(), rows, c, loc.data_ptr(), scale.data_ptr(), 0.2, y.data_ptr(), st), "an fwd")

    def k_an_bwd():
        lib.check(L.odvae_actnorm_lrelu_bwd_f32(xd.data_ptr(), dy.data_ptr(), rows, c, loc.data_ptr(), scale.data_ptr(), 0.2, dx.data_ptr(),
                                                dloc.data_ptr(), dscale.data_ptr(), wp, wn, st), "an bwd")

    def k_an_bwd_dx():
        lib.check(L.odvae_actnorm_lrelu_bwd_f32(xd.data_ptr(), dy.data_ptr(), rows, c, loc.data_ptr(), scale.data_ptr(), 0.2, dx.data_ptr(),
                                                None, None, None, 0, st), "an bwd dx")

    def k_bn_fwd():
        lib.check(L.odvae_batchnorm_lrelu_fwd_f32(xd.data_ptr(), rows, c, gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, 0.2, 1, mean.data_ptr(),
                                                  rstd.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), y.data_ptr(), wp, wn, st), "bn fwd")

    def k_bn_bwd():
        lib.check(L.odvae_batchnorm_lrelu_bwd_f32(xd.data_ptr(), dy.data_ptr(), rows, c, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                                  rstd.data_ptr(), 0.2, 1, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), wp, wn, st), "bn bwd")

    def both(a_, b_):
        def call():
            a_(); b_()
        return call

    variants = {"kernels: actnorm fwd": k_an_fwd, "kernels: batchnorm fwd": k_bn_fwd,
                "kernels: actnorm bwd": k_an_bwd, "kernels: batchnorm bwd": k_bn_bwd,
                "kernels: actnorm bwd (dx only)": k_an_bwd_dx,
                "kernels: actnorm fwd+bwd": both(k_an_fwd, k_an_bwd), "kernels: batchnorm fwd+bwd": both(k_bn_fwd, k_bn_bwd),
                "actnorm fwd": run(an, False), "batchnorm fwd": run(bn, False),
                "actnorm fwd+bwd": run(an, True), "batchnorm fwd+bwd": run(bn, True),
                "actnorm fwd+bwd (dx only)": run(an_frozen, True),
                "actnorm init": lambda: ops.actnorm_init(x, an.loc, an.scale, an.EPS)}
    times = {k: [] for k in variants}
    for fn in variants.values():      # warm-up: code objects, workspace growth, the allocator's blocks
        window(fn, 2)
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps))
    ms = {k: statistics.median(v) for k, v in times.items()}
    tensor_bytes = 4.0 * n * c * h * w
    res = {"shape": list(shape), "ms": ms, "ms_min": {k: min(v) for k, v in times.items()},
           "tensor_mbytes": tensor_bytes / 1e6,
           # 2 passes forward + 3 backward for ActNorm, 3 + 5 for BatchNorm, against the float4 copy rate
           "actnorm_fwd_bwd_fraction_of_copy_rate": 5 * tensor_bytes / (ms["kernels: actnorm fwd+bwd"] * 1e-3) / HBM_COPY,
           "batchnorm_fwd_bwd_fraction_of_copy_rate": 8 * tensor_bytes / (ms["kernels: batchnorm fwd+bwd"] * 1e-3) / HBM_COPY,
           "kernels_actnorm_over_batchnorm_fwd_bwd": ms["kernels: actnorm fwd+bwd"] / ms["kernels: batchnorm fwd+bwd"],
           "actnorm_over_batchnorm_fwd_bwd": ms["actnorm fwd+bwd"] / ms["batchnorm fwd+bwd"],
           "actnorm_over_batchnorm_fwd": ms["actnorm fwd"] / ms["batchnorm fwd"]}
    print("shape %s (%.1f MB per tensor)" % ("x".join(map(str, shape)), tensor_bytes / 1e6))
    for k in variants:
        print("  %-32s median %8.4f ms   min %8.4f ms" % (k, ms[k], res["ms_min"][k]), flush=True)
    return res


def step_times(res_px, batch, steps, warmup):
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    yaml = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
    dev = torch.device("cuda:0")
    out = {"res": res_px, "batch": batch, "steps": steps, "warmup": warmup}
    for name in ("batchnorm", "actnorm", "batchnorm", "actnorm"):
        torch.manual_seed(23)
        mcfg, _ = synthetic.model_config(yaml, latent_hw=res_px // 16, perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
        mcfg.params.lossconfig.params["use_actnorm"] = name == "actnorm"
        model = instantiate_from_config(mcfg)
        model.learning_rate = 12 * 4.5e-6
        model = model.to(dev).train()
        model._global_step = 1
        trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
        data = synthetic.make_batch(batch, res_px, seed=23)
        data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}

        def step(i):
            b = dict(data)
            b["pose_6d"] = data["pose_6d"].clone()
            return trainer.training_batch(b, i)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i in range(warmup):
                step(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                loss = step(warmup + i)
            e1.record()
            e1.synchronize()
        ms = e0.elapsed_time(e1) / steps
        rec = {"ms_per_batch": ms, "images_per_s": batch / ms * 1e3, "last_aeloss": float(loss[0]), "last_discloss": float(loss[1])}
        out.setdefault(name, []).append(rec)
        print(name, json.dumps(rec), flush=True)
        del model, trainer, data, loss
        gc.collect()
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"reps": a.reps, "rounds": a.rounds, "layers": [layer_times(s, a.reps, a.rounds) for s in SHAPES]}
    if not a.no_step:
        res["step"] = step_times(a.res, a.batch, a.steps, a.warmup)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
