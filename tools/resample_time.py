"""The conv-less resamplers (ddconfig.resamp_with_conv = False: odvae_avgpool2x2_* / odvae_upsample2x_*) and the decoder's tanh at the
layer shapes of the headline network (B = 32, 256 x 256, ch = 128, ch_mult 1,1,2,2,4), f32 and bf16, all in one process:
  * every new kernel alone, with the bytes/s it reaches beside the GroupNorm apply stream's at the shape of the resampler's result;
  * the pair resampler -> GroupNorm(32) + swish, once with the statistics from the resampler's own pass (odvae_groupnorm_fwd_partials_*) and
    once as plain resamplers would run it (no statistics from the resampler, odvae_groupnorm_fwd_* with its statistics pass);
  * the same pair through ops, as the modules call it -- ops.<resampler>(x, gn_stats=True) -> ops.group_norm_skip(swish) -- with the tag, with
    the tag removed by y.clone() (which also charges the copy to that variant) and with gn_stats=False (no tag, no copy); forward only;
  * one whole training step of the headline geometry with resamp_with_conv on and off (two different networks: information, not an A/B).
Everything in the first two groups goes through the C ABI on preallocated buffers: no autograd node, no allocation, a few microseconds of
host work per call, so the queue stays full and a window holds device time.
Timing: one HIP event pair around `reps` calls queued back to back, one synchronise per window; windows of the variants alternate, the
median over the rounds is reported (and the minimum, whose distance from the median is the spread of the session).
usage: python tools/resample_time.py [--reps R] [--rounds K] [--batch B] [--no-step] [--steps K] [--warmup W] [--json PATH]"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (kind, C, input H = W) at 256 x 256, ch = 128, ch_mult 1,1,2,2,4: the Encoder's four Downsamples, the Decoder's four Upsamples
LAYERS = [("down", 128, 256), ("down", 128, 128), ("down", 256, 64), ("down", 256, 32),
          ("up", 512, 16), ("up", 256, 32), ("up", 256, 64), ("up", 128, 128)]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(variants, reps, rounds):
    times = {k: [] for k in variants}
    for fn in variants.values():      # warm-up: code objects, workspace growth
        window(fn, 2)
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


def layer_times(kind, c, hw, batch, bf16, reps, rounds):
    from odvae_amd import lib
    L, st = lib.load(), lib.stream_ptr()
    dev = torch.device("cuda:0")
    dt, esz, sfx = (torch.bfloat16, 2, "bf16") if bf16 else (torch.float32, 4, "f32")
    up = kind == "up"
    n, h, w = batch, hw, hw
    ho, wo = (2 * h, 2 * w) if up else (h // 2, w // 2)
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(n, h, w, c, device=dev, generator=g) * 0.7 + 0.3).to(dt)          # NHWC
    y, z = torch.empty(n, ho, wo, c, device=dev, dtype=dt), torch.empty(n, ho, wo, c, device=dev, dtype=dt)
    dy = torch.randn(n, ho, wo, c, device=dev, generator=g).to(dt)
    dx = torch.empty_like(x)
    gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    mean, rstd = torch.empty(n, 32, device=dev), torch.empty(n, 32, device=dev)
    chunks = (L.odvae_conv_bf16_stats_chunks if bf16 else L.odvae_conv3x3_wino4_stats_chunks)(ho, wo)
    part = torch.empty(n, chunks, 32, 2, device=dev)
    gn_ws = getattr(L, "odvae_groupnorm_bf16_workspace_bytes" if bf16 else "odvae_groupnorm_workspace_bytes")
    wp, wn = lib.workspace.get(gn_ws(n, ho * wo, c, 32), dev)
    fwd = getattr(L, "odvae_%s_%s" % ("upsample2x" if up else "avgpool2x2", sfx))
    bwd = getattr(L, "odvae_%s_%s" % ("upsample2x_bwd" if up else "avgpool2x2_bwd", sfx))
    gn_fwd, gn_part, gn_apply = (getattr(L, "odvae_groupnorm_%s_%s" % (k, sfx)) for k in ("fwd", "fwd_partials", "apply"))

    def k_fwd():
        lib.check(fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, None, 0, 0, st), "resampler")

    def k_fwd_stats():
        lib.check(fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, part.data_ptr(), 32, chunks, st), "resampler + statistics")

    def k_bwd():
        lib.check(bwd(dy.data_ptr(), dx.data_ptr(), n, h, w, c, st), "resampler backward")

    def k_gn_partials():
        lib.check(gn_part(y.data_ptr(), n, ho * wo, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-6, 1, z.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                          part.data_ptr(), chunks, st), "groupnorm from partials")

    def k_gn_full():
        lib.check(gn_fwd(y.data_ptr(), n, ho * wo, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-6, 1, z.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                         wp, wn, st), "groupnorm")

    def k_gn_apply():
        lib.check(gn_apply(y.data_ptr(), n, ho * wo, c, 32, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1, z.data_ptr(), st), "groupnorm apply")

    def both(a_, b_):
        def call():
            a_(); b_()
        return call

    # through ops (forward only, no autograd graph): what Upsample / Downsample.forward + ResnetBlock.norm1 run; torch allocates the results
    from odvae_amd import ops
    xl = x.permute(0, 3, 1, 2)      # the logical NCHW view of the NHWC buffer
    resample = ops.upsample2x if up else ops.avg_pool2x2

    def o_pair(gn_stats, clone):
        def call():
            with torch.no_grad():
                r = resample(xl, gn_stats=gn_stats)
                ops.group_norm_skip(r.clone() if clone else r, gamma, beta, 32, 1e-6, swish=True)
        return call

    k_fwd_stats(); k_gn_partials()      # mean / rstd for the apply stream
    variants = {"forward": k_fwd, "forward + statistics": k_fwd_stats, "backward": k_bwd, "groupnorm apply stream": k_gn_apply,
                "pair, statistics from the resampler": both(k_fwd_stats, k_gn_partials), "pair, plain resampler": both(k_fwd, k_gn_full),
                "ops pair, tagged": o_pair(True, False), "ops pair, y.clone()": o_pair(True, True), "ops pair, gn_stats=False": o_pair(False, False)}
    ms, ms_min = measure(variants, reps, rounds)
    small, big = esz * n * c * min(h * w, ho * wo), esz * n * c * max(h * w, ho * wo)
    # algorithmic bytes: avg-pool reads what it uses of x (4 per result vector) and writes y; the upsampler reads x, writes 4x; backwards mirror
    used = esz * n * c * 4 * ho * wo if not up else big
    nbytes = {"forward": small + used, "forward + statistics": small + used, "backward": small + used, "groupnorm apply stream": 2 * esz * n * c * ho * wo}
    res = {"kind": kind, "dtype": sfx, "shape_in": [n, c, h, w], "shape_out": [n, c, ho, wo], "ms": ms, "ms_min": ms_min,
           "tbytes_per_s": {k: nbytes[k] / (ms[k] * 1e-3) / 1e12 for k in nbytes},
           "pair_tagged_over_plain": ms["pair, statistics from the resampler"] / ms["pair, plain resampler"],
           "ops_pair_tagged_over_clone": ms["ops pair, tagged"] / ms["ops pair, y.clone()"],
           "ops_pair_tagged_over_untagged": ms["ops pair, tagged"] / ms["ops pair, gn_stats=False"],
           "pair_spread": max((ms[k] - ms_min[k]) / ms[k] for k in ("pair, statistics from the resampler", "pair, plain resampler"))}
    print("%s %s  C=%d  %dx%d -> %dx%d  (B=%d)" % (kind, sfx, c, h, w, ho, wo, n))
    for k in variants:
        print("  %-38s median %8.4f ms   min %8.4f ms%s" % (k, ms[k], ms_min[k], "   %6.2f TB/s" % res["tbytes_per_s"][k] if k in nbytes else ""), flush=True)
    return res


def tanh_times(batch, reps, rounds):
    from odvae_amd import lib
    L, st = lib.load(), lib.stream_ptr()
    dev = torch.device("cuda:0")
    numel = batch * 3 * 256 * 256
    x = torch.randn(numel, device=dev)
    y, dy, dx = torch.empty_like(x), torch.randn(numel, device=dev), torch.empty_like(x)
    variants = {"tanh forward": lambda: lib.check(L.odvae_tanh_f32(x.data_ptr(), y.data_ptr(), numel, st), "tanh"),
                "tanh backward": lambda: lib.check(L.odvae_tanh_bwd_f32(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), numel, st), "tanh_bwd")}
    ms, ms_min = measure(variants, reps, rounds)
    res = {"numel": numel, "ms": ms, "ms_min": ms_min,
           "tbytes_per_s": {"tanh forward": 8.0 * numel / (ms["tanh forward"] * 1e-3) / 1e12, "tanh backward": 12.0 * numel / (ms["tanh backward"] * 1e-3) / 1e12}}
    for k in variants:
        print("  %-38s median %8.4f ms   min %8.4f ms   %6.2f TB/s" % (k, ms[k], ms_min[k], res["tbytes_per_s"][k]), flush=True)
    return res


def step_times(batch, steps, warmup):
    import warnings
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    yaml = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
    dev = torch.device("cuda:0")
    out = {"batch": batch, "steps": steps, "warmup": warmup}
    for precision in ("32", "bf16"):
        for with_conv in (True, False, True, False):
            torch.manual_seed(23)
            mcfg, _ = synthetic.model_config(yaml, latent_hw=16)
            mcfg.params.ddconfig["resamp_with_conv"] = with_conv
            model = instantiate_from_config(mcfg)
            model.learning_rate = 12 * 4.5e-6
            model = model.to(dev).train()
            model._global_step = 1
            trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision=precision)
            data = synthetic.make_batch(batch, 256, seed=23)
            data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}

            def step(i):
                b = dict(data)
                b["pose_6d"] = data["pose_6d"].clone()
                return trainer.training_batch(b, i)
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
            rec = {"ms_per_step": ms, "images_per_s": batch / ms * 1e3, "last_loss": float(loss[0])}
            name = "precision %s, resamp_with_conv %s" % (precision, with_conv)
            out.setdefault(name, []).append(rec)
            print(name, json.dumps(rec), flush=True)
            del model, trainer, data, loss
            gc.collect()
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py times kernels on the device: no HIP device found")
    res = {"reps": a.reps, "rounds": a.rounds, "layers": []}
    for bf16 in (False, True):
        for kind, c, hw in LAYERS:
            res["layers"].append(layer_times(kind, c, hw, a.batch, bf16, a.reps, a.rounds))
            gc.collect()
            torch.cuda.empty_cache()
    res["tanh"] = tanh_times(a.batch, a.reps, a.rounds)
    if not a.no_step:
        res["step"] = step_times(a.batch, a.steps, a.warmup)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
