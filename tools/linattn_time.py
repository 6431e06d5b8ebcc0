"""Linear attention (ops.linear_attention_qkv, linattn_f32.hip) against the vanilla f32 attention core (ops.attention_qkv) at one shape:
each new kernel by itself, the whole core forward and forward + backward, and the column-statistics pass as a fraction of the HBM rate.
Timing: one HIP event pair around `reps` launches queued back to back (the queue stays full, the host never waits inside the window), one
synchronise per window; windows of the variants alternate, the median over the rounds is reported.
usage: python tools/linattn_time.py [N] [C] [T] [--no-vanilla] [--reps R] [--rounds K] [--json PATH]
       python tools/linattn_time.py --step RES BATCH [--bf16] [--ckpt] [--steps K] [--warmup W] [--json PATH]
--step: the whole training step of the benchmark's model (rec + KL, as bench.py builds it) with ddconfig.use_linear_attn against vanilla:
one event pair around the K timed steps of each, one after the other in one process (each model is freed before the next is built)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12      # bytes/s: data sheet; what a float4 copy reaches on this chip


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def step_mode(a):
    import gc
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    yaml = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
    res_px, batch = a.step
    dev = torch.device("cuda:0")
    out = {"res": res_px, "batch": batch, "bf16": a.bf16, "ckpt": a.ckpt, "steps": a.steps, "warmup": a.warmup}
    for name in ("vanilla", "linear", "vanilla", "linear"):
        torch.manual_seed(23)
        mcfg, _ = synthetic.model_config(yaml, latent_hw=res_px // 16)
        mcfg.params.ddconfig["use_linear_attn"] = name == "linear"
        model = instantiate_from_config(mcfg)
        model.learning_rate = 12 * 4.5e-6
        model = model.to(dev).train()
        model.decoder.activation_checkpoint = bool(a.ckpt)
        model._global_step = 1
        trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision="bf16" if a.bf16 else 32)
        data = synthetic.make_batch(batch, res_px, seed=23)
        data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}

        def step(i):
            b = dict(data)
            b["pose_6d"] = data["pose_6d"].clone()
            return trainer.training_batch(b, i)
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.steps):
            loss = step(a.warmup + i)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        rec = {"ms_per_step": ms, "images_per_s": batch / ms * 1e3, "peak_device_memory_gb": torch.cuda.max_memory_allocated(dev) / 1e9,
               "last_loss": float(loss[0])}
        out.setdefault(name, []).append(rec)
        print(name, json.dumps(rec), flush=True)
        del model, trainer, data, loss
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2, metavar=("RES", "BATCH"), default=None)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--ckpt", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("n", type=int, nargs="?", default=32)
    ap.add_argument("c", type=int, nargs="?", default=256)
    ap.add_argument("t", type=int, nargs="?", default=4096)
    ap.add_argument("--no-vanilla", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        return step_mode(a)
    from odvae_amd import lib, ops
    L = lib.load()
    n, c, t = a.n, a.c, a.t
    h = max(d for d in range(1, int(t ** 0.5) + 1) if t % d == 0)
    w = t // h
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(n, 3 * c, h, w, device=dev, generator=g) * 0.6).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    go = torch.randn(n, c, h, w, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    c3, sq, st = 3 * c, t * 3 * c, lib.stream_ptr()
    q, k, v = ops._qkv_views(qkv.detach(), c)
    stats = torch.empty(2, n, c, device=dev)
    cx, dcx = torch.empty(n, c, c, device=dev), torch.randn(n, c, c, device=dev, generator=g)
    gd = torch.randn(n, c, device=dev, generator=g)
    dqkv = torch.empty_like(qkv.detach())
    _, dk, dv = ops._qkv_views(dqkv, c)
    ws, wn = lib.workspace.get(max(L.odvae_linattn_colstats_workspace_bytes(n, t, c), L.odvae_linattn_ctx_workspace_bytes(n, t, c)), dev)

    def colstats():
        lib.check(L.odvae_linattn_colstats_f32(k.data_ptr(), c3, sq, n, t, c, stats[0].data_ptr(), stats[1].data_ptr(), ws, wn, st), "colstats")

    def context():
        lib.check(L.odvae_linattn_ctx_f32(k.data_ptr(), v.data_ptr(), c3, sq, stats[0].data_ptr(), stats[1].data_ptr(), n, t, c,
                                          cx.data_ptr(), ws, wn, st), "ctx")

    def dkv():
        lib.check(L.odvae_linattn_dkv_f32(k.data_ptr(), v.data_ptr(), c3, sq, stats[0].data_ptr(), stats[1].data_ptr(), dcx.data_ptr(),
                                          gd.data_ptr(), n, t, c, dk.data_ptr(), dv.data_ptr(), c3, sq, st), "dkv")

    def core(fn, backward):
        def run():
            o = fn(qkv)
            if backward:
                o.backward(go)
                qkv.grad = None
        return run

    variants = {"colstats": colstats, "ctx": context, "dkv": dkv,
                "linear fwd": core(ops.linear_attention_qkv, False), "linear fwd+bwd": core(ops.linear_attention_qkv, True)}
    if not a.no_vanilla:
        variants["vanilla fwd"] = core(ops.attention_qkv, False)
        variants["vanilla fwd+bwd"] = core(ops.attention_qkv, True)
    times = {name: [] for name in variants}
    for name, fn in variants.items():      # warm-up: code objects, workspace growth, the allocator's blocks
        window(fn, 2)
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(window(fn, a.reps))
    res = {"N": n, "C": c, "T": t, "reps": a.reps, "rounds": a.rounds, "ms": {k_: statistics.median(v_) for k_, v_ in times.items()},
           "ms_min": {k_: min(v_) for k_, v_ in times.items()}}
    ms = res["ms"]
    stat_bytes = 4.0 * n * t * c
    res["colstats_bytes_per_s"] = stat_bytes / (ms["colstats"] * 1e-3)
    res["colstats_fraction_of_hbm_spec"] = res["colstats_bytes_per_s"] / HBM_SPEC
    res["colstats_fraction_of_hbm_copy_rate"] = res["colstats_bytes_per_s"] / HBM_COPY
    res["ctx_tflops"] = 2.0 * t * c * c * n / (ms["ctx"] * 1e-3) / 1e12
    res["dkv_tflops"] = 4.0 * t * c * c * n / (ms["dkv"] * 1e-3) / 1e12
    if not a.no_vanilla:
        res["vanilla_over_linear_fwd_bwd"] = ms["vanilla fwd+bwd"] / ms["linear fwd+bwd"]
    for name in variants:
        print("%-18s median %9.3f ms   min %9.3f ms" % (name, ms[name], res["ms_min"][name]), flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
