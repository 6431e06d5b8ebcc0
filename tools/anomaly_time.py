"""Cost of anomaly detection on the benchmark step: the same training step timed with detection off, with the device-side mode
(Trainer(detect_anomaly=True): hooks + anomaly_scan_kernel + one wait per optimizer step) and under torch's own
torch.autograd.set_detect_anomaly(True) (one host sync per backward output).  Also prints, for the device mode, the hook firings and
watched nodes per step, the host time of the hooks and the bytes scanned per step (counted from the shapes).

    python tools/anomaly_time.py [--res 256] [--batch 32] [--bf16] [--steps 6] [--warmup 2] [--modes off,device,torch]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def run(mode, args):
    import torch
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=args.res // 16).to("cuda:0").train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision="bf16" if args.bf16 else None,
                      detect_anomaly=(mode == "device"))
    batch = synthetic.make_batch(args.batch, args.res, seed=23)
    batch = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step(i):
        b = dict(batch)
        b["pose_6d"] = batch["pose_6d"].clone()
        return trainer.training_batch(b, i)
    with warnings.catch_warnings(), torch.autograd.set_detect_anomaly(mode == "torch"):
        warnings.simplefilter("ignore")
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        an = trainer.anomaly
        h0, b0 = (an.hook_seconds, an.bytes_scanned) if an else (0.0, 0)
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
    out = {"mode": mode, "ms_per_step": dt * 1e3, "images_per_s": args.batch / dt}
    if an:
        st = an.stats()
        out.update(firings_per_step=st["firings"], watched_nodes=st["watched"], fallbacks=st["fallbacks"],
                   hook_ms_per_step=(an.hook_seconds - h0) / args.steps * 1e3, gb_scanned_per_step=(an.bytes_scanned - b0) / args.steps / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="off,device,torch")
    args = ap.parse_args()
    for mode in args.modes.split(","):
        print(json.dumps(run(mode, args)), flush=True)


if __name__ == "__main__":
    main()
