"""Two training batches (both optimizers) of the width-reduced PoseAutoencoder WITHOUT image_mask_key -- ch = 32, 32 x 32, B = 4, VAE phase,
LPIPS-style and PatchGAN terms on, f32 -- sampled the way `bench.py --dump-outputs` samples a step: the losses, every logged scalar, and a
fixed sample of the parameters after the optimizer steps.

    python tests/golden/mask_unset_step.py        # on an MI355X, at the commit BEFORE image_mask_key was honoured

wrote tests/golden/mask_unset_parent.npz; tests/test_image_mask_gpu.py runs `run_steps` again and asserts the same bits: honouring the key
changed nothing for a model that does not set it.  Uses only what that earlier commit already had."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
YAML = os.path.join(HERE, "autoencoder_kl_16x16x16.yaml")
OUT = os.path.join(HERE, "mask_unset_parent.npz")


def run_steps(device="cuda:0"):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(29)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=2, ch=32, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
    synthetic.fill_state_procedural(model, seed=23)
    model = model.to(device).train()
    trainer = Trainer(model, gradient_clip_val=1.0)
    arrays = {}
    for step in range(2):
        batch = synthetic.make_batch(4, 32, seed=40 + step)
        batch["mask_2d_bbox"][1, :, :10, :] = 0.0
        model.injected_noise = synthetic.make_noise(4, 2, seed=50 + step)
        losses = trainer.training_batch(batch, step)
        arrays["step%d.loss" % step] = np.array([float(x.item()) for x in losses], dtype=np.float32)
        for k, v in sorted(model.logged_metrics.items()):
            arrays["step%d.log.%s" % (step, k)] = np.float32(float(v))
    flat = torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()])
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))[:4096].sort().values
    arrays["params_sample"] = flat[idx.to(flat.device)].cpu().numpy()
    arrays["params_count"] = np.int64(flat.numel())
    return arrays


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    arrays = run_steps()
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
