"""What a run that sets neither `weights` nor `cond` computes, sampled the way `bench.py --dump-outputs` samples a step:

  * two training batches (both optimizers) of the width-reduced PoseAutoencoder -- ch = 32, 32 x 32, B = 4, VAE phase, LPIPS-style and
    PatchGAN terms on, f32, no cond_key / loss_weights_key: the losses, every logged scalar, a fixed sample of the parameters afterwards;
  * the plain LPIPSWithDiscriminator.forward (optimizer_idx 0, on both sides of disc_start) with weights None, a scalar and one weight per
    sample ([N]): the total, every logged scalar and the gradient at the reconstruction and at logvar.

    python tests/golden/weights_cond_unset_step.py        # on an MI355X, at the commit BEFORE weights and disc_conditional were honoured

wrote tests/golden/weights_cond_unset_parent.npz; tests/test_loss_weights_cond_gpu.py runs `run_steps` again and asserts the same bits:
honouring the two arguments changed nothing for a run that does not pass them, nor for the weights the loss already took.  Uses only what
that earlier commit already had."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
YAML = os.path.join(HERE, "autoencoder_kl_16x16x16.yaml")
OUT = os.path.join(HERE, "weights_cond_unset_parent.npz")


def pose_steps(arrays, device):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(31)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=2, ch=32, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
    synthetic.fill_state_procedural(model, seed=29)
    model = model.to(device).train()
    trainer = Trainer(model, gradient_clip_val=1.0)
    for step in range(2):
        batch = synthetic.make_batch(4, 32, seed=140 + step)
        batch["mask_2d_bbox"][2, :, :, 12:] = 0.0
        model.injected_noise = synthetic.make_noise(4, 2, seed=150 + step)
        losses = trainer.training_batch(batch, step)
        arrays["pose.step%d.loss" % step] = np.array([float(x.item()) for x in losses], dtype=np.float32)
        for k, v in sorted(model.logged_metrics.items()):
            arrays["pose.step%d.log.%s" % (step, k)] = np.float32(float(v))
    flat = torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()])
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))[:4096].sort().values
    arrays["pose.params_sample"] = flat[idx.to(flat.device)].cpu().numpy()
    arrays["pose.params_count"] = np.int64(flat.numel())


def plain_loss_calls(arrays, device):
    from odvae_amd import synthetic
    from odvae_amd.distributions import DiagonalGaussianDistribution
    from odvae_amd.losses import LPIPSWithDiscriminator
    torch.manual_seed(7)
    loss = LPIPSWithDiscriminator(disc_start=10, kl_weight=0.3, disc_weight=0.5, perceptual_weight=1.0, disc_factor=1.0)

    class Holder(torch.nn.Module):      # fill_state_procedural keys its draws by the state_dict key: the model's `loss.` prefix
        def __init__(self, loss):
            super().__init__()
            self.loss = loss
    synthetic.fill_state_procedural(Holder(loss), seed=37)
    with torch.no_grad():
        loss.logvar.fill_(0.25)
        for name, p in loss.discriminator.named_parameters():
            if p.dim() == 1 and name.endswith("weight"):
                p.add_(1.0)
    loss = loss.to(device).train()
    state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(3, 3, 32, 32, generator=g) * 2 - 1).to(device)
    xr0 = (torch.rand(3, 3, 32, 32, generator=g) * 2 - 1).to(device)
    moments = (torch.randn(3, 8, 16, 16, generator=g) * 0.5).to(device)
    kinds = {"none": None, "scalar": 0.5, "scalar_tensor": torch.tensor(2.0), "sample": torch.tensor([0.5, 1.75, 1.0]).to(device)}
    for name, weights in kinds.items():
        for gs in (9, 10):
            loss.discriminator.load_state_dict(state)
            loss.zero_grad(set_to_none=True)
            leaf = xr0.clone().requires_grad_(True)
            gain = torch.ones(3, device=device, requires_grad=True)
            total, log = loss(x, leaf * gain.view(1, 3, 1, 1), DiagonalGaussianDistribution(moments.clone()), 0, gs, last_layer=gain, weights=weights)
            total.backward()
            pre = "plain.%s.step%d" % (name, gs)
            arrays[pre + ".loss"] = np.float32(float(total))
            for k, v in sorted(log.items()):
                arrays[pre + ".log." + k] = np.float32(float(v))
            arrays[pre + ".grad.reconstruction"] = leaf.grad.reshape(-1)[::7].cpu().numpy()
            arrays[pre + ".grad.logvar"] = np.float32(float(loss.logvar.grad))


def run_steps(device="cuda:0"):
    arrays = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (the synthetic-LPIPS-weights warning)
        pose_steps(arrays, device)
        plain_loss_calls(arrays, device)
    return arrays


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    arrays = run_steps()
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
