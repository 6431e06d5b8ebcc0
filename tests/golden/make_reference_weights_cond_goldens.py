"""Generates tests/golden/reference_weights_cond.npz by RUNNING the reference's own, unmodified PoseLoss.forward with its `weights` and
`cond` arguments (src/modules/losses/contperceptual.py:147-158: weights * nll_loss on [B,3,H,W]; :283-289,354-361: torch.cat((x, cond), 1)
in front of the discriminator) on the stand-ins of make_reference_goldens.py.

Shape B = 4, 32 x 32, dec_obj = conv3x3(feat) (so that last_layer reaches the loss), one sample of the masked class id 1, two partial boxes.
Cases: weights in {None, 0.5, [B,1,1,1], [B,1,H,W], [B,3,H,W], [1,1,H,W]} x cond in {None, [B,2,H,W]} (disc_conditional and
disc_in_channels 5 with it) x global_step in {5, 12, 20, 40} under reference_cases.LOSS_KW's thresholds (encoder_pretrain_steps 10,
disc_start 15, pixel loss from 30) x optimizer_idx in {0, 1}; plus one RGBA sequence (image_mask_key: a 4-channel dec_obj and an alpha
mask, mask loss off) with cond (disc_in_channels 6) and the per-pixel weight.

The reference's code runs here in FLOAT64 (module.double(), float64 inputs: the same f32 weights and inputs, exactly), as in
make_reference_mask_goldens.py.  Stored: the inputs (f32), every logged key, the loss, and a digest of the gradient w.r.t. dec_obj.
Weights of the networks follow from fill_state_procedural, so none are stored.

Build container only (the reference does not travel):

    python tests/golden/make_reference_weights_cond_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT]
OUT = os.path.join(HERE, "reference_weights_cond.npz")

from make_reference_goldens import install_standins, import_reference, np_, stats_pickle  # noqa: E402
from reference_cases import LABELS, LOSS_KW, digest_of  # noqa: E402

B, H, CFEAT = 4, 32, 8
CLASS_IDS = [0, 1, 3, 0]
STEPS = (5, 12, 20, 40)
WEIGHT_KINDS = ("none", "scalar", "sample", "pixel", "element", "shared")
COND_CHANNELS = 2
DIGEST = dict(limit=1024, keep=512)


def inputs(seed=400):
    g = torch.Generator().manual_seed(seed)
    d = {"rgb_gt": torch.rand(B, 3, H, H, generator=g) * 2 - 1, "mask_gt": (torch.rand(B, 1, H, H, generator=g) < 0.5).float(),
         "feat": torch.randn(B, CFEAT, H, H, generator=g), "last_w": torch.randn(3, CFEAT, 3, 3, generator=g) * 0.1,
         "last_b": torch.randn(3, generator=g) * 0.1, "last_w4": torch.randn(4, CFEAT, 3, 3, generator=g) * 0.1,
         "last_b4": torch.randn(4, generator=g) * 0.1, "dec_pose": torch.randn(B, 19, generator=g), "pose_gt": torch.randn(B, 4, generator=g),
         "bbox_gt": torch.randn(B, 3, generator=g), "fill_factor_gt": torch.rand(B, generator=g),
         "moments": torch.randn(B, 32, 2, 2, generator=g) * 0.5, "bbox_moments": torch.randn(B, 16, generator=g) * 0.5,
         "class_id": torch.tensor(CLASS_IDS, dtype=torch.int64),
         "cond": torch.rand(B, COND_CHANNELS, H, H, generator=g),
         "w_sample": 0.25 + 1.75 * torch.rand(B, 1, 1, 1, generator=g), "w_pixel": 0.25 + 1.75 * torch.rand(B, 1, H, H, generator=g),
         "w_element": 0.25 + 1.75 * torch.rand(B, 3, H, H, generator=g), "w_shared": 0.25 + 1.75 * torch.rand(1, 1, H, H, generator=g)}
    box = torch.ones(B, 1, H, H)
    box[1, :, :10, :] = 0.0       # two partial boxes
    box[2, :, :, 20:] = 0.0
    d["mask_2d_bbox"] = box
    return d


def weights_of(d, kind):
    return {"none": None, "scalar": 0.5, "sample": d["w_sample"], "pixel": d["w_pixel"], "element": d["w_element"], "shared": d["w_shared"]}[kind]


def run_case(arrays, pre, loss, ref_dist, d, opt, gs, weights, cond, rgba=False):
    from odvae_amd.synthetic import fill_state_procedural
    feat = d["feat"].clone().requires_grad_(True)
    last_w = (d["last_w4"] if rgba else d["last_w"]).clone().requires_grad_(True)
    dec_obj = torch.nn.functional.conv2d(feat, last_w, d["last_b4"] if rgba else d["last_b"], padding=1)
    dec_pose = d["dec_pose"].clone().requires_grad_(True)
    post = ref_dist.DiagonalGaussianDistribution(d["moments"].clone().requires_grad_(True))
    bpost = ref_dist.DiagonalGaussianDistribution(d["bbox_moments"].clone().requires_grad_(True))
    fill_state_procedural(loss.discriminator, seed=31)      # BatchNorm buffers back to the same start for every call
    for p in loss.parameters():
        p.grad = None
    out, log = loss(d["rgb_gt"], d["mask_gt"] if rgba else None, d["pose_gt"], dec_obj, dec_pose, d["class_id"], [LABELS[c] for c in CLASS_IDS],
                    d["bbox_gt"], d["fill_factor_gt"], post, bpost, opt, gs, d["mask_2d_bbox"], last_layer=last_w, cond=cond, split="train",
                    weights=weights)
    assert out.dim() == 0
    arrays[pre + ".loss"] = np_(out.detach().double())
    for k, v in log.items():
        arrays[pre + ".log." + k] = np_(torch.as_tensor(v).double())
    if out.requires_grad:
        dec_obj.retain_grad()      # only now: calculate_adaptive_weight's autograd.grad passes run through dec_obj inside forward
        out.backward()
        if dec_obj.grad is not None:
            arrays[pre + ".grad.dec_obj.norm"], arrays[pre + ".grad.dec_obj.samples"] = digest_of(dec_obj.grad, **DIGEST)


def main():
    from odvae_amd.synthetic import fill_state_procedural
    torch.set_num_threads(4)
    install_standins()
    _, ref_loss, ref_dist = import_reference()
    arrays = {}
    d = inputs()
    for k, v in d.items():
        arrays["in." + k] = np_(v)      # f32, as a test hands them to the device
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}
    arrays["in.global_steps"] = np.array(STEPS, dtype=np.int64)

    def make(**kw):
        path, _ = stats_pickle()
        torch.manual_seed(5)
        loss = ref_loss.PoseLoss(dataset_stats_path=path, **dict(LOSS_KW, **kw))
        os.unlink(path)
        fill_state_procedural(loss, seed=31)
        with torch.no_grad():
            loss.logvar.fill_(0.3)
        loss = loss.double().train()      # the same f32 weights, evaluated in float64
        loss.perceptual_loss.eval()
        return loss

    for with_cond in (False, True):
        loss = make(disc_conditional=True, disc_in_channels=3 + COND_CHANNELS) if with_cond else make()
        arrays["state_keys.cond%d" % with_cond] = np.array(sorted(loss.state_dict().keys()))
        for kind in WEIGHT_KINDS:
            for gs in STEPS:
                for opt in (0, 1):
                    run_case(arrays, "%s.cond%d.step%d.opt%d" % (kind, with_cond, gs, opt), loss, ref_dist, d, opt, gs, weights_of(d, kind),
                             d["cond"] if with_cond else None)
    loss = make(disc_conditional=True, disc_in_channels=4 + COND_CHANNELS, use_mask_loss=False)
    for gs in STEPS:
        for opt in (0, 1):
            run_case(arrays, "rgba.pixel.cond1.step%d.opt%d" % (gs, opt), loss, ref_dist, d, opt, gs, d["w_pixel"], d["cond"], rgba=True)
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
