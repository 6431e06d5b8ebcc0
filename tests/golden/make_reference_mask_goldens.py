"""Generates tests/golden/reference_mask.npz by RUNNING the reference's own, unmodified PoseLoss.forward with an alpha mask
(image_mask_key: src/modules/losses/contperceptual.py:230-257,166-174,270) on the stand-ins of make_reference_goldens.py.

Shape B = 4, 32 x 32, a 4-channel dec_obj = conv3x3(feat) (so that last_layer is [4,C,3,3] and reaches the loss), one sample of the masked
class id 1, two partial boxes.  Cases: use_mask_loss in {True, False} x mask_loss_fn in {l1, l2} x global_step in {5, 12, 20, 40} under
reference_cases.LOSS_KW's thresholds (encoder_pretrain_steps 10, disc_start 15, pixel loss from 30) x optimizer_idx in {0, 1}, with
mask_weight 0.5, perceptual_weight 1, disc_in_channels 4; plus one "sticky" sequence per mask loss: a call without a mask (optimizer_idx 2,
which evaluates everything and returns None, :214-375) followed by a call with one, which finds use_mask_loss off (QUIRK :232).

The reference's code runs here in FLOAT64 (module.double(), float64 inputs: the same f32 weights and inputs, exactly), so that the fixture
holds what the reference computes and not the rounding of one f32 evaluation of it -- in f32 the reference's own d_weight, a ratio of two
gradient norms, sits 5e-6 from the float64 value, the whole tolerance of a device test.

Stored: the inputs (f32), every logged key, the SHAPE of the returned loss (with use_mask_loss past encoder_pretrain_steps the reference returns
a [B,1,H,W] tensor: weighted_mask_loss is left unreduced, :168-170) with its mean, and a digest of the gradient w.r.t. dec_obj -- of the
scalar loss, or of loss.mean() in the tensor case.  Weights follow from fill_state_procedural, so none are stored.

Build container only (the reference does not travel):

    python tests/golden/make_reference_mask_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT]
OUT = os.path.join(HERE, "reference_mask.npz")

from make_reference_goldens import install_standins, import_reference, np_, stats_pickle  # noqa: E402
from reference_cases import LABELS, LOSS_KW, digest_of  # noqa: E402

B, H, CFEAT = 4, 32, 8
CLASS_IDS = [0, 1, 3, 0]
STEPS = (5, 12, 20, 40)
MASK_KW = dict(mask_weight=0.5, perceptual_weight=1.0, disc_in_channels=4)
DIGEST = dict(limit=1024, keep=512)      # of the [4,4,32,32] gradient: its norm and every 32nd element


def mask_inputs(seed=300):
    g = torch.Generator().manual_seed(seed)
    d = {"rgb_gt": torch.rand(B, 3, H, H, generator=g) * 2 - 1, "mask_gt": (torch.rand(B, 1, H, H, generator=g) < 0.5).float(),
         "feat": torch.randn(B, CFEAT, H, H, generator=g), "last_w": torch.randn(4, CFEAT, 3, 3, generator=g) * 0.1,
         "last_b": torch.randn(4, generator=g) * 0.1, "dec_pose": torch.randn(B, 19, generator=g), "pose_gt": torch.randn(B, 4, generator=g),
         "bbox_gt": torch.randn(B, 3, generator=g), "fill_factor_gt": torch.rand(B, generator=g),
         "moments": torch.randn(B, 32, 2, 2, generator=g) * 0.5, "bbox_moments": torch.randn(B, 16, generator=g) * 0.5,
         "class_id": torch.tensor(CLASS_IDS, dtype=torch.int64)}
    box = torch.ones(B, 1, H, H)
    box[1, :, :10, :] = 0.0       # two partial boxes
    box[2, :, :, 20:] = 0.0
    d["mask_2d_bbox"] = box
    return d


def run_case(arrays, pre, loss, ref_dist, d, opt, gs, with_mask=True):
    from odvae_amd.synthetic import fill_state_procedural
    feat = d["feat"].clone().requires_grad_(True)
    last_w = d["last_w"].clone().requires_grad_(True)
    dec_obj = torch.nn.functional.conv2d(feat, last_w, d["last_b"], padding=1)
    dec_pose = d["dec_pose"].clone().requires_grad_(True)
    post = ref_dist.DiagonalGaussianDistribution(d["moments"].clone().requires_grad_(True))
    bpost = ref_dist.DiagonalGaussianDistribution(d["bbox_moments"].clone().requires_grad_(True))
    fill_state_procedural(loss.discriminator, seed=31)      # BatchNorm buffers back to the same start for every call
    for p in loss.parameters():
        p.grad = None
    ret = loss(d["rgb_gt"], d["mask_gt"] if with_mask else None, d["pose_gt"], dec_obj, dec_pose, d["class_id"], [LABELS[c] for c in CLASS_IDS],
               d["bbox_gt"], d["fill_factor_gt"], post, bpost, opt, gs, d["mask_2d_bbox"], last_layer=last_w, split="train")
    if ret is None:
        return
    out, log = ret
    arrays[pre + ".loss_shape"] = np.array(tuple(out.shape), dtype=np.int64)
    arrays[pre + ".loss_mean"] = np_(out.detach().mean())
    for k, v in log.items():
        arrays[pre + ".log." + k] = np_(torch.as_tensor(v).double())
    if out.requires_grad:
        # retain_grad only now: calculate_adaptive_weight's two autograd.grad passes run through dec_obj inside forward, and a tensor
        # that already retains its gradient would add theirs to .grad
        dec_obj.retain_grad()
        out.mean().backward()
        if dec_obj.grad is not None:
            arrays[pre + ".grad.dec_obj.norm"], arrays[pre + ".grad.dec_obj.samples"] = digest_of(dec_obj.grad, **DIGEST)


def main():
    from odvae_amd.synthetic import fill_state_procedural
    torch.set_num_threads(4)
    install_standins()
    _, ref_loss, ref_dist = import_reference()
    arrays = {}
    d = mask_inputs()
    for k, v in d.items():
        arrays["in." + k] = np_(v)      # f32, as a test hands them to the device
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}
    arrays["in.global_steps"] = np.array(STEPS, dtype=np.int64)

    def make(uml, fn):
        path, _ = stats_pickle()
        torch.manual_seed(5)
        loss = ref_loss.PoseLoss(dataset_stats_path=path, **dict(LOSS_KW, mask_loss_fn=fn, use_mask_loss=uml, **MASK_KW))
        os.unlink(path)
        fill_state_procedural(loss, seed=31)
        with torch.no_grad():
            loss.logvar.fill_(0.3)
        loss = loss.double().train()      # the same f32 weights, evaluated in float64
        loss.perceptual_loss.eval()
        return loss

    for uml in (True, False):
        for fn in ("l1", "l2"):
            loss = make(uml, fn)
            for gs in STEPS:
                for opt in (0, 1):
                    run_case(arrays, "mask.uml%d.%s.step%d.opt%d" % (int(uml), fn, gs, opt), loss, ref_dist, d, opt, gs)
                    assert loss.use_mask_loss == uml
    for fn in ("l1", "l2"):
        loss = make(True, fn)
        run_case(arrays, "unused", loss, ref_dist, d, 2, 40, with_mask=False)       # no mask: use_mask_loss goes off ...
        assert loss.use_mask_loss is False
        run_case(arrays, "sticky.%s.step40.opt0" % fn, loss, ref_dist, d, 0, 40)    # ... and stays off
    arrays["state_keys"] = np.array(sorted(loss.state_dict().keys()))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))
    for k in sorted(arrays):
        if k.endswith("loss_shape"):
            print(k, arrays[k].tolist(), float(arrays[k[:-len("shape")] + "mean"]))


if __name__ == "__main__":
    main()
