"""The nine pose loss terms of pose_f32.hip and both gradients against the float64 reference of tests/pose_head_inputs.py, under the
acceptance rule derived in profiles/pose_head_exact.md: per output and per gradient element, never one scale for a vector.  The cases
walk the block stride (B = 1 .. 1000), the masks (foreground only in the last row, only past row 256, nowhere; every label
"background"), NC below, at and above 8, L = 1 and 3, both background indices, l1 / l2 with and without the yaw term, predicted yaws up
to 2000 rad, logits up to +-100 under gamma 2, 1.5, 1 and 0, log-variances on and just past the clamp, prior variances of 1e-6 and 1e3.
Then what must hold exactly: zero rows, zero and non-zero clamp gradients, the all-background batch, and that the upstream gradient
of the four logged means reaches nothing."""
import pytest
import torch

import pose_head_inputs as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c["name"] for c in P.POSE_CASES]
_REFS = {}


def ref_of(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = P.pose_reference(c)
    return _REFS[c["name"]]


def run_kernel(c, g9=P.G9):
    from odvae_amd import ops
    dp = c["dec_pose"].to(DEV).requires_grad_()
    mo = c["moments"].to(DEV).requires_grad_()
    out = ops.pose_losses(dp, mo, c["pose_gt"].to(DEV), c["bbox_gt"].to(DEV), c["fill_gt"].to(DEV), c["class_gt"].to(DEV),
                          c["prior"].to(DEV), c["prior_idx"].to(DEV), bg_idx=c["bg_idx"], l2=c["l2"], yaw=c["yaw"], gamma=c["gamma"],
                          alpha=c["alpha"])
    out.backward(torch.tensor(g9, device=DEV))
    return out.detach().cpu(), dp.grad.cpu(), mo.grad.cpu()


@pytest.mark.parametrize("name", CASE_IDS)
def test_pose_terms_and_gradients_under_the_rule(hip_lib, name):
    c = P.pose_case(name)
    ref = ref_of(c)
    out, d_pose, d_mom = run_kernel(c)
    print("pose_f32 %s: %s" % (name, {k: float("%.3g" % v) for k, v in P.rule_margins(ref, out, d_pose, d_mom).items()}))
    for what, t in (("out", out), ("d dec_pose", d_pose), ("d moments", d_mom)):
        assert torch.isfinite(t).all(), "%s holds NaN or inf" % what
    P.assert_rule(ref, out, d_pose, d_mom, "pose_f32 on " + name)


@pytest.mark.parametrize("name", ["B257", "fg_last", "fg_tail", "prior_neg", "NC8_L1_bg0", "NC40_L1_bg1", "l2_yaw0", "gamma0_alpha0.5"])
def test_masks_and_clamp_are_exact(hip_lib, name):
    c = P.pose_case(name)
    out, d_pose, d_mom = run_kernel(c)
    fg = c["class_gt"] != c["bg_idx"]
    keep = c["prior_idx"] >= 0
    assert (d_pose[~fg, :8] == 0).all(), "a masked sample has a gradient in its pose, box or fill columns"
    assert (d_mom[~keep] == 0).all(), "a sample labelled background has a gradient in its moments"
    lv = c["moments"][:, 8:]
    outside = (lv < -30.0) | (lv > 20.0)
    edge = ((lv == -30.0) | (lv == 20.0)) & keep[:, None]
    assert outside.any() and (d_mom[:, 8:][outside] == 0).all(), "a clamped log-variance carries a gradient"
    if name != "prior_neg":
        assert edge.any() and (d_mom[:, 8:][edge] != 0).all(), "a log-variance exactly on the clamp lost its gradient"
        assert (d_pose[fg, :8] != 0).any()
    else:
        assert out[4].item() == 0.0 and (d_mom == 0).all()


def test_all_background_batch(hip_lib):
    """Nothing is foreground: the four masked terms are exactly 0, and so is every gradient they own (d dec_pose[:, :8], d moments);
    the class term is a mean over all samples, masked or not, and stays finite and non-zero, like the four logged means."""
    c = P.pose_case("all_bg")
    out, d_pose, d_mom = run_kernel(c)
    for i in (0, 2, 3, 4):
        assert out[i].item() == 0.0, P.OUT_NAMES[i]
    assert (d_pose[:, :8] == 0).all() and (d_mom == 0).all()
    assert torch.isfinite(out).all() and (out[[1, 5, 6, 7, 8]] > 0).all()
    assert torch.isfinite(d_pose).all() and (d_pose[:, 8:] != 0).any()


def test_upstream_gradient_of_the_logged_means_reaches_nothing(hip_lib):
    """outputs 5 to 8 are only logged by the reference; the backward kernel ignores their upstream gradient"""
    c = P.pose_case(P.EDGE_CASE)
    _, d_pose, d_mom = run_kernel(c)
    _, d_pose2, d_mom2 = run_kernel(c, P.G9[:5] + [3.0, -2.0, 0.5, 7.0])
    assert torch.equal(d_pose, d_pose2) and torch.equal(d_mom, d_mom2)


def make_loss():
    """the PoseLoss of the committed yaml (l1, yaw term on), width-reduced as the other loss tests build it"""
    import os
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    mcfg, _ = synthetic.model_config(os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml"), latent_hw=4, ch=32)
    lc = mcfg.params.lossconfig
    lc.params["pose_loss_fn"] = "l1"
    lc.params["train_on_yaw"] = True
    return instantiate_from_config(lc).to(DEV)


@pytest.mark.parametrize("fused", [True, False])
def test_loss_forward_fused_and_per_term_under_the_same_rule(hip_lib, fused):
    """PoseLoss.forward itself on the edge batch, with fused_pose_terms on (the kernel) and off (the per-term torch-op branch of
    forward): the five logged terms, the four logged means and the gradients of the total loss w.r.t. dec_pose and the box moments,
    each against float64.  Before the discriminator starts the total is the weighted sum of the five pose-head terms, so its
    gradient is the reference's with the loss weights as upstream gradient."""
    from odvae_amd.distributions import DiagonalGaussianDistribution
    loss = make_loss()
    loss.fused_pose_terms = fused
    loss.perceptual_weight = 0.0          # the image terms are not under test and do not reach dec_pose or the box moments
    loss.disc_factor = 0.0
    rows, p_mean, p_var, p_logvar = loss._prior_table(torch.device(DEV))
    labs = [l for l in rows if l != "background"]
    c = dict(P.make_pose_case("fallback", 37, NC=loss.num_classes, L=3, gamma=loss.class_loss_fn.gamma, alpha=loss.class_loss_fn.alpha, seed=5))
    labels = ["background" if i < 0 else labs[i] for i in c["prior_idx"].tolist()]
    c["prior"] = torch.stack([p_mean, p_var, p_logvar], dim=1).float().cpu().contiguous()
    c["L"] = c["prior"].shape[0]
    c["prior_idx"] = torch.tensor([rows[l] if l != "background" else -1 for l in labels], dtype=torch.int32)
    g9 = [float(w) for w in (loss.pose_weight, loss.class_weight, loss.bbox_weight, loss.fill_factor_weight, loss.kl_weight_bbox)] + [0.0] * 4
    assert all(w != 0 for w in g9[:5])
    ref = P.pose_reference(c, g9)
    B = c["B"]
    g = torch.Generator().manual_seed(3)
    rgb, rec = (torch.randn(B, 3, 32, 32, generator=g).to(DEV) for _ in range(2))
    post_obj = DiagonalGaussianDistribution(torch.randn(B, 32, 4, 4, generator=g).to(DEV))
    dp, mo = c["dec_pose"].to(DEV).requires_grad_(), c["moments"].to(DEV).requires_grad_()
    total, log = loss(rgb, None, c["pose_gt"].to(DEV), rec, dp, c["class_gt"].to(DEV), labels, c["bbox_gt"].to(DEV), c["fill_gt"].to(DEV),
                      post_obj, DiagonalGaussianDistribution(mo), 0, 0, None, split="train")
    total.backward()
    out = torch.stack([log["train/" + k].detach().float().reshape(()) for k in
                       ("pose_loss", "class_loss", "bbox_loss", "fill_factor_loss", "kl_loss_bbox", "t1_loss", "t2_loss", "t3_loss", "v3_loss")]).cpu()
    margins = P.rule_margins(ref, out, dp.grad.cpu(), mo.grad.cpu())
    print("PoseLoss.forward, fused %s: %s" % (fused, {k: float("%.3g" % v) for k, v in margins.items()}))
    P.assert_rule(ref, out, dp.grad.cpu(), mo.grad.cpu(), "PoseLoss.forward, fused_pose_terms = %s" % fused)
