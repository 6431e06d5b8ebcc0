"""The plain AutoencoderKL / LPIPSWithDiscriminator on the HIP kernels against the float64 restatement of the upstream methods
(tests/plain_vae_ref.py), same weights (synthetic.fill_state_procedural), same tensors, same injected noise.

Geometry: ch 32, ch_mult [1, 2], num_res_blocks 1, attn_resolutions [16], resolution 32, N = 2, 32 x 32 images -- the smallest at which
the discriminator's five 4x4 layers and the VGG stack's four pools still have output; z_channels = embed_dim = 4, and once 3 (the kl-f4
layout: 6-channel moments, 3-channel latent, through the thin and direct conv routes).

Bounds are 4x what was measured on an MI355X (profiles/plain_vae.md lists measured value and bound per comparison); deviations are
relative to max|ref|, gradients to max(|ref grad|, 1e-3 * the largest gradient of the comparison), as in tests/test_model_gpu.py:
  loss level   logged values and total  TOL_LOSS_OUT,  gradients at the reconstruction, logvar, the moments  TOL_LOSS_GRAD,  of the
               discriminator's parameters  TOL_LOSS_GRAD_D;  one pass against three passes  TOL_ONE_PASS
  PoseLoss cross-check (the same kernels in the same order on the same device)  TOL_CROSS
  model level  reconstruction, moments, loss terms, pictures  TOL_MODEL_OUT,  parameter gradients  TOL_MODEL_GRAD,  losses of the
               three-batch loop  TOL_CURVE
The output bounds are below those of the corresponding PoseAutoencoder tests (tests/test_model_gpu.py: outputs 2e-5); TOL_MODEL_GRAD
(1.6e-4) is above the 1.2e-4 of its flip-free gradient test and below the 4.4e-4 of its test at this width: profiles/plain_vae.md says why."""
import os
import warnings

import pytest
import torch

import plain_vae_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PLAIN_YAML = os.path.join(GOLDEN, "autoencoder_kl_plain.yaml")
POSE_YAML = os.path.join(GOLDEN, "autoencoder_kl_16x16x16.yaml")
DEV = "cuda:0"
SMALL = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
         "model.params.ddconfig.resolution=32"]

# 4 x the worst figure measured on an MI355X (profiles/plain_vae.md)
TOL_LOSS_OUT = 1.2e-6        # measured 2.8e-7 (d_weight, mean of the real logits)
TOL_LOSS_GRAD = 4.1e-6       # measured 1.0e-6 (gradient at the reconstruction; moments 1.5e-7, logvar 4.1e-8)
TOL_LOSS_GRAD_D = 2.8e-5     # measured 6.8e-6 (a discriminator BatchNorm scale: five layers of f32 sums behind it)
TOL_CROSS = 3.4e-7           # measured 8.4e-8 (total; g_loss 3.0e-8; every other term and every gradient came out bit-identical)
TOL_ONE_PASS = 3.4e-6        # measured 8.5e-7 (gradient at the reconstruction: two f32 addends in the other order; all else identical)
TOL_MODEL_OUT = 1.2e-5       # measured 2.8e-6 (samples / reconstruction; loss terms 7.3e-7)
TOL_MODEL_GRAD = 1.6e-4      # measured 3.9e-5 (z = 3: encoder.down.0.block.0.conv1.bias, a conv bias in front of a GroupNorm, whose gradient is what
                             # is left of 1 024 terms that nearly cancel; tests/test_model_gpu.py measures 1.2e-4 on such a bias.  z = 4: 2.3e-5)
TOL_CURVE = 2e-6             # measured 4.9e-7 (loss after up to six optimizer steps)


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


def grad_rel(got, want, scale):
    return (got.detach().cpu().double() - want.double()).abs().max().item() / max(want.abs().max().item(), 1e-3 * scale, 1e-30)


class Worst:
    """the worst figure per name over a test, printed once: what profiles/plain_vae.md records"""

    def __init__(self, title):
        self.title, self.v = title, {}

    def __call__(self, name, value, where=""):
        if value > self.v.get(name, (-1.0, ""))[0]:
            self.v[name] = (value, where)
        return value

    def report(self):
        print("%s: %s" % (self.title, ", ".join("%s %.3e%s" % (k, v, " (%s)" % w if w else "") for k, (v, w) in sorted(self.v.items()))))

    def check(self, bounds=None, **more):
        bounds = dict(bounds or {}, **more)
        self.report()
        for name, bound in bounds.items():
            hit = [(k, v, w) for k, (v, w) in self.v.items() if k.startswith(name) and not v <= bound]
            assert not hit, "%s: %s over the bound %.1e" % (self.title, hit, bound)


def liven_discriminator(disc):
    """fill_state_procedural leaves the discriminator's BatchNorm scales at 0.05 N(0, 1): its logits then sit within 0.1 of zero, no hinge is
    ever at its kink, and d g_loss / d x_rec is so small that the adaptive weight is clamped at its ceiling -- a constant.  Scales of 1 + that
    spread the logits over several units and bring the adaptive weight inside (0, 1e4)."""
    with torch.no_grad():
        for name, p in disc.named_parameters():
            if p.dim() == 1 and name.endswith("weight"):
                p.add_(1.0)


def quiet():
    ctx = warnings.catch_warnings()
    ctx.__enter__()
    warnings.simplefilter("ignore")      # (the synthetic-LPIPS-weights warning)
    return ctx


# ------------------------------------------------------------------------------------------------------------------------------
# loss level
# ------------------------------------------------------------------------------------------------------------------------------
def loss_pair(disc_loss="hinge", perceptual_weight=1.0, disc_factor=1.0, disc_start=10, seed=23):
    from odvae_amd import synthetic
    from odvae_amd.losses import LPIPSWithDiscriminator
    kw = dict(disc_start=disc_start, kl_weight=0.3, disc_weight=0.5, disc_loss=disc_loss, perceptual_weight=perceptual_weight,
              disc_factor=disc_factor)
    loss = LPIPSWithDiscriminator(**kw)

    class Holder(torch.nn.Module):      # fill_state_procedural keys its draws by the state_dict key: the model's `loss.` prefix
        def __init__(self, loss):
            super().__init__()
            self.loss = loss
    synthetic.fill_state_procedural(Holder(loss), seed=seed)
    liven_discriminator(loss.discriminator)
    with torch.no_grad():
        loss.logvar.fill_(0.25)
    ref = R.PlainLoss(**kw).double()
    ref.load_state_dict(loss.state_dict(), strict=True)
    return loss.to(DEV), ref


def loss_tensors(seed=5):
    """x, x_rec with |x_rec - x| >= 1e-3 everywhere (no L1 sign in doubt), posterior moments, per-sample weights; float64 on the host"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    d = (1e-3 + 0.3 * torch.rand(2, 3, 32, 32, generator=g)) * torch.where(torch.rand(2, 3, 32, 32, generator=g) < 0.5, -1.0, 1.0)
    xr = x + d
    assert ((xr - x).abs() >= 1e-3 * (1 - 1e-3)).all()
    moments = torch.randn(2, 8, 16, 16, generator=g) * 0.5
    return x, xr, moments, torch.tensor([0.5, 1.75])


def evaluate(loss_mod, dist_cls, x, xr, moments, optimizer_idx, global_step, weights, dtype, device, **kw):
    """One loss evaluation on leaf tensors.  The reconstruction is leaf * gain with gain = 1 (exactly the leaf's values): `gain` [3] stands in
    for the decoder's last layer, so the adaptive weight has something to differentiate to.  Returns total, log, gradients."""
    for p in loss_mod.discriminator.parameters():
        p.requires_grad_(optimizer_idx == 1)       # what the trainer's optimizer toggle does
    leaf = xr.to(device=device, dtype=dtype).requires_grad_()
    gain = torch.ones(3, device=device, dtype=dtype, requires_grad=True)
    mom = moments.to(device=device, dtype=dtype).requires_grad_()
    rec = leaf * gain.view(1, 3, 1, 1)
    w = None if weights is None else weights.to(device=device, dtype=dtype)
    loss_mod.zero_grad(set_to_none=True)
    total, log = loss_mod(x.to(device=device, dtype=dtype), rec, dist_cls(mom), optimizer_idx, global_step, last_layer=gain, weights=w, **kw)
    grads = {}
    if total.requires_grad:
        total.backward()
        grads = {"reconstruction": leaf.grad, "moments": mom.grad, "logvar": loss_mod.logvar.grad}
        grads.update({"D." + n: p.grad for n, p in loss_mod.discriminator.named_parameters()})
        grads = {k: v for k, v in grads.items() if v is not None}
    return total.detach(), log, grads


@pytest.mark.parametrize("disc_factor", [1.0, 0.0], ids=["disc-on", "disc-off"])
@pytest.mark.parametrize("perceptual_weight", [1.0, 0.0], ids=["lpips", "l1-only"])
@pytest.mark.parametrize("disc_loss", ["hinge", "vanilla"])
def test_loss_forward_matches_the_restatement(hip_lib, disc_loss, perceptual_weight, disc_factor):
    """optimizer_idx 0 and 1, global_step on both sides of disc_start, weights None and per sample, train and eval: every logged value,
    the total and the gradients at the reconstruction, logvar, the posterior moments and the discriminator's parameters"""
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    from oracle.distributions import DiagonalGaussianDistribution as DGRef
    ctx = quiet()
    loss, ref = loss_pair(disc_loss, perceptual_weight, disc_factor)
    loss.log_exact_g_loss = True          # log -mean D(x_rec) with the discriminator off too, as upstream does
    x, xr, moments, per_sample = loss_tensors()
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    worst = Worst("loss %s pw=%g df=%g" % (disc_loss, perceptual_weight, disc_factor))
    seen_keys = set()
    for training in (True, False):
        for optimizer_idx in (0, 1):
            for global_step in (9, 10):
                for weights in ((None, per_sample) if optimizer_idx == 0 else (None,)):
                    where = "%s opt%d step%d%s" % ("train" if training else "eval", optimizer_idx, global_step, "" if weights is None else " weighted")
                    loss.train(training); ref.train(training)
                    loss.discriminator.load_state_dict(d_state)           # BatchNorm's running statistics move in training: same start
                    ref.discriminator.load_state_dict(d_state)
                    got = evaluate(loss, DG, x, xr, moments, optimizer_idx, global_step, weights, torch.float32, DEV)
                    want = evaluate(ref, DGRef, x, xr, moments, optimizer_idx, global_step, weights, torch.float64, "cpu")
                    worst("out total", rel(got[0], want[0]), where)
                    assert set(got[1]) == set(want[1]), where
                    seen_keys |= set(got[1])
                    for k in want[1]:
                        assert torch.as_tensor(got[1][k]).numel() == 1, k
                        e = abs(float(got[1][k]) - float(want[1][k])) / max(1.0, abs(float(want[1][k])))
                        worst("out " + k.split("/")[1], e, where)
                    assert set(got[2]) == set(want[2]), (where, sorted(set(got[2]) ^ set(want[2])))
                    if want[2]:
                        for group in ("reconstruction", "moments", "logvar", "D."):
                            names = [k for k in want[2] if k.startswith(group)]
                            if not names:
                                continue
                            scale = max(want[2][k].abs().max().item() for k in names)
                            for k in names:
                                worst("grad " + group.rstrip("."), grad_rel(got[2][k], want[2][k], scale), where + " " + k)
                    if optimizer_idx == 0:
                        assert "reconstruction" in want[2] and want[2]["reconstruction"].abs().max() > 0 and "logvar" in want[2]
                        assert float(want[1]["train/disc_factor"]) == (disc_factor if global_step >= 10 else 0.0)
                        assert (float(want[1]["train/d_weight"]) > 0) == (disc_factor > 0)
                    elif disc_factor > 0 and global_step >= 10:
                        assert any(k.startswith("D.") and v.abs().max() > 0 for k, v in want[2].items()), where
                        assert "reconstruction" not in want[2]
    assert seen_keys == {"train/" + k for k in ("total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss",
                                                "disc_loss", "logits_real", "logits_fake")}
    ctx.__exit__(None, None, None)
    worst.check({"out": TOL_LOSS_OUT, "grad reconstruction": TOL_LOSS_GRAD, "grad moments": TOL_LOSS_GRAD, "grad logvar": TOL_LOSS_GRAD,
                 "grad D": TOL_LOSS_GRAD_D})
    assert {k.split()[0] + " " + k.split()[1] for k in worst.v if k.startswith("grad")} <= {"grad reconstruction", "grad moments", "grad logvar", "grad D"}


def test_disc_off_shortcut_logs_zero_and_changes_nothing_else(hip_lib):
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    ctx = quiet()
    loss, _ = loss_pair(disc_factor=0.0)
    x, xr, moments, _ = loss_tensors()
    loss.train()
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    assert loss.log_exact_g_loss is False
    short = evaluate(loss, DG, x, xr, moments, 0, 10, None, torch.float32, DEV)
    assert all(torch.equal(v, d_state[k].to(DEV)) for k, v in loss.discriminator.state_dict().items())       # D did not run
    loss.log_exact_g_loss = True
    exact = evaluate(loss, DG, x, xr, moments, 0, 10, None, torch.float32, DEV)
    assert not torch.equal(loss.discriminator.state_dict()["main.3.running_mean"], d_state["main.3.running_mean"].to(DEV))
    assert float(short[1]["train/g_loss"]) == 0.0 and float(exact[1]["train/g_loss"]) != 0.0
    assert torch.equal(short[0], exact[0])
    for k in exact[1]:
        if k != "train/g_loss":
            assert torch.equal(torch.as_tensor(short[1][k]).cpu(), torch.as_tensor(exact[1][k]).cpu()), k
    assert set(short[2]) == set(exact[2]) and all(torch.equal(short[2][k], exact[2][k]) for k in exact[2])
    ctx.__exit__(None, None, None)


def test_one_pass_adaptive_weight_equals_the_three_pass_form(hip_lib):
    """The same d_weight and g_loss to f32 rounding, and the same gradients to summation order: both forms run the same kernels on the
    same values; the one-pass form adds d nll / d x_rec and d_weight d g / d x_rec before, not after, the reconstruction's own backward."""
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    ctx = quiet()
    loss, _ = loss_pair()
    loss.train()
    x, xr, moments, _ = loss_tensors()
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    out = {}
    for one_pass in (True, False):
        loss.ONE_PASS = one_pass
        loss.discriminator.load_state_dict(d_state)
        out[one_pass] = evaluate(loss, DG, x, xr, moments, 0, 10, None, torch.float32, DEV)
    del loss.ONE_PASS
    assert type(loss).ONE_PASS is True, "this run has ODVAE_ADAPTIVE_WEIGHT_ONE_PASS=0: both evaluations above took the three passes"
    a, b = out[True], out[False]
    worst = Worst("one pass vs three passes")
    worst("total", rel(a[0], b[0]))
    for k in b[1]:
        worst(k, abs(float(a[1][k]) - float(b[1][k])) / max(1.0, abs(float(b[1][k]))))
    assert set(a[2]) == set(b[2]) == {"reconstruction", "moments", "logvar"}
    for k in b[2]:
        worst("grad " + k, rel(a[2][k], b[2][k]))
    ctx.__exit__(None, None, None)
    worst.check({"": TOL_ONE_PASS})


def test_loss_refuses_what_it_cannot_do(hip_lib):
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    ctx = quiet()
    loss, _ = loss_pair(perceptual_weight=0.0)
    x, xr, moments, per_sample = loss_tensors()
    with pytest.raises(NotImplementedError, match="per-pixel"):
        evaluate(loss, DG, x, xr, moments, 0, 10, torch.ones(2, 1, 32, 32), torch.float32, DEV)
    for idx in (0, 1):
        with pytest.raises(AssertionError):
            evaluate(loss, DG, x, xr, moments, idx, 10, None, torch.float32, DEV, cond=x.to(DEV))
    # a scalar and the [N, 1, 1, 1] form of the per-sample weights
    base = evaluate(loss, DG, x, xr, moments, 0, 10, per_sample, torch.float32, DEV)
    again = evaluate(loss, DG, x, xr, moments, 0, 10, per_sample.reshape(2, 1, 1, 1), torch.float32, DEV)
    assert torch.equal(base[0], again[0])
    two = evaluate(loss, DG, x, xr, moments, 0, 10, torch.tensor(2.0), torch.float32, DEV)
    one = evaluate(loss, DG, x, xr, moments, 0, 10, None, torch.float32, DEV)
    assert float(two[1]["train/nll_loss"]) == float(one[1]["train/nll_loss"]) and two[0] > one[0]
    assert loss(x.to(DEV), xr.to(DEV), DG(moments.to(DEV)), 2, 10) is None
    ctx.__exit__(None, None, None)


def test_plain_loss_is_poseloss_with_the_pose_terms_off(hip_lib):
    """PoseLoss (pinned to the reference by tests/test_reference_glue*.py and the oracle tests) with every pose weight 0, kl_weight_bbox 0,
    no pretraining phases, no mask, no sample of class id 1 and logvar = 0 (where its +1e-8 vanishes in f32) is the plain loss."""
    from odvae_amd import synthetic
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    from odvae_amd.losses import PoseLoss
    ctx = quiet()
    plain, _ = loss_pair(disc_start=0)
    with torch.no_grad():
        plain.logvar.zero_()
    pose = PoseLoss(disc_start=0, kl_weight_obj=0.3, kl_weight_bbox=0.0, pose_weight=0.0, mask_weight=0.0, class_weight=0.0, bbox_weight=0.0,
                    fill_factor_weight=0.0, pose_loss_fn="l1", mask_loss_fn="l2", encoder_pretrain_steps=0, pose_conditioned_generation_steps=0,
                    num_classes=11, dataset_stats=synthetic.dataset_stats_standin(), disc_weight=0.5, perceptual_weight=1.0, disc_factor=1.0).to(DEV)
    pose.load_state_dict(plain.state_dict(), strict=True)
    plain.train(); pose.train()
    x, xr, moments, _ = loss_tensors()
    g = torch.Generator().manual_seed(3)
    dec_pose = torch.randn(2, 8 + 11, generator=g).to(DEV)
    bbox_post = DG(torch.randn(2, 16, generator=g).to(DEV) * 0.1)
    class_gt, labels = torch.zeros(2, dtype=torch.int64), ["car", "car"]
    d_state = {k: v.clone() for k, v in plain.discriminator.state_dict().items()}

    def run(which):
        mod = plain if which == "plain" else pose
        mod.discriminator.load_state_dict(d_state)
        for p in mod.discriminator.parameters():
            p.requires_grad_(False)
        leaf = xr.to(DEV).requires_grad_()
        gain = torch.ones(3, device=DEV, requires_grad=True)
        mom = moments.to(DEV).requires_grad_()
        rec = leaf * gain.view(1, 3, 1, 1)
        mod.zero_grad(set_to_none=True)
        if which == "plain":
            total, log = mod(x.to(DEV), rec, DG(mom), 0, 1, last_layer=gain)
        else:
            total, log = mod(x.to(DEV), None, torch.randn(2, 4, generator=torch.Generator().manual_seed(4)).to(DEV), rec, dec_pose, class_gt,
                             labels, torch.randn(2, 3, generator=torch.Generator().manual_seed(5)).to(DEV), torch.rand(2).to(DEV), DG(mom),
                             bbox_post, 0, 1, None, last_layer=gain)
        total.backward()
        return total.detach(), log, {"reconstruction": leaf.grad, "moments": mom.grad, "logvar": mod.logvar.grad}
    a, b = run("plain"), run("pose")
    worst = Worst("plain loss vs PoseLoss with the pose terms off")
    worst("total", rel(a[0], b[0]))
    for ka, kb in (("nll_loss", "nll_loss"), ("kl_loss", "kl_loss_obj"), ("rec_loss", "rec_loss"), ("g_loss", "g_loss"), ("d_weight", "d_weight")):
        worst(ka, abs(float(a[1]["train/" + ka]) - float(b[1]["train/" + kb])) / max(1.0, abs(float(b[1]["train/" + kb]))))
    assert float(b[1]["train/d_weight"]) > 0 and float(b[1]["train/disc_factor"]) == 1.0 and float(b[1]["train/g_loss"]) != 0.0
    for k in b[2]:
        worst("grad " + k, rel(a[2][k], b[2][k]))
    ctx.__exit__(None, None, None)
    worst.check({"": TOL_CROSS})


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
def build_pair(zc=4, overrides=(), seed=23, dtype=torch.float64):
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    dots = SMALL + ["model.params.ddconfig.z_channels=%d" % zc, "model.params.embed_dim=%d" % zc,
                    "model.params.lossconfig.params.disc_start=0", "model.params.lossconfig.params.kl_weight=0.01"] + list(overrides)
    config = Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(dots))
    model = instantiate_from_config(config.model)
    synthetic.fill_state_procedural(model, seed=seed)
    liven_discriminator(model.loss.discriminator)
    model.learning_rate = 2 * config.model.base_learning_rate
    p = config.model.params.to_container()
    ref = R.PlainAutoencoder(p["ddconfig"], p["lossconfig"]["params"], p["embed_dim"]).to(dtype)
    res = ref.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ref.learning_rate = model.learning_rate
    return model.to(DEV), ref


def make_noise(zc, seed):
    g = torch.Generator().manual_seed(seed)
    return {"posterior_eps": torch.randn(2, zc, 16, 16, generator=g), "samples_eps": torch.randn(2, zc, 16, 16, generator=g)}


def compare_param_grads(worst, model, ref, where):
    ref_params = dict(ref.named_parameters())
    with_grad = [p.grad for p in ref_params.values() if p.grad is not None]
    scale = max(g.abs().max().item() for g in with_grad)
    compared = set()
    for name, p in model.named_parameters():
        rg = ref_params[name].grad
        if rg is None or p.grad is None:
            assert (rg is None or rg.abs().max().item() == 0.0) and (p.grad is None or p.grad.abs().max().item() == 0.0), name
            continue
        compared.add(name.split(".")[0] if not name.startswith("loss.") else ".".join(name.split(".")[:2]))
        worst("grad " + name.split(".")[0], grad_rel(p.grad, rg, scale), where + " " + name)
    return compared


@pytest.mark.parametrize("zc", [4, 3], ids=["z4", "kl-f4-z3"])
def test_training_step_matches_the_restatement(hip_lib, zc):
    from odvae_amd import synthetic
    ctx = quiet()
    model, ref = build_pair(zc)
    model.train(); ref.train()
    batch = synthetic.make_image_batch(2, 32, seed=5)
    noise = make_noise(zc, 6)
    model.injected_noise = noise
    model._global_step = ref.global_step = 1
    worst = Worst("training_step z=%d" % zc)
    d_state = {k: v.clone() for k, v in model.loss.discriminator.state_dict().items()}
    for optimizer_idx in (0, 1):
        model.loss.discriminator.load_state_dict(d_state); ref.loss.discriminator.load_state_dict(d_state)
        for m in (model, ref):       # the optimizer toggle: the discriminator's parameters belong to optimizer 1, logvar to neither
            for n, p in m.named_parameters():
                if not n.startswith("loss.perceptual_loss"):
                    p.requires_grad_(n.startswith("loss.discriminator") == (optimizer_idx == 1) and n != "loss.logvar")
            m.zero_grad(set_to_none=True)
        loss = model.training_step(dict(batch), 0, optimizer_idx)
        loss_ref, log_ref, aux = ref.training_step(batch, optimizer_idx, noise)
        logs = dict(model.logged_metrics)
        where = "opt%d" % optimizer_idx
        worst("out total", rel(loss, loss_ref), where)
        assert float(logs["aeloss" if optimizer_idx == 0 else "discloss"]) == loss.item()
        for k in log_ref:
            worst("out " + k.split("/")[1], abs(float(logs[k]) - float(log_ref[k])) / max(1.0, abs(float(log_ref[k]))), where)
        if optimizer_idx == 0:
            with torch.no_grad():
                xrec, post = model(model.get_input(batch, "image"))
            # precondition of the gradient bound: no L1 sign in doubt -- sign(x_rec - x) is the restatement's at every pixel of this batch
            # (the nearest |x_rec - x| is printed; a flipped sign would move every gradient behind it, tests/test_model_gpu.py)
            diff_ref = aux["reconstructions"] - aux["inputs"]
            flips = (torch.sign(xrec.cpu().double() - aux["inputs"]) != torch.sign(diff_ref)).sum().item()
            print("z=%d: nearest |x_rec - x| %.3e of max|x_rec| %.3e, L1 sign flips %d" % (zc, diff_ref.abs().min().item(),
                                                                                         aux["reconstructions"].abs().max().item(), flips))
            assert flips == 0
            worst("out reconstruction", rel(xrec, aux["reconstructions"]), where)
            worst("out moments", rel(post.parameters, aux["posterior"].parameters), where)
            assert post.parameters.shape == (2, 2 * zc, 16, 16) and float(log_ref["train/d_weight"]) > 0
        loss.backward(); loss_ref.backward()
        compared = compare_param_grads(worst, model, ref, where)
        assert compared == ({"encoder", "decoder", "quant_conv", "post_quant_conv"} if optimizer_idx == 0 else {"loss.discriminator"}), compared
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT, grad=TOL_MODEL_GRAD)


def test_three_training_batches_match_the_restatement_under_adam(hip_lib):
    """Three batches of Trainer.training_batch (two optimizers, clip 1.0) against the same loop on the restatement with torch.optim.Adam.
    The reconstruction term is an L1: a sign(x_rec - x) that flips at a pixel whose |x_rec - x| is below the forward's deviation moves every
    gradient behind it, so the weights are held as tests/test_model_gpu.py holds them after Adam steps (2.2 lr per step, a gradient that is zero
    up to rounding may move a weight either way, + 5e-3 of the tensor's largest entry) and the six losses to TOL_CURVE."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, ref = build_pair(4)
    model.train(); ref.train()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
    ref_opts = ref.configure_optimizers()
    worst = Worst("three batches")
    for step in range(3):
        batch = synthetic.make_image_batch(2, 32, seed=300 + step)
        noises = {0: make_noise(4, 400 + 2 * step), 1: make_noise(4, 401 + 2 * step)}
        got = []
        for idx in (0, 1):       # one optimizer at a time so that each forward sees its own injected noise
            model.injected_noise = noises[idx]
            trainer.optimizer_indices = (idx,)
            got.append(trainer.training_batch(dict(batch), step)[0])
        out = R.train_batch(ref, ref_opts, batch, noises, clip=1.0)
        for idx in (0, 1):
            worst("loss", rel(got[idx], out[idx][0]), "batch %d opt%d" % (step, idx))
    assert model.global_step == 6 and ref.global_step == 6
    ref_sd = ref.state_dict()
    lr, steps = model.learning_rate, 3
    moved = 0
    for k, v in model.state_dict().items():
        if v.dtype == torch.float32 and k.startswith(("encoder", "decoder", "quant", "post_quant", "loss.discriminator")):
            diff = (v.detach().cpu().double() - ref_sd[k]).abs().max().item()
            assert diff <= 2.2 * lr * steps + 5e-3 * ref_sd[k].abs().max().item(), (k, diff)
            moved += 1
    assert moved > 50 and float(model.state_dict()["loss.logvar"]) == 0.0          # logvar is in neither optimizer
    ctx.__exit__(None, None, None)
    worst.check(loss=TOL_CURVE)


def test_validate_yields_the_eleven_val_keys(hip_lib):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, ref = build_pair(4)
    model.train(); ref.eval()
    model.loss.log_exact_g_loss = True
    batch = synthetic.make_image_batch(2, 32, seed=11)
    noise = make_noise(4, 12)
    model.injected_noise = noise
    trainer = Trainer(model, gradient_clip_val=1.0)
    metrics = trainer.validate([dict(batch)])
    assert model.training and trainer.callback_metrics["val/rec_loss"] == metrics["val/rec_loss"]
    with torch.no_grad():
        want = ref.validation_step(batch, noise)
    assert set(metrics) == set(want) == {"val/" + k for k in ("total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor",
                                                                  "g_loss", "disc_loss", "logits_real", "logits_fake")}
    assert float(want["val/d_weight"]) == 0.0        # no graph under no_grad: RuntimeError -> 0 outside training, on both sides
    worst = Worst("validate")
    for k in want:
        worst("out " + k.split("/")[1], abs(float(metrics[k]) - float(want[k])) / max(1.0, abs(float(want[k]))))
    assert model.validation_step(dict(batch), 0) == model.log_dict
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT)


def test_log_images_and_image_logger(hip_lib, tmp_path):
    from odvae_amd import synthetic
    from odvae_amd.callbacks import ImageLogger
    ctx = quiet()
    model, ref = build_pair(4)
    model.eval(); ref.eval()
    batch = synthetic.make_image_batch(2, 32, seed=21)
    noise = make_noise(4, 22)
    model.injected_noise = noise
    got, want = model.log_images(dict(batch)), ref.log_images(batch, noise)
    assert set(got) == set(want) == {"inputs", "reconstructions", "samples"}
    worst = Worst("log_images")
    for k in want:
        assert got[k].shape == (2, 3, 32, 32) and got[k].is_cuda and not got[k].requires_grad, k
        worst("out " + k, rel(got[k], want[k]))
    assert torch.equal(got["inputs"].cpu(), batch["image"].permute(0, 3, 1, 2))
    only = model.log_images(dict(batch), only_inputs=True)
    assert list(only) == ["inputs"] and torch.equal(only["inputs"], got["inputs"])
    # without the hook the draws are the host generator's: seeded the same, the same pictures
    model.injected_noise = None
    torch.manual_seed(7)
    a = model.log_images(dict(batch))
    torch.manual_seed(7)
    b = model.log_images(dict(batch))
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["samples"], got["samples"])
    # forward(sample_posterior=False) decodes the mode
    with torch.no_grad():
        xm, post = model(got["inputs"], sample_posterior=False)
        assert torch.equal(xm, model.decode(post.mode()))

    class _Logger:
        save_dir = str(tmp_path)
    model.logger = _Logger()
    model._global_step = 1
    model.train()
    written = ImageLogger(batch_frequency=1, max_images=2).log_img(model, dict(batch), 0, split="train")
    assert model.training
    assert sorted(os.path.basename(p).split("_gs-")[0] for p in written) == ["inputs", "reconstructions", "samples"]
    from PIL import Image
    for p in written:
        assert os.path.dirname(p) == str(tmp_path / "images" / "train") and Image.open(p).size == (2 * 32 + 3 * 2, 32 + 2 * 2), p      # two 32 x 32 images, padding 2
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT)


def test_checkpoint_round_trip_and_init_from_ckpt(hip_lib, tmp_path):
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, _ = build_pair(4)
    model.train()
    trainer = Trainer(model, gradient_clip_val=1.0)
    batch = synthetic.make_image_batch(2, 32, seed=31)
    model.injected_noise = make_noise(4, 32)
    trainer.training_batch(dict(batch), 0)
    path = trainer.save_checkpoint(str(tmp_path / "plain.ckpt"))
    after_one = [l.clone() for l in trainer.training_batch(dict(batch), 1)]
    sd_two = {k: v.clone() for k, v in model.state_dict().items()}

    other, _ = build_pair(4, seed=99)
    other.train()
    other.injected_noise = make_noise(4, 32)
    resumed = Trainer(other, gradient_clip_val=1.0)
    res = resumed.load_checkpoint(path)
    assert not res.missing_keys and not res.unexpected_keys and other.global_step == 2
    again = resumed.training_batch(dict(batch), 1)
    assert all(torch.equal(a, b) for a, b in zip(after_one, again))              # weights, optimizer moments and step counts all came back
    assert all(torch.equal(v, sd_two[k]) for k, v in other.state_dict().items())

    # a CompVis-layout checkpoint without the loss: ckpt_path + ignore_keys=["loss"] restores the autoencoder and leaves the loss as built
    dots = SMALL + ["model.params.ddconfig.z_channels=4", "model.params.embed_dim=4", "model.params.ckpt_path=%s" % path,
                    "model.params.ignore_keys=[loss]"]
    fresh = instantiate_from_config(Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(dots)).model)
    saved = torch.load(path, map_location="cpu")["state_dict"]
    fresh_sd = fresh.state_dict()
    assert set(fresh_sd) == set(saved)
    for k, v in saved.items():
        if k.startswith("loss.discriminator.") and v.is_floating_point() and v.dim() == 4:
            assert not torch.equal(fresh_sd[k], v), k
        elif not k.startswith("loss."):
            assert torch.equal(fresh_sd[k], v), k
    ctx.__exit__(None, None, None)


def test_bf16_step_is_as_close_to_f32_as_autocast(hip_lib):
    """`precision: bf16` on the plain model, held as tests/test_bf16_model_gpu.py holds the pose model: no further from the f32 restatement
    than twice the restatement under CPU autocast is, plus that test's floors (2e-2 tensors, 1e-2 scalars), the gradient cosine, and per
    tensor holding >= 1e-3 of the gradient energy err <= 2 * err_autocast + 5e-2.  z_channels = 4
    is no multiple of 8: the latent enters decoder.conv_in in f32 (modules.Decoder.forward)."""
    from odvae_amd import synthetic
    ctx = quiet()
    model, ref = build_pair(4, dtype=torch.float32)
    model.set_precision("bf16")
    assert model.encoder.compute_dtype == torch.bfloat16
    model.train(); ref.train()
    model._global_step = ref.global_step = 1
    batch = synthetic.make_image_batch(2, 32, seed=5)
    noise = make_noise(4, 6)
    d_state = {k: v.clone() for k, v in ref.loss.discriminator.state_dict().items()}
    for m in (model, ref):
        for n, p in m.named_parameters():
            p.requires_grad_(not n.startswith("loss."))

    def run_ref(autocast):
        ref.loss.discriminator.load_state_dict(d_state)
        ref.zero_grad(set_to_none=True)
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                loss, log, aux = ref.training_step(batch, 0, noise)
        else:
            loss, log, aux = ref.training_step(batch, 0, noise)
        loss.backward()
        grads = {k: p.grad.detach().clone().float() for k, p in ref.named_parameters() if p.grad is not None}
        return loss.detach().float(), {k: float(v) for k, v in log.items()}, aux, grads
    l32, log32, aux32, g32 = run_ref(False)
    lac, logac, auxac, gac = run_ref(True)
    model.injected_noise = noise
    loss = model.training_step(dict(batch), 0, 0)
    logs = dict(model.logged_metrics)
    loss.backward()
    with torch.no_grad():
        xrec, post = model(model.get_input(batch, "image"))
    assert xrec.dtype == torch.float32 and post.parameters.dtype == torch.float32
    report = []

    def check(name, got, want, ac, floor):
        e, eac = rel(got.float(), want.float()), rel(ac.float(), want.float())
        report.append("%s: hip %.3e autocast %.3e" % (name, e, eac))
        assert e <= 2 * eac + floor, "%s: bf16 HIP path %.3e from the f32 restatement, autocast %.3e (floor %.0e)" % (name, e, eac, floor)
    check("moments", post.parameters, aux32["posterior"].parameters, auxac["posterior"].parameters, 2e-2)
    check("reconstruction", xrec, aux32["reconstructions"], auxac["reconstructions"], 2e-2)
    check("total loss", loss, l32, lac, 1e-2)
    for key in ("kl_loss", "nll_loss", "rec_loss"):      # (not g_loss: a mean of signed logits near zero has no scale of its own to be relative to)
        check(key, torch.as_tensor(float(logs["train/" + key])), torch.as_tensor(log32["train/" + key]), torch.as_tensor(logac["train/" + key]), 1e-2)
    params = dict(model.named_parameters())
    keys = [k for k in g32 if params[k].grad is not None]
    assert {k.split(".")[0] for k in keys} == {"encoder", "decoder", "quant_conv", "post_quant_conv"}
    flat = lambda g: torch.cat([g[k].flatten().double() for k in keys])
    for k in keys:
        assert params[k].grad.dtype == torch.float32 and torch.isfinite(params[k].grad).all(), k
    ghip = {k: params[k].grad.detach().cpu().float() for k in keys}
    v32, vhip, vac = flat(g32), flat(ghip), flat(gac)
    cos = lambda a, b: (a @ b / (a.norm() * b.norm())).item()
    report.append("gradient cosine: hip %.5f autocast %.5f" % (cos(vhip, v32), cos(vac, v32)))
    assert cos(vhip, v32) >= min(0.98, cos(vac, v32) - 0.01), report[-1]
    energy = v32.pow(2).sum().item()
    judged, worst_tensor = 0, ("", 0.0, 0.0)
    for k in keys:
        if g32[k].double().pow(2).sum().item() < 1e-3 * energy:
            continue
        judged += 1
        e, eac = rel(ghip[k], g32[k]), rel(gac[k], g32[k])
        if e - 2 * eac > worst_tensor[1] - 2 * worst_tensor[2] or not worst_tensor[0]:
            worst_tensor = (k, e, eac)
        assert e <= 2 * eac + 5e-2, "grad %s: hip %.3e autocast %.3e" % (k, e, eac)
    report.append("per-tensor gradients: %d tensors judged, nearest to its bound %s hip %.3e autocast %.3e" % ((judged,) + worst_tensor))
    report.append("conv_in / quant convs: " + ", ".join("%s hip %.3e autocast %.3e" % (k, rel(ghip[k], g32[k]), rel(gac[k], g32[k]))
                                                         for k in ("decoder.conv_in.weight", "post_quant_conv.weight", "quant_conv.weight")))
    print("; ".join(report))
    assert judged > 0
    ctx.__exit__(None, None, None)


def test_launcher_trains_the_plain_yaml(hip_lib, capsys):
    from odvae_amd import autoencoder, run
    ctx = quiet()
    model = run.main(["-b", PLAIN_YAML, "--height", "32", "--steps", "2", "data.params.batch_size=2",
                      "model.params.lossconfig.params.disc_start=0"] + SMALL)
    ctx.__exit__(None, None, None)
    assert type(model) is autoencoder.Autoencoder and model.global_step == 4
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("batch ")]
    assert len(lines) == 2
    for line in lines:
        words = line.split()
        ae, disc = float(words[words.index("aeloss") + 1]), float(words[words.index("discloss") + 1])
        assert ae == ae and disc == disc and abs(ae) < float("inf") and abs(disc) < float("inf"), line
    assert all(torch.isfinite(v).all() for k, v in model.logged_metrics.items() if torch.is_tensor(v))
    assert model.decoder.conv_out.weight.grad is None or torch.isfinite(model.decoder.conv_out.weight.grad).all()
