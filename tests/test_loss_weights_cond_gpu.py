"""`weights` and `cond` on the device: PoseLoss against what the REFERENCE's PoseLoss.forward returned and logged with those arguments
(tests/golden/reference_weights_cond.npz, written by tests/golden/make_reference_weights_cond_goldens.py), the plain loss against the
float64 restatement of upstream's forward (tests/loss_weights_ref.WeightedPlainLoss), the input checks, a width-reduced PoseAutoencoder
with cond_key / loss_weights_key through Trainer steps in f32 and under precision: bf16, the launcher, the checkpoint of the 5-channel
discriminator, and -- with neither argument given -- the same bits as before they were honoured.

Tolerances against the fixture (relative, as tests/test_image_mask_gpu.py takes them: scalars to |expected| + 1e-6, the gradient to its
norm).  The fixture is the reference evaluated in float64, so the distance is the device path's own f32 rounding; measured worst on an
MI355X over all cases (profiles/loss_weights_cond.md): scalars 6.75e-7 (reached by the case with neither argument already), gradient norm
1.82e-7, gradient samples 1.18e-7.  The bounds are the smaller of 4 x those and tests/test_image_mask_gpu.py's for the same keys (9.0e-7,
5.5e-7, 2.0e-7) -- which is the latter, three times.  The plain loss (cond, and the scalar / per-sample weights it always took) is bounded
the same way against tests/test_plain_vae_gpu.py's constants: measured 2.78e-7 (outputs), 9.96e-7 (gradient at the reconstruction) and
6.78e-6 (discriminator parameters), so 4 x the measured figure is the smaller one each time (the constants beside TOL_PLAIN_*)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path[:0] = [HERE, GOLD]
import loss_weights_ref as R  # noqa: E402
from reference_cases import LABELS, LOSS_KW, digest_of, stats_table  # noqa: E402

YAML = os.path.join(GOLD, "autoencoder_kl_16x16x16.yaml")
CLASS_IDS = [0, 1, 3, 0]
STEPS = (5, 12, 20, 40)
WEIGHT_KINDS = ("none", "scalar", "sample", "pixel", "element", "shared")
SCALAR_TOL, GRAD_NORM_TOL, GRAD_SAMPLE_TOL = 9.0e-7, 5.5e-7, 2.0e-7
# the plain loss: min(4 x the worst measured here, the constant of tests/test_plain_vae_gpu.py for the same quantity)
TOL_PLAIN_OUT = 1.11e-6        # measured 2.78e-7 (mean of the real logits); TOL_LOSS_OUT there 1.2e-6
TOL_PLAIN_GRAD = 3.98e-6       # measured 9.96e-7 (gradient at the reconstruction; moments 1.5e-7, logvar 8.2e-8); TOL_LOSS_GRAD there 4.1e-6
TOL_PLAIN_GRAD_D = 2.71e-5     # measured 6.78e-6 (a discriminator BatchNorm scale); TOL_LOSS_GRAD_D there 2.8e-5
TOL_ONE_PASS = 3.4e-6          # measured 9.24e-7 under cond (4 x that is 3.7e-6); TOL_ONE_PASS there 3.4e-6
WORST = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "reference_weights_cond.npz"))


@pytest.fixture(scope="module")
def inputs(gold):
    return {k[3:]: torch.from_numpy(gold[k]).to(DEV) for k in gold.files if k.startswith("in.") and k != "in.global_steps"}


def weights_of(d, kind):
    return {"none": None, "scalar": 0.5, "sample": d["w_sample"], "pixel": d["w_pixel"], "element": d["w_element"], "shared": d["w_shared"]}[kind]


def product_loss(**kw):
    from odvae_amd.losses import PoseLoss
    from odvae_amd.synthetic import fill_state_procedural
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = PoseLoss(dataset_stats=stats_table(), **dict(LOSS_KW, **kw))
    fill_state_procedural(loss, seed=31)
    with torch.no_grad():
        loss.logvar.fill_(0.3)
    return loss.to(DEV).train()


def call(loss, d, opt, gs, weights=None, cond=None, rgba=False):
    """One PoseLoss.forward on the fixture's inputs with dec_obj = conv3x3(feat) of a stand-in conv_out; (ret, dec_obj)."""
    from odvae_amd import modules
    from odvae_amd.distributions import DiagonalGaussianDistribution as D
    from odvae_amd.synthetic import fill_state_procedural
    last = modules.Conv3x3(8, 4 if rgba else 3).to(DEV)
    with torch.no_grad():
        last.weight.copy_(d["last_w4" if rgba else "last_w"])
        last.bias.copy_(d["last_b4" if rgba else "last_b"])
        fill_state_procedural(loss.discriminator, seed=31)
    dec_obj = last(d["feat"].clone().requires_grad_(True))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ret = loss(d["rgb_gt"], d["mask_gt"] if rgba else None, d["pose_gt"], dec_obj, d["dec_pose"].clone().requires_grad_(True), d["class_id"],
                   [LABELS[c] for c in CLASS_IDS], d["bbox_gt"], d["fill_factor_gt"], D(d["moments"].clone().requires_grad_(True)),
                   D(d["bbox_moments"].clone().requires_grad_(True)), opt, gs, d["mask_2d_bbox"], last_layer=last.weight, cond=cond, split="train",
                   weights=weights)
    return ret, dec_obj


def check_case(gold, pre, ret, dec_obj):
    out, log = ret
    assert out.dim() == 0

    def scalar(key, got, want):
        e = abs(float(torch.as_tensor(got).detach()) - float(want)) / (abs(float(want)) + 1e-6)
        WORST["scalar"] = max(WORST.get("scalar", 0.0), e)
        assert e <= SCALAR_TOL, "%s %s: %.8g vs %.8g (rel %.2e)" % (pre, key, float(got), float(want), e)

    scalar("loss", out, gold[pre + ".loss"])
    keys = [f[len(pre + ".log."):] for f in gold.files if f.startswith(pre + ".log.")]
    assert sorted(keys) == sorted(log.keys())
    for k in keys:
        scalar(k, log[k], gold[pre + ".log." + k])
    if pre + ".grad.dec_obj.norm" in gold.files:
        dec_obj.retain_grad()      # only now: the adaptive weight's own autograd.grad calls would be accumulated into .grad too
        out.backward()
        gn = float(gold[pre + ".grad.dec_obj.norm"])
        norm, samples = digest_of(dec_obj.grad, limit=1024, keep=512)
        e1 = abs(float(norm) - gn) / gn
        e2 = float(np.abs(samples.astype(np.float64) - gold[pre + ".grad.dec_obj.samples"]).max()) / gn
        WORST["grad.norm"] = max(WORST.get("grad.norm", 0.0), e1)
        WORST["grad.sample"] = max(WORST.get("grad.sample", 0.0), e2)
        assert e1 <= GRAD_NORM_TOL and e2 <= GRAD_SAMPLE_TOL, "%s grad: norm %.8g vs %.8g (%.2e), samples %.2e" % (pre, norm, gn, e1, e2)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (reading .grad of a non-leaf tensor warns; it is None, which is the point)
            assert not out.requires_grad or dec_obj.grad is None


@pytest.mark.parametrize("with_cond", [False, True], ids=["no-cond", "cond"])
@pytest.mark.parametrize("kind", WEIGHT_KINDS)
def test_pose_loss_matches_the_reference(hip_lib, gold, inputs, kind, with_cond):
    loss = product_loss(disc_conditional=True, disc_in_channels=5) if with_cond else product_loss()
    assert sorted(loss.state_dict().keys()) == list(gold["state_keys.cond%d" % with_cond])
    for gs in STEPS:
        for opt in (0, 1):
            check_case(gold, "%s.cond%d.step%d.opt%d" % (kind, with_cond, gs, opt),
                       *call(loss, inputs, opt, gs, weights_of(inputs, kind), inputs["cond"] if with_cond else None))
    print("weights/cond margins (worst relative distance to the reference):", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def test_pose_loss_rgba_with_cond_and_a_pixel_weight_matches_the_reference(hip_lib, gold, inputs):
    """image_mask_key: rgba_terms supplies the unweighted sums and the masked copies, the weighted sums come from the 4-channel
    reconstruction in place, and the discriminator sees 4 + 2 channels"""
    loss = product_loss(disc_conditional=True, disc_in_channels=6, use_mask_loss=False)
    for gs in STEPS:
        for opt in (0, 1):
            check_case(gold, "rgba.pixel.cond1.step%d.opt%d" % (gs, opt), *call(loss, inputs, opt, gs, inputs["w_pixel"], inputs["cond"], rgba=True))
    print("weights/cond margins (worst relative distance to the reference):", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def test_pose_loss_with_weights_shaped_b111_is_the_reference_value(hip_lib, gold, inputs):
    """[B,1,1,1] weights times the [B] per-sample sums used to broadcast to [B,1,1,B]; the reference multiplies on [B,3,H,W]"""
    loss = product_loss()
    w = inputs["w_sample"]
    assert tuple(w.shape) == (4, 1, 1, 1)
    (out, log), _ = call(loss, inputs, 0, 40, w)
    want = float(gold["sample.cond0.step40.opt0.log.train/weighted_nll_loss"])
    assert abs(float(log["train/weighted_nll_loss"]) - want) / abs(want) <= SCALAR_TOL
    (_, flat), _ = call(loss, inputs, 0, 40, w.reshape(4))      # the 1-D form is the same weight per sample: the same bits
    assert torch.equal(flat["train/weighted_nll_loss"], log["train/weighted_nll_loss"])
    plain = float(gold["none.cond0.step40.opt0.log.train/weighted_nll_loss"])
    assert abs(want - plain) / abs(want) > 1e-2      # (the weights do move the value)


# ---- the plain loss against the restatement --------------------------------------------------------------------------------------------
def plain_pair(cond_channels):
    import test_plain_vae_gpu as T
    from odvae_amd import synthetic
    from odvae_amd.losses import LPIPSWithDiscriminator
    kw = dict(disc_start=10, kl_weight=0.3, disc_weight=0.5, perceptual_weight=1.0, disc_factor=1.0)
    if cond_channels:
        kw.update(disc_conditional=True, disc_in_channels=3 + cond_channels)
    torch.manual_seed(11)
    loss = LPIPSWithDiscriminator(**kw)

    class Holder(torch.nn.Module):
        def __init__(self, loss):
            super().__init__()
            self.loss = loss
    synthetic.fill_state_procedural(Holder(loss), seed=23)
    T.liven_discriminator(loss.discriminator)
    with torch.no_grad():
        loss.logvar.fill_(0.25)
    ref = R.WeightedPlainLoss(**kw).double()
    ref.load_state_dict(loss.state_dict(), strict=True)
    return loss.to(DEV), ref


@pytest.mark.parametrize("cond_channels", [0, 2], ids=["no-cond", "cond"])
def test_plain_loss_matches_the_restatement(hip_lib, cond_channels):
    """optimizer_idx 0 and 1 on both sides of disc_start; weights None, a scalar, one per sample as [N] and as [N,1,1,1] (the plain forward
    takes no weight map: tests/test_plain_vae_gpu.py pins that refusal), without and with cond"""
    import test_plain_vae_gpu as T
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    from oracle.distributions import DiagonalGaussianDistribution as DGRef
    ctx = T.quiet()
    loss, ref = plain_pair(cond_channels)
    loss.train(); ref.train()
    x, xr, moments, _ = T.loss_tensors()
    g = torch.Generator().manual_seed(13)
    per_sample = 0.25 + 1.75 * torch.rand(2, generator=g)
    maps = {"none": None, "scalar": torch.tensor(0.5), "sample": per_sample, "sample4": per_sample.reshape(2, 1, 1, 1)}
    cond = torch.rand(2, cond_channels, 32, 32, generator=g) if cond_channels else None
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    worst = T.Worst("plain loss, cond channels %d" % cond_channels)
    for optimizer_idx in (0, 1):
        for global_step in (9, 10):
            for name, weights in (maps.items() if optimizer_idx == 0 else [("none", None)]):
                where = "opt%d step%d %s" % (optimizer_idx, global_step, name)
                loss.discriminator.load_state_dict(d_state)
                ref.discriminator.load_state_dict(d_state)
                got = T.evaluate(loss, DG, x, xr, moments, optimizer_idx, global_step, weights, torch.float32, DEV,
                                 **({} if cond is None else {"cond": cond}))
                want = T.evaluate(ref, DGRef, x, xr, moments, optimizer_idx, global_step, weights, torch.float64, "cpu",
                                  **({} if cond is None else {"cond": cond.double()}))
                worst("out total", T.rel(got[0], want[0]), where)
                assert set(got[1]) == set(want[1]), where
                for k in want[1]:
                    worst("out " + k.split("/")[1], abs(float(got[1][k]) - float(want[1][k])) / max(1.0, abs(float(want[1][k]))), where)
                assert set(got[2]) == set(want[2]), (where, sorted(set(got[2]) ^ set(want[2])))
                for group in ("reconstruction", "moments", "logvar", "D."):
                    names = [k for k in want[2] if k.startswith(group)]
                    if names:
                        scale = max(want[2][k].abs().max().item() for k in names)
                        for k in names:
                            worst("grad " + group.rstrip("."), T.grad_rel(got[2][k], want[2][k], scale), where + " " + k)
    ctx.__exit__(None, None, None)
    if cond_channels:
        assert tuple(loss.discriminator.main[0].weight.shape) == (64, 5, 4, 4)
    worst.check({"out": TOL_PLAIN_OUT, "grad reconstruction": TOL_PLAIN_GRAD, "grad moments": TOL_PLAIN_GRAD, "grad logvar": TOL_PLAIN_GRAD,
                 "grad D": TOL_PLAIN_GRAD_D})


def test_plain_loss_refusals(hip_lib):
    """The plain forward: a weight map is refused (PoseLoss takes one), a wrong-shape cond and a cond / disc_in_channels mismatch are
    ValueErrors, and cond needs disc_conditional in both phases."""
    import test_plain_vae_gpu as T
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    ctx = T.quiet()
    x, xr, moments, _ = T.loss_tensors()
    loss, _ = plain_pair(0)
    for wmap in (torch.ones(2, 1, 32, 32), torch.ones(2, 3, 32, 32), torch.ones(1, 1, 32, 32), torch.ones(2, 1, 31, 32)):
        with pytest.raises(NotImplementedError, match="per-pixel"):      # (the plain forward's handling of weights is the parent's, untouched)
            T.evaluate(loss, DG, x, xr, moments, 0, 10, wmap, torch.float32, DEV)
    for idx in (0, 1):
        with pytest.raises(AssertionError):
            T.evaluate(loss, DG, x, xr, moments, idx, 10, None, torch.float32, DEV, cond=torch.zeros(2, 2, 32, 32))
    closs, _ = plain_pair(2)
    with pytest.raises(AssertionError):      # disc_conditional without cond, generator phase
        T.evaluate(closs, DG, x, xr, moments, 0, 10, None, torch.float32, DEV)
    for idx in (0, 1):
        with pytest.raises(ValueError, match="disc_in_channels"):
            T.evaluate(closs, DG, x, xr, moments, idx, 10, None, torch.float32, DEV, cond=torch.zeros(2, 3, 32, 32))
        with pytest.raises(ValueError, match="cond must be"):
            T.evaluate(closs, DG, x, xr, moments, idx, 10, None, torch.float32, DEV, cond=torch.zeros(2, 2, 16, 32))
    ctx.__exit__(None, None, None)


def test_one_pass_and_three_pass_adaptive_weight_agree_under_cond(hip_lib):
    import test_plain_vae_gpu as T
    from odvae_amd.distributions import DiagonalGaussianDistribution as DG
    ctx = T.quiet()
    loss, _ = plain_pair(2)
    loss.train()
    x, xr, moments, _ = T.loss_tensors()
    cond = torch.rand(2, 2, 32, 32, generator=torch.Generator().manual_seed(17))
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    out = {}
    for one_pass in (True, False):
        loss.ONE_PASS = one_pass
        loss.discriminator.load_state_dict(d_state)
        out[one_pass] = T.evaluate(loss, DG, x, xr, moments, 0, 10, None, torch.float32, DEV, cond=cond)
    del loss.ONE_PASS
    assert type(loss).ONE_PASS is True
    a, b = out[True], out[False]
    worst = T.Worst("one pass vs three passes under cond")
    worst("total", T.rel(a[0], b[0]))
    for k in b[1]:
        worst(k, abs(float(a[1][k]) - float(b[1][k])) / max(1.0, abs(float(b[1][k]))))
    assert set(a[2]) == set(b[2]) == {"reconstruction", "moments", "logvar"} and float(b[1]["train/d_weight"]) > 0
    for k in b[2]:
        worst("grad " + k, T.rel(a[2][k], b[2][k]))
    ctx.__exit__(None, None, None)
    worst.check({"": TOL_ONE_PASS})


def test_input_checks(hip_lib, inputs):
    d = inputs
    loss = product_loss()
    for bad in (torch.ones(3), torch.ones(4, 2, 32, 32), torch.ones(4, 1, 16, 32), torch.ones(4, 3, 32)):
        with pytest.raises(ValueError, match="do not broadcast"):
            call(loss, d, 0, 40, bad)
    with pytest.raises(ValueError, match="requires grad"):
        call(loss, d, 0, 40, torch.ones(4, 1, 32, 32, requires_grad=True))
    closs = product_loss(disc_conditional=True, disc_in_channels=5)
    for bad in (d["cond"][:2], d["cond"][:, :, :16], d["cond"][0], "cond"):
        for opt in (0, 1):
            with pytest.raises(ValueError, match="cond must be"):
                call(closs, d, opt, 40, None, bad)
    for opt in (0, 1):      # three side channels for a discriminator built for two
        with pytest.raises(ValueError, match="disc_in_channels"):
            call(closs, d, opt, 40, None, torch.cat((d["cond"], d["cond"][:, :1]), dim=1))
    with pytest.raises(AssertionError):      # upstream's pair of asserts, generator phase only
        call(closs, d, 0, 40)
    (dl, _), _ = call(product_loss(), d, 1, 40)      # no cond in the discriminator phase: no concatenation, no assert
    assert bool(torch.isfinite(dl))
    # bool and uint8 side channels are the same side channel
    binary = (d["cond"] > 0.5)
    want = call(closs, d, 0, 40, None, binary.float())[0][0]
    for cast in (torch.bool, torch.uint8):
        assert torch.equal(call(closs, d, 0, 40, None, binary.to(cast).cpu())[0][0], want)


# ---- model, trainer, launcher ----------------------------------------------------------------------------------------------------------
def side_model():
    from odvae_amd import synthetic
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=2, ch=32, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0,
                                      cond_key="cond", cond_channels=2, loss_weights_key="wts")
    synthetic.fill_state_procedural(model, seed=23)
    return model.to(DEV).train()


@pytest.mark.parametrize("precision", [None, "bf16"], ids=["f32", "bf16"])
def test_trainer_steps_with_cond_key_and_loss_weights_key(hip_lib, tmp_path, precision):
    """A step pair (both optimizers) with detect_anomaly on: finite losses, every input channel of the discriminator's first conv (3 image +
    2 side channels) got a gradient, validation runs; the f32 run's checkpoint holds the 5-channel layer and loads back bit for bit."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    model = side_model()
    assert model.cond_key == "cond" and model.loss_weights_key == "wts" and model.loss.disc_conditional
    w_d0 = model.loss.discriminator.main[0].weight.detach().clone()
    assert tuple(w_d0.shape) == (64, 5, 4, 4)
    b_d0 = model.loss.discriminator.main[0].bias.detach().clone()
    trainer = Trainer(model, gradient_clip_val=1.0, detect_anomaly=True, **({} if precision is None else {"precision": precision}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = synthetic.make_batch(4, 32, seed=60, cond_key="cond", cond_channels=2, weights_key="wts")
        losses = trainer.training_batch(batch, 0)
        assert len(losses) == 2 and all(x.dim() == 0 and bool(torch.isfinite(x)) for x in losses), losses
        logs = model.logged_metrics
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logs.values())
        assert float(logs["train/weighted_nll_loss"]) != float(logs["train/nll_loss"])
        moved = (model.loss.discriminator.main[0].weight.detach() - w_d0) != 0      # Adam moves exactly the entries whose gradient is not zero
        assert bool(moved.all()), "a weight of the first conv got no gradient: per input channel %s" % moved.float().mean(dim=(0, 2, 3)).tolist()
        assert bool(((model.loss.discriminator.main[0].bias.detach() - b_d0) != 0).all())
        metrics = trainer.validate([synthetic.make_batch(4, 32, seed=70, cond_key="cond", cond_channels=2, weights_key="wts")])
        assert bool(torch.isfinite(metrics["val/rec_loss"])) and bool(torch.isfinite(metrics["val/disc_loss"]))
        with pytest.raises(KeyError):      # a batch without the side channel is an error, not a silent unconditional step
            model._loss_extras(synthetic.make_batch(4, 32, seed=61))
        if precision is None:
            path = trainer.save_checkpoint(str(tmp_path / "side.ckpt"))
            sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
            assert tuple(sd["loss.discriminator.main.0.weight"].shape) == (64, 5, 4, 4)
            other = side_model()
            Trainer(other, gradient_clip_val=1.0).load_checkpoint(path)
            for (k, a), (_, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
                assert torch.equal(a, b), k


def test_run_main_with_the_overrides(hip_lib, capsys):
    from odvae_amd import run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = run.main(["-b", YAML, "--height", "32", "--steps", "2", "model.params.cond_key=cond", "model.params.loss_weights_key=wts",
                          "model.params.lossconfig.params.disc_conditional=True", "model.params.lossconfig.params.disc_in_channels=5",
                          "model.params.ddconfig.ch=32", "data.params.batch_size=4"])
    text = capsys.readouterr().out
    assert model.cond_key == "cond" and model.loss_weights_key == "wts" and text.count("batch ") == 2
    assert tuple(model.loss.discriminator.main[0].weight.shape) == (64, 5, 4, 4)


PLAIN_YAML = os.path.join(GOLD, "autoencoder_kl_plain.yaml")
PLAIN_SMALL = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
               "model.params.ddconfig.resolution=32", "model.params.lossconfig.params.disc_start=0"]
PLAIN_COND = ["model.params.cond_key=cond", "model.params.lossconfig.params.disc_conditional=True", "model.params.lossconfig.params.disc_in_channels=5"]


def test_plain_autoencoder_steps_with_cond_key(hip_lib):
    """AutoencoderKL with cond_key (its loss is the plain LPIPSWithDiscriminator, 3 + 2 channels into the discriminator): a step pair and
    a validation batch through the Trainer with detect_anomaly on; every weight of the discriminator's first conv moves; the model takes
    no loss_weights_key (a weight map is PoseLoss's)."""
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    from odvae_amd.trainer import Trainer
    config = Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(PLAIN_SMALL + PLAIN_COND))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(3)
        model = instantiate_from_config(config.model)
        synthetic.fill_state_procedural(model, seed=23)
        model.learning_rate = 2 * 4.5e-6
        model = model.to(DEV).train()
        assert model.cond_key == "cond" and model.loss.disc_conditional and not hasattr(model, "loss_weights_key")
        w_d0 = model.loss.discriminator.main[0].weight.detach().clone()
        assert tuple(w_d0.shape) == (64, 5, 4, 4)
        trainer = Trainer(model, gradient_clip_val=1.0, detect_anomaly=True)
        batch = synthetic.make_image_batch(2, 32, seed=5, cond_key="cond", cond_channels=2)
        assert tuple(batch["cond"].shape) == (2, 2, 32, 32) and torch.equal(batch["image"], synthetic.make_image_batch(2, 32, seed=5)["image"])
        losses = trainer.training_batch(batch, 0)
        assert len(losses) == 2 and all(x.dim() == 0 and bool(torch.isfinite(x)) for x in losses), losses
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in model.logged_metrics.values())
        assert bool(((model.loss.discriminator.main[0].weight.detach() - w_d0) != 0).all())
        metrics = trainer.validate([synthetic.make_image_batch(2, 32, seed=6, cond_key="cond", cond_channels=2)])
        assert bool(torch.isfinite(metrics["val/rec_loss"])) and bool(torch.isfinite(metrics["val/disc_loss"]))
        with pytest.raises(KeyError):
            model._loss_extras(synthetic.make_image_batch(2, 32, seed=7))
    bad = Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(PLAIN_SMALL + ["model.params.loss_weights_key=wts"]))
    with pytest.raises(TypeError):
        instantiate_from_config(bad.model)


def test_run_main_on_the_plain_yaml_with_cond_key(hip_lib, capsys):
    from odvae_amd import run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = run.main(["-b", PLAIN_YAML, "--height", "32", "--steps", "2", "data.params.batch_size=2"] + PLAIN_SMALL + PLAIN_COND)
    text = capsys.readouterr().out
    assert model.cond_key == "cond" and text.count("batch ") == 2 and model.global_step == 4
    assert tuple(model.loss.discriminator.main[0].weight.shape) == (64, 5, 4, 4)
    assert all(torch.isfinite(v).all() for v in model.logged_metrics.values() if torch.is_tensor(v))


def test_with_neither_argument_a_step_computes_the_bits_it_did_before(hip_lib):
    """tests/golden/weights_cond_unset_parent.npz was sampled at the commit before `weights` maps and `cond` were honoured
    (tests/golden/weights_cond_unset_step.py): a PoseAutoencoder step pair without the keys, and the plain loss with weights None, a scalar
    and one weight per sample."""
    from weights_cond_unset_step import run_steps
    want = np.load(os.path.join(GOLD, "weights_cond_unset_parent.npz"))
    got = run_steps(DEV)
    assert sorted(got.keys()) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
