"""image_mask_key on the device: PoseLoss with an alpha mask against what the REFERENCE's PoseLoss.forward returned and logged
(tests/golden/reference_mask.npz, written by tests/golden/make_reference_mask_goldens.py), a width-reduced PoseAutoencoder with the three
keys set (image_mask_key, ddconfig.out_ch: 4, disc_in_channels: 4) through Trainer steps in f32 and under precision: bf16, its
checkpoint, the input checks, and -- with the key unset -- the same bits as before the key was honoured.

Tolerances against the fixture (relative, as tests/test_reference_glue_gpu.py takes them: scalars to |expected| + 1e-6, the gradient to its
norm).  The fixture is the reference evaluated in float64, so the distance is the device path's own f32 rounding; measured worst on an
MI355X over all cases (profiles/image_mask.md): scalars 2.25e-7, gradient norm 1.39e-7, gradient samples 5.14e-8.  The three bounds
below are 4x those, far under that file's constants for the 3-channel cases (5e-6 and 4e-5).

Where the reference returns a [B,1,H,W] tensor (use_mask_loss past encoder_pretrain_steps: its weighted_mask_loss is left unreduced), the
product returns the scalar the reference logs as total_loss -- the tensor's mean -- and the gradient compared is that of the mean."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path[:0] = [HERE, GOLD]
from reference_cases import LABELS, LOSS_KW, digest_of, stats_table  # noqa: E402

YAML = os.path.join(GOLD, "autoencoder_kl_16x16x16.yaml")
MASK_KW = dict(mask_weight=0.5, perceptual_weight=1.0, disc_in_channels=4)
CLASS_IDS = [0, 1, 3, 0]
STEPS = (5, 12, 20, 40)
SCALAR_TOL, GRAD_NORM_TOL, GRAD_SAMPLE_TOL = 9.0e-7, 5.5e-7, 2.0e-7
WORST = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "reference_mask.npz"))


@pytest.fixture(scope="module")
def inputs(gold):
    return {k[3:]: torch.from_numpy(gold[k]).to(DEV) for k in gold.files if k.startswith("in.") and k != "in.global_steps"}


def product_loss(fn, uml):
    from odvae_amd.losses import PoseLoss
    from odvae_amd.synthetic import fill_state_procedural
    torch.manual_seed(5)
    loss = PoseLoss(dataset_stats=stats_table(), **dict(LOSS_KW, mask_loss_fn=fn, use_mask_loss=uml, **MASK_KW))
    fill_state_procedural(loss, seed=31)
    with torch.no_grad():
        loss.logvar.fill_(0.3)
    return loss.to(DEV).train()


def call(loss, d, opt, gs, with_mask=True):
    """One PoseLoss.forward on the fixture's inputs with dec_obj = conv3x3(feat) of a stand-in conv_out [4,8,3,3]; (ret, dec_obj)."""
    from odvae_amd import modules
    from odvae_amd.distributions import DiagonalGaussianDistribution as D
    from odvae_amd.synthetic import fill_state_procedural
    last = modules.Conv3x3(8, 4).to(DEV)
    with torch.no_grad():
        last.weight.copy_(d["last_w"])
        last.bias.copy_(d["last_b"])
        fill_state_procedural(loss.discriminator, seed=31)
    dec_obj = last(d["feat"].clone().requires_grad_(True))
    ret = loss(d["rgb_gt"], d["mask_gt"] if with_mask else None, d["pose_gt"], dec_obj, d["dec_pose"].clone().requires_grad_(True), d["class_id"],
               [LABELS[c] for c in CLASS_IDS], d["bbox_gt"], d["fill_factor_gt"], D(d["moments"].clone().requires_grad_(True)),
               D(d["bbox_moments"].clone().requires_grad_(True)), opt, gs, d["mask_2d_bbox"], last_layer=last.weight, split="train")
    return ret, dec_obj


def check_case(gold, pre, ret, dec_obj):
    out, log = ret
    assert out.dim() == 0, "the returned loss is a scalar in every phase"

    def scalar(key, got, want):
        e = abs(float(torch.as_tensor(got).detach()) - float(want)) / (abs(float(want)) + 1e-6)
        WORST["scalar"] = max(WORST.get("scalar", 0.0), e)
        assert e <= SCALAR_TOL, "%s %s: %.8g vs %.8g (rel %.2e)" % (pre, key, float(got), float(want), e)

    scalar("loss", out, gold[pre + ".loss_mean"])
    keys = [f[len(pre + ".log."):] for f in gold.files if f.startswith(pre + ".log.")]
    assert sorted(keys) == sorted(log.keys())
    for k in keys:
        scalar(k, log[k], gold[pre + ".log." + k])
    if pre + ".grad.dec_obj.norm" in gold.files:
        dec_obj.retain_grad()      # only now: the one-pass adaptive weight's own autograd.grad calls would be accumulated into .grad too
        out.backward()
        gn = float(gold[pre + ".grad.dec_obj.norm"])
        norm, samples = digest_of(dec_obj.grad, limit=1024, keep=512)
        e1 = abs(float(norm) - gn) / gn
        e2 = float(np.abs(samples.astype(np.float64) - gold[pre + ".grad.dec_obj.samples"]).max()) / gn
        WORST["grad.norm"] = max(WORST.get("grad.norm", 0.0), e1)
        WORST["grad.sample"] = max(WORST.get("grad.sample", 0.0), e2)
        assert e1 <= GRAD_NORM_TOL and e2 <= GRAD_SAMPLE_TOL, "%s grad: norm %.8g vs %.8g (%.2e), samples %.2e" % (pre, norm, gn, e1, e2)
    else:
        assert not out.requires_grad or dec_obj.grad is None


@pytest.mark.parametrize("one_pass", [True, False], ids=["one-pass-weight", "three-pass-weight"])
@pytest.mark.parametrize("fn", ["l1", "l2"])
@pytest.mark.parametrize("uml", [True, False], ids=["mask-loss", "no-mask-loss"])
def test_pose_loss_with_a_mask_matches_the_reference(hip_lib, gold, inputs, uml, fn, one_pass):
    loss = product_loss(fn, uml)
    loss.ONE_PASS = one_pass
    assert sorted(loss.state_dict().keys()) == list(gold["state_keys"])
    for gs in STEPS:
        for opt in (0, 1):
            check_case(gold, "mask.uml%d.%s.step%d.opt%d" % (int(uml), fn, gs, opt), *call(loss, inputs, opt, gs))
            assert loss.use_mask_loss == uml
    print("image_mask margins (worst relative distance to the reference):", {k: "%.2e" % v for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("fn", ["l1", "l2"])
def test_use_mask_loss_stays_off_after_a_call_without_a_mask(hip_lib, gold, inputs, fn):
    """QUIRK (contperceptual.py:232): the reference switches use_mask_loss off for good.  optimizer_idx 2 evaluates and returns None."""
    loss = product_loss(fn, True)
    ret, _ = call(loss, inputs, 2, 40, with_mask=False)
    assert ret is None and loss.use_mask_loss is False
    check_case(gold, "sticky.%s.step40.opt0" % fn, *call(loss, inputs, 0, 40))


def test_mask_input_checks(hip_lib, inputs):
    from odvae_amd import modules
    loss = product_loss("l2", True)
    d = dict(inputs)
    for bad in (d["mask_gt"][:, 0], d["mask_gt"][:2], d["mask_gt"].expand(-1, 3, -1, -1), d["mask_gt"][:, :, :16]):
        with pytest.raises(ValueError):
            call(loss, dict(d, mask_gt=bad), 0, 40)
    # a mask with a 3-channel reconstruction (the reference dies there with a shape error in its discriminator call)
    rec3 = modules.Conv3x3(8, 3).to(DEV)(d["feat"])
    from odvae_amd.distributions import DiagonalGaussianDistribution as D
    with pytest.raises(ValueError):
        loss(d["rgb_gt"], d["mask_gt"], d["pose_gt"], rec3, d["dec_pose"], d["class_id"], [LABELS[c] for c in CLASS_IDS], d["bbox_gt"],
             d["fill_factor_gt"], D(d["moments"]), D(d["bbox_moments"]), 0, 40, d["mask_2d_bbox"], last_layer=None, split="train")
    assert loss.use_mask_loss is True      # a refused call changes nothing
    # bool and uint8 masks are the same mask
    want = call(loss, d, 0, 40)[0][1]["train/mask_loss"]
    for cast in (torch.bool, torch.uint8):
        got = call(loss, dict(d, mask_gt=d["mask_gt"].to(cast)), 0, 40)[0][1]["train/mask_loss"]
        assert torch.equal(got, want)


def mask_model(uml, precision=None):
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    mcfg, _ = synthetic.model_config(YAML, latent_hw=2, ch=32, phase="vae", perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
    p = mcfg.params
    p["image_mask_key"] = "mask"
    p.ddconfig["out_ch"] = 4
    lp = p.lossconfig.params
    lp["disc_in_channels"], lp["mask_weight"], lp["use_mask_loss"] = 4, 0.5, uml
    torch.manual_seed(3)
    model = instantiate_from_config(mcfg)
    model.learning_rate = 12 * 4.5e-6
    synthetic.fill_state_procedural(model, seed=23)
    return model.to(DEV).train()


@pytest.mark.parametrize("uml", [False, True], ids=["no-mask-loss", "mask-loss"])
@pytest.mark.parametrize("precision", [None, "bf16", "bf16+disc"], ids=["f32", "bf16", "bf16-disc-bf16"])
def test_trainer_steps_with_the_three_keys(hip_lib, tmp_path, precision, uml):
    """Two batches, both optimizers: finite losses, all four channels of conv_out and of the discriminator's first layer move (each got a
    gradient), validation and log_images run, and the checkpoint holds the 4-channel layers and loads back bit for bit."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    model = mask_model(uml)
    kw = {} if precision is None else {"precision": "bf16"}
    if precision == "bf16+disc":
        kw["discriminator_precision"] = "bf16"
    trainer = Trainer(model, gradient_clip_val=1.0, **kw)
    w_out, w_d0 = model.decoder.conv_out.weight.detach().clone(), model.loss.discriminator.main[0].weight.detach().clone()
    assert tuple(w_out.shape) == (4, 32, 3, 3) and tuple(w_d0.shape) == (64, 4, 4, 4)
    for step in range(2):
        batch = synthetic.make_batch(4, 32, seed=60 + step, mask_key="mask")
        assert tuple(batch["mask"].shape) == (4, 1, 32, 32) and set(batch["mask"].unique().tolist()) <= {0.0, 1.0}
        losses = trainer.training_batch(batch, step)
        assert len(losses) == 2 and all(x.dim() == 0 and bool(torch.isfinite(x)) for x in losses), losses
        logs = model.logged_metrics
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logs.values())
        assert (float(logs["train/mask_loss"]) > 0.0) == uml
    moved_out = (model.decoder.conv_out.weight.detach() - w_out).abs().amax(dim=(1, 2, 3))
    moved_d0 = (model.loss.discriminator.main[0].weight.detach() - w_d0).abs().amax(dim=(0, 2, 3))
    assert bool((moved_out > 0).all()) and bool((moved_d0 > 0).all()), (moved_out.tolist(), moved_d0.tolist())
    if precision is None:
        metrics = trainer.validate([synthetic.make_batch(4, 32, seed=70, mask_key="mask")])
        assert bool(torch.isfinite(metrics["val/rec_loss"])) and (float(metrics["val/mask_loss"]) > 0.0) == uml
        imgs = model.log_images(synthetic.make_batch(4, 32, seed=71, mask_key="mask"))
        assert tuple(imgs["reconstructions_rgb"].shape) == (4, 3, 32, 32)      # xrec[:, :3], as the reference logs it
        path = trainer.save_checkpoint(str(tmp_path / "mask.ckpt"))
        sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
        assert tuple(sd["decoder.conv_out.weight"].shape) == (4, 32, 3, 3)
        assert tuple(sd["loss.discriminator.main.0.weight"].shape) == (64, 4, 4, 4)
        other = mask_model(uml)
        Trainer(other, gradient_clip_val=1.0).load_checkpoint(path)
        for (k, a), (_, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
            assert torch.equal(a, b), k
        assert other.global_step == model.global_step


def test_run_main_with_the_three_keys(hip_lib, tmp_path, capsys):
    """python -m odvae_amd.run with image_mask_key, out_ch 4, disc_in_channels 4 and a log directory (network narrowed to ch = 32): two
    batches train, one validates, ImageLogger writes 3-channel images, and <logdir>/checkpoints/last.ckpt holds the 4-channel layers."""
    from odvae_amd import run
    logdir = str(tmp_path / "mask")
    model = run.main(["-b", YAML, "--height", "32", "--steps", "2", "-l", logdir, "model.params.image_mask_key=mask",
                      "model.params.ddconfig.out_ch=4", "model.params.lossconfig.params.disc_in_channels=4", "model.params.ddconfig.ch=32",
                      "data.params.batch_size=4"])
    text = capsys.readouterr().out
    assert model.image_mask_key == "mask" and text.count("batch ") == 2 and "val/mask_loss" in text and "checkpoint" in text
    sd = torch.load(os.path.join(logdir, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=True)["state_dict"]
    assert tuple(sd["decoder.conv_out.weight"].shape) == (4, 32, 3, 3) and tuple(sd["loss.discriminator.main.0.weight"].shape) == (64, 4, 4, 4)
    pngs = [f for _, _, fs in os.walk(os.path.join(logdir, "images")) for f in fs if f.endswith(".png")]
    assert any(f.startswith("reconstructions_rgb") for f in pngs) and any(f.startswith("inputs_rgb") for f in pngs), pngs


def test_pretrain_phase_with_a_mask_hands_the_loss_four_channels(hip_lib):
    """Before encoder_pretrain_steps the decoder does not run and dec_obj is all zeros: with image_mask_key it has the decoder's four
    channels (the reference's zeros_like(input_im) would die in its 4-channel discriminator), without the key the input's three."""
    from odvae_amd import synthetic
    model = mask_model(True)
    model.encoder_pretrain_steps = 5
    x = model._rgb_input(synthetic.make_batch(2, 32, seed=80))
    assert tuple(model(x)[0].shape) == (2, 4, 32, 32) and float(model(x)[0].abs().max()) == 0.0
    model.image_mask_key = None
    assert tuple(model(x)[0].shape) == (2, 3, 32, 32)


def test_with_the_key_unset_a_step_computes_the_bits_it_did_before(hip_lib):
    """tests/golden/mask_unset_parent.npz was sampled at the commit before image_mask_key was honoured (tests/golden/mask_unset_step.py)."""
    from mask_unset_step import run_steps
    want = np.load(os.path.join(GOLD, "mask_unset_parent.npz"))
    got = run_steps(DEV)
    assert sorted(got.keys()) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
