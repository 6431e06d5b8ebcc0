"""`use_actnorm: True` through the model: the ActNorm PatchGAN against its plain-torch restatement (tests/actnorm_ref.py), PoseLoss with
it against the oracle's PoseLoss carrying the restated discriminator, the generator phase's initialisation with the discriminator
switched off, and the runner end to end.  The oracle package ignores `use_actnorm`, so the yardstick discriminator is always the
restatement with the same state.  Tolerances: whole networks 1e-3 / 5e-3 (tests/test_gan_lpips_gpu.py); training batches 2e-3 on
the losses and 5e-3 on logged values (tests/test_model_gpu.py::test_gan_lpips_training_batch_matches_oracle), gradients 5e-3 of
max(|ref grad|, 1e-3 * the largest gradient) as tests/test_model_gpu.py::check_step takes them."""
import os
import re
import subprocess
import sys

import pytest
import torch

import actnorm_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def close(a, b, tol, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    ref = max(1e-6, b.abs().max().item())
    assert err <= tol * ref, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, ref)


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


# ---- the discriminator alone ---------------------------------------------------------------------------------------------------------
# LeakyReLU's derivative jumps from 0.2 to 1 at h = 0, and on the initialising step every normalised channel is centred on exactly that
# point.  Where a pre-activation lies within the forward's own rounding of 0, neither slope is wrong, but the layer in front of main.9
# sums only 98 rows at 64 x 64, so ONE such element moves its weight gradient by about 2 % of its largest entry (seen on the device
# with an input that has |h_64| = 1.3e-6 at main.9: every other tensor within 5e-3, main.8.weight off by 1.7e-2).  As
# `bn_offset_inputs.kink_free_dy` does for the single op, the inputs are therefore chosen -- from the restatement alone -- so that no
# LeakyReLU input comes closer to 0 in float64 than KINK_FACTOR times torch f32's own deviation from float64 at that layer; the test
# asserts that rule before it compares anything.  (size -> seeds of the two steps' inputs; found by counting up from 6 and 106)
KINK_FACTOR = 4.0
INPUT_SEEDS = {64: (76, 248), 32: (7, 115)}


def lrelu_inputs(net, x):
    """the inputs of the restatement's four LeakyReLU layers for one (graph-less) forward of x"""
    pre = []
    # (a pre-hook: the restatement's LeakyReLU works in place, so after its forward the input holds the output)
    hooks = [m.register_forward_pre_hook(lambda m, i: pre.append(i[0].detach().clone())) for m in net.main if isinstance(m, torch.nn.LeakyReLU)]
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return pre


@pytest.mark.parametrize("size", [64, 32])
def test_discriminator_matches_the_restatement(hip_lib, size):
    """Logits, dx and every parameter gradient on the initialising step and on the following one; loc / scale after the first"""
    import copy
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    torch.manual_seed(5)
    ref = A.NLayerDiscriminator(n_layers=3).apply(A.weights_init)
    net = NLayerDiscriminator(n_layers=3, use_actnorm=True).apply(weights_init)
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    ref.train(); net.train()
    ref64 = copy.deepcopy(ref).double()
    assert net.actnorm_uninitialized()
    for step in range(2):
        x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(INPUT_SEEDS[size][step]))
        # the rule on the inputs: the kink is further away than KINK_FACTOR x torch f32's own deviation, at every LeakyReLU
        # (both copies initialise here on step 0; the second forward of `ref` below then finds it initialised: same values)
        for k, (h32, h64) in enumerate(zip(lrelu_inputs(ref, x), lrelu_inputs(ref64, x.double()))):
            assert h64.abs().min().item() >= KINK_FACTOR * (h32.double() - h64).abs().max().item(), (step, k)
        xr = x.clone().requires_grad_(True)
        ref.zero_grad(); net.zero_grad()
        y_ref = ref(xr)
        gy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(8 + step))
        y_ref.backward(gy)
        xd = x.to(DEV).requires_grad_(True)
        y = net(xd)
        what = "D(%d) step %d " % (size, step)
        close(y, y_ref, 1e-3, what + "fwd")
        y.backward(gy.to(DEV))
        close(xd.grad, xr.grad, 5e-3, what + "dx")
        refp = dict(ref.named_parameters())
        for name, p in net.named_parameters():
            close(p.grad, refp[name].grad, 5e-3, what + "grad " + name)
        if step == 0:
            keep = {k: v.detach().clone() for k, v in net.state_dict().items() if k.endswith(("loc", "scale"))}
            assert not net.actnorm_uninitialized()
        for (name, m), mr in zip(((n, m) for n, m in net.named_modules() if type(m).__name__ == "ActNormLReLU"), A.actnorm_layers(ref)):
            assert int(m.initialized) == 1 and int(mr.initialized) == 1
            close(m.loc * mr.scale.to(DEV), mr.loc * mr.scale, 1e-3, what + name + ".loc in units of the channel's std")
            close(m.scale, mr.scale, 1e-3, what + name + ".scale")
    for k, v in keep.items():          # the second training forward initialised nothing
        assert torch.equal(net.state_dict()[k], v), k


# ---- PoseLoss with the ActNorm discriminator against the oracle ------------------------------------------------------------------------------
def build_pair(disc_factor, perceptual_weight):
    """tests/test_model_gpu.py::build_pair with `use_actnorm: True` in the lossconfig; the oracle's loss gets the restated discriminator"""
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from oracle.autoencoder import PoseAutoencoder as OraclePA
    torch.manual_seed(23)
    mcfg, cfg = synthetic.model_config(YAML, latent_hw=4, ch=32, perceptual_weight=perceptual_weight, disc_factor=disc_factor, disc_start=0)
    mcfg.params.lossconfig.params["use_actnorm"] = True
    model = instantiate_from_config(mcfg)
    model.learning_rate = 12 * cfg.model.base_learning_rate
    p = mcfg.params.to_container()
    ref = OraclePA(p["ddconfig"], dict(p["lossconfig"]["params"]), p["embed_dim"], p["pose_decoder_config"]["params"],
                   p["pose_encoder_config"]["params"], feat_dims=p.get("feat_dims", [16, 16, 16]), dropout_prob_init=p["dropout_prob_init"],
                   dropout_prob_final=p["dropout_prob_final"], dropout_warmup_steps=p["dropout_warmup_steps"],
                   pose_conditioned_generation_steps=p["pose_conditioned_generation_steps"],
                   add_noise_to_z_obj=p["add_noise_to_z_obj"], train_on_yaw=p["train_on_yaw"])
    ref.loss.discriminator = A.NLayerDiscriminator(n_layers=3)
    res = ref.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert len(model.loss.discriminator.actnorm_layers()) == 3
    model, ref = model.to(DEV).train(), ref.train()
    ref.loss.perceptual_loss.eval()       # the product's metric pins itself to eval mode
    return model, ref


def phase(model, ref, batch, noise, idx, global_step):
    """One optimizer phase on both sides with PL's toggle_optimizer (the other optimizer's parameters do not require grad), no
    optimizer step: (loss, loss_ref, logs, logs_ref); gradients are left on the parameters."""
    for m, prefix in ((model, "loss.discriminator."), (ref, "loss.discriminator.")):
        for name, p in m.named_parameters():
            if name == "loss.logvar" or name.startswith("loss.perceptual_loss"):
                continue
            p.requires_grad_(name.startswith(prefix) == (idx == 1))
            p.grad = None
    model._global_step = ref.global_step = global_step
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, idx)
    logs = dict(model.logged_metrics)
    loss_ref, log_ref, _ = ref.training_step(batch, idx, noise)
    loss.backward()
    loss_ref.backward()
    return loss, loss_ref, logs, log_ref


def compare_grads(model, ref, prefixes, tol, what):
    ref_params = dict(ref.named_parameters())
    scale = max(p.grad.abs().max().item() for p in ref_params.values() if p.grad is not None)
    seen = 0
    for name, p in model.named_parameters():
        if not name.startswith(prefixes):
            continue
        rg = ref_params[name].grad
        if rg is None:
            assert p.grad is None or p.grad.abs().max().item() == 0.0, (what, name)
            continue
        assert p.grad is not None, (what, name)
        e = (p.grad.detach().cpu().double() - rg.double()).abs().max().item() / max(rg.abs().max().item(), 1e-3 * scale)
        print("%s grad %-40s rel err %.3e" % (what, name, e))
        assert e < tol, "%s: param grad %s rel err %.3e" % (what, name, e)
        seen += 1
    return seen


def test_pose_loss_with_actnorm_matches_oracle_over_two_steps(hip_lib):
    """Generator phase then discriminator phase, two consecutive steps at 64x64, B = 2, disc_start = 0: the first generator phase
    initialises the ActNorm layers from D(x_rec * mask), as upstream does; every value the oracle logs, d_weight among them, and the
    gradients of the decoder's last layer and of the discriminator."""
    from odvae_amd import synthetic
    model, ref = build_pair(disc_factor=1.0, perceptual_weight=1.0)
    assert model.loss.discriminator.actnorm_uninitialized()
    gs = 1          # from global_step 1 on the adaptive weight is live (global_step > encoder_pretrain_steps = 0)
    for step in range(2):
        batch = synthetic.make_batch(2, 64, seed=300 + step)
        for idx in (0, 1):
            noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=400 + 2 * step + idx)
            loss, loss_ref, logs, log_ref = phase(model, ref, batch, noise, idx, gs)
            what = "step %d optimizer %d" % (step, idx)
            a, b = loss.item(), loss_ref.item()
            print("%s loss %.6f oracle %.6f" % (what, a, b))
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (what, a, b)
            assert len(log_ref) >= 3
            for key, want in log_ref.items():
                e = rel(logs[key], want)
                print("%s %-32s %.6g oracle %.6g rel %.2e" % (what, key, float(logs[key]), float(want), e))
                assert e < 5e-3, (what, key, float(logs[key]), float(want))
            if idx == 0:
                assert float(log_ref["train/d_weight"]) > 0.0
                assert compare_grads(model, ref, ("decoder.conv_out",), 5e-3, what) == 2
            else:
                assert compare_grads(model, ref, ("loss.discriminator",), 5e-3, what) == 16
            assert not model.loss.discriminator.actnorm_uninitialized()
            gs += 1


def test_generator_phase_initialises_actnorm_with_the_discriminator_off(hip_lib):
    """disc_factor = 0: the generator phase skips D except while an ActNorm layer is uninitialised -- upstream evaluates
    D(x_rec * mask) on every step, so its ActNorm initialises from that tensor on the first training batch.  After the first phase the
    layers hold what the restatement's run of D(x_rec * mask) gives; the term contributes an exact 0: the total and the gradients
    are the oracle's at tests/test_model_gpu.py's tolerances for this network (2e-5, 4.4e-4); the second phase does not run D."""
    from odvae_amd import synthetic
    model, ref = build_pair(disc_factor=0.0, perceptual_weight=0.0)
    assert not model.loss.log_exact_g_loss
    calls = []
    model.loss.discriminator.register_forward_hook(lambda *a: calls.append(1))
    for step in range(2):
        batch = synthetic.make_batch(2, 64, seed=5 + step)
        noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6 + step)
        loss, loss_ref, logs, log_ref = phase(model, ref, batch, noise, 0, 1 + step)
        assert len(calls) == 1, "D runs in the first generator phase only"
        assert rel(loss, loss_ref) < 2e-5, (loss.item(), loss_ref.item())
        assert float(logs["train/g_loss"]) == 0.0 and float(logs["train/d_weight"]) == 0.0
        for key in ("kl_loss_obj", "nll_loss", "rec_loss", "pose_loss", "class_loss", "bbox_loss", "kl_loss_bbox", "fill_factor_loss", "total_loss"):
            assert rel(logs["train/" + key], log_ref["train/" + key]) < 2e-5, key
        assert compare_grads(model, ref, ("encoder", "decoder", "quant_conv_obj", "post_quant_conv", "pose_"), 4.4e-4, "step %d" % step) > 50
        for name, p in model.named_parameters():
            if name.startswith("loss.discriminator"):
                assert p.grad is None, name
        if step == 0:
            layers, layers_ref = model.loss.discriminator.actnorm_layers(), A.actnorm_layers(ref.loss.discriminator)
            assert len(layers) == len(layers_ref) == 3
            keep = []
            for m, mr in zip(layers, layers_ref):
                assert int(m.initialized) == 1 and m._initialized_host and int(mr.initialized) == 1
                close(m.loc * mr.scale.to(DEV), mr.loc * mr.scale, 1e-3, "loc in units of the channel's std")
                close(m.scale, mr.scale, 1e-3, "scale")
                keep.append((m.loc.detach().clone(), m.scale.detach().clone()))
    for m, (loc, scale) in zip(model.loss.discriminator.actnorm_layers(), keep):
        assert torch.equal(m.loc.detach(), loc) and torch.equal(m.scale.detach(), scale)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
def test_run_to_completion_with_use_actnorm(hip_lib):
    """`use_actnorm: True` from the command line, GAN on from step 0, under the yaml's detect_anomaly: True; a fresh child process
    (its own HIP context) with a time limit"""
    cmd = [sys.executable, "-m", "odvae_amd.run", "-b", os.path.join("tests", "golden", "autoencoder_kl_16x16x16.yaml"), "--steps", "3",
           "--height", "64", "model.params.lossconfig.params.use_actnorm=True", "model.params.lossconfig.params.disc_start=0",
           "model.params.lossconfig.params.encoder_pretrain_steps=0", "data.params.batch_size=2"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"batch (\d+)\s+global_step (\d+)\s+aeloss (\S+)\s+discloss (\S+)", r.stdout)
    assert [int(l[0]) for l in lines] == [0, 1, 2] and int(lines[-1][1]) == 6, r.stdout[-2000:]
    for l in lines:
        assert torch.isfinite(torch.tensor([float(l[2]), float(l[3])])).all(), l
