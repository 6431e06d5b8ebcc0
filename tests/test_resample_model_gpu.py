"""ddconfig.resamp_with_conv = False and tanh_out = True through Encoder / Decoder and the whole model on the device.
Oracle parity follows tests/test_modules_gpu.py (width-reduced ch=32 network at 64x64, B=2, the oracle's state_dict; outputs 1e-3, gradients
3e-3 of max|ref|, parameter gradients against max(|ref grad|, 1e-3 * largest gradient)); the activation-checkpoint policies agree bit for bit,
as tests/test_model_gpu.py holds them to; bf16 follows tests/test_bf16_model_gpu.py's rule (no further from the f32 oracle than twice the
oracle under CPU autocast, plus that file's floors)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
DD = dict(double_z=True, z_channels=16, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2, 4],
          num_res_blocks=2, attn_resolutions=[16], dropout=0.0)
CONVLESS = dict(resamp_with_conv=False)


def rel_err(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


def _watch_resamplers(net, seen):
    """Forward hooks: did each conv-less resampler's output carry the GroupNorm statistics for the Normalize that reads it next?"""
    from odvae_amd import modules, ops
    handles = []
    for name, m in net.named_modules():
        if isinstance(m, (modules.Upsample, modules.Downsample)) and not m.with_conv:
            handles.append(m.register_forward_hook(lambda mod, inp, out, name=name: seen.append((name, ops._gn_partials_of(out, 32) is not None))))
    return handles


@pytest.mark.parametrize("which,extra", [("encoder", CONVLESS), ("decoder", CONVLESS), ("decoder", dict(tanh_out=True)),
                                         ("decoder", dict(tanh_out=True, resamp_with_conv=False))],
                         ids=["encoder-convless", "decoder-convless", "decoder-tanh", "decoder-tanh-convless"])
def test_encoder_decoder_match_oracle(hip_lib, which, extra):
    from odvae_amd import modules
    from oracle import ldm_model
    torch.manual_seed(23)
    cfg = dict(DD, **extra)
    ref = getattr(ldm_model, which.capitalize())(**cfg)
    net = getattr(modules, which.capitalize())(**cfg)
    missing = net.load_state_dict(ref.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    net = net.to("cuda:0")
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 64, 64, generator=g) if which == "encoder" else torch.randn(2, 16, 4, 4, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    xd = x.to("cuda:0").requires_grad_(True)
    seen = []
    handles = _watch_resamplers(net, seen)
    y = net(xd)
    for h in handles:
        h.remove()
    if not cfg.get("resamp_with_conv", True):
        assert len(seen) == 4 and all(ok for _, ok in seen), seen      # every resampler left the statistics: no statistics pass behind it
    else:
        assert not seen
    assert tuple(y.shape) == tuple(y_ref.shape)
    assert rel_err(y, y_ref) < 1e-3, "forward rel err %.3e" % rel_err(y, y_ref)
    if cfg.get("tanh_out"):
        assert y.abs().max().item() <= 1.0
    y.backward(gy.to("cuda:0"))
    assert rel_err(xd.grad, xr.grad) < 3e-3, "input grad rel err %.3e" % rel_err(xd.grad, xr.grad)
    worst = ("", 0.0)
    ref_params = dict(ref.named_parameters())
    # some gradients are analytically zero (attention k.bias: softmax is shift-invariant), so errors are
    # measured against max(|ref grad|, 1e-3 * largest gradient in the net)
    scale = max(p.grad.abs().max().item() for p in ref_params.values())
    for name, p in net.named_parameters():
        r = ref_params[name].grad.double()
        e = (p.grad.detach().cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        if e > worst[1]:
            worst = (name, e)
    print("%s %s: forward %.3e, input grad %.3e, worst param grad %s %.3e" % (which, extra, rel_err(y, y_ref), rel_err(xd.grad, xr.grad), *worst))
    assert worst[1] < 3e-3, "param grad %s rel err %.3e" % worst


def test_give_pre_end_returns_before_the_tanh(hip_lib):
    from odvae_amd import modules
    torch.manual_seed(2)
    net = modules.Decoder(**dict(DD, tanh_out=True, resamp_with_conv=False, give_pre_end=True)).to("cuda:0")
    with torch.no_grad():
        h = net(torch.randn(1, 16, 4, 4, generator=torch.Generator().manual_seed(3)).to("cuda:0"))
    assert tuple(h.shape) == (1, 32, 64, 64)      # the last Upsample's (here: last ResnetBlock's) feature map, not a squashed image


def test_decoder_checkpoint_policies_are_bit_identical(hip_lib):
    """activation_checkpoint False / "unit" / "norm" on Decoder(resamp_with_conv=False, tanh_out=True): deterministic kernels on the same
    values -- output and every gradient bit-identical (the tanh sits behind the "norm" policy's re-make context, the resamplers between the
    recomputed units)."""
    from odvae_amd import modules
    torch.manual_seed(23)
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 16, 4, 4, generator=g)
    outs = []
    state = None
    for policy in (False, "unit", "norm", True):
        net = modules.Decoder(**dict(DD, tanh_out=True, resamp_with_conv=False, activation_checkpoint=policy))
        if state is None:
            state = net.state_dict()
        net.load_state_dict(state, strict=True)
        net = net.to("cuda:0").train()
        zd = z.to("cuda:0").requires_grad_(True)
        y = net(zd)
        if not outs:
            gy = torch.randn(y.shape, generator=g).to("cuda:0")
        y.backward(gy)
        outs.append((y.detach(), zd.grad, {k: p.grad for k, p in net.named_parameters()}))
    y0, dz0, g0 = outs[0]
    assert g0["conv_in.weight"].abs().max().item() > 0
    for policy, (y, dz, grads) in zip(("unit", "norm", True), outs[1:]):
        assert torch.equal(y, y0) and torch.equal(dz, dz0), policy
        for k in g0:
            assert torch.equal(grads[k], g0[k]), (policy, k)


def _build_pair(dd_extra):
    """tests/test_model_gpu.py's build_pair with extra ddconfig keys."""
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    from oracle.autoencoder import PoseAutoencoder as OraclePA
    torch.manual_seed(23)
    mcfg, cfg = synthetic.model_config(YAML, latent_hw=4, ch=32)
    for k, v in dd_extra.items():
        mcfg.params.ddconfig[k] = v
    model = instantiate_from_config(mcfg)
    model.learning_rate = 12 * cfg.model.base_learning_rate
    p = mcfg.params.to_container()
    ref = OraclePA(p["ddconfig"], dict(p["lossconfig"]["params"]), p["embed_dim"], p["pose_decoder_config"]["params"],
                   p["pose_encoder_config"]["params"], feat_dims=p.get("feat_dims", [16, 16, 16]), dropout_prob_init=p["dropout_prob_init"],
                   dropout_prob_final=p["dropout_prob_final"], dropout_warmup_steps=p["dropout_warmup_steps"],
                   pose_conditioned_generation_steps=p["pose_conditioned_generation_steps"],
                   add_noise_to_z_obj=p["add_noise_to_z_obj"], train_on_yaw=p["train_on_yaw"])
    res = ref.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ref.learning_rate = model.learning_rate
    return model.to("cuda:0"), ref


def test_bf16_step_is_as_close_to_f32_as_autocast(hip_lib):
    """The conv-less, tanh_out network under set_precision("bf16"): the resamplers run on the bf16 kernels, the two f32 ends stay f32."""
    from test_bf16_model_gpu import flat, rel, run_oracle
    from odvae_amd import ops, synthetic
    model, ref = _build_pair(dict(resamp_with_conv=False, tanh_out=True))
    assert not [k for k in model.state_dict() if "sample.conv" in k]
    model.set_precision("bf16")
    assert model.encoder.compute_dtype == torch.bfloat16 and model.decoder.compute_dtype == torch.bfloat16
    model.train(); ref.train()
    model._global_step = ref.global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    l32, log32, aux32, g32 = run_oracle(ref, batch, noise, False)
    lac, logac, auxac, gac = run_oracle(ref, batch, noise, True)
    seen, dtypes = [], []
    handles = _watch_resamplers(model, seen)
    for m in list(model.encoder.modules()) + list(model.decoder.modules()):
        if type(m).__name__ in ("Upsample", "Downsample"):
            handles.append(m.register_forward_hook(lambda mod, inp, out: dtypes.append(out.dtype)))
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0)
    for h in handles:
        h.remove()
    assert len(seen) >= 8 and all(ok for _, ok in seen), seen      # four Downsamples, four Upsamples per forward
    assert dtypes and all(d == torch.bfloat16 for d in dtypes)
    logs = model.logged_metrics
    loss.backward()
    with torch.no_grad():
        dec_obj, dec_pose, post, _ = model.forward(model._rescale(batch["patch"].to("cuda:0")))
    assert dec_obj.dtype == torch.float32 and post.parameters.dtype == torch.float32
    assert dec_obj.abs().max().item() <= 1.0

    def check(name, got, want, ac, floor):
        e, eac = rel(got, want), rel(ac, want)
        print("%s: hip %.3e autocast %.3e" % (name, e, eac))
        assert e <= 2 * eac + floor, "%s: bf16 HIP path %.3e from the f32 oracle, autocast oracle %.3e (floor %.0e)" % (name, e, eac, floor)

    check("moments", post.parameters, aux32["posterior"].parameters, auxac["posterior"].parameters, 2e-2)
    check("reconstruction", dec_obj, aux32["dec_obj"], auxac["dec_obj"], 2e-2)
    check("total loss", loss, l32, lac, 1e-2)
    for key in ("kl_loss_obj", "nll_loss", "rec_loss"):
        check(key, torch.as_tensor(float(logs["train/" + key])), torch.as_tensor(log32["train/" + key]), torch.as_tensor(logac["train/" + key]), 1e-2)
    params = dict(model.named_parameters())
    keys = [k for k in g32 if params[k].grad is not None]
    assert {k.split(".")[0] for k in keys} >= {"encoder", "decoder", "quant_conv_obj", "post_quant_conv"}
    for k in keys:
        assert params[k].grad.dtype == torch.float32 and torch.isfinite(params[k].grad).all(), k
    ghip = {k: params[k].grad.detach().cpu().float() for k in keys}
    v32, vhip, vac = flat(g32, keys), flat(ghip, keys), flat(gac, keys)
    cos = lambda a, b: (a @ b / (a.norm() * b.norm())).item()
    c_hip, c_ac = cos(vhip, v32), cos(vac, v32)
    print("gradient cosine: hip %.5f autocast %.5f" % (c_hip, c_ac))
    assert c_hip >= min(0.98, c_ac - 0.01), (c_hip, c_ac)
    energy = v32.pow(2).sum().item()
    for k in keys:
        if g32[k].double().pow(2).sum().item() < 1e-3 * energy:
            continue
        e, eac = rel(ghip[k], g32[k]), rel(gac[k], g32[k])
        assert e <= 2 * eac + 5e-2, "grad %s: hip %.3e autocast %.3e" % (k, e, eac)
    assert ops.GN_FUSED_STATS


def test_runner_trains_and_checkpoints_the_convless_network(hip_lib, tmp_path):
    """`python -m odvae_amd.run` on the untouched yaml with the two dotlist overrides: finite losses, a checkpoint with fewer keys that loads
    back strictly, and reloaded weights that reproduce the next step's loss (and a decode) bit for bit."""
    from odvae_amd import run, synthetic
    from odvae_amd.trainer import Trainer
    args = ["-b", YAML, "--height", "64", "model.params.ddconfig.ch=32", "data.params.batch_size=2",
            "model.params.ddconfig.resamp_with_conv=False", "model.params.ddconfig.tanh_out=True"]
    model = run.main(args + ["--steps", "2"])
    assert model.global_step == 4
    assert not model.encoder.down[0].downsample.with_conv and not model.decoder.up[1].upsample.with_conv and model.decoder.tanh_out is True
    logs = model.logged_metrics
    assert torch.isfinite(logs["train/total_loss"]) and torch.isfinite(logs["train/disc_loss"])
    trainer = Trainer(model, gradient_clip_val=1.0)
    path = trainer.save_checkpoint(os.path.join(tmp_path, "convless.ckpt"))
    sd = torch.load(path, map_location="cpu")["state_dict"]
    default = run.main(["-b", YAML, "--height", "64", "--steps", "0", "model.params.ddconfig.ch=32", "data.params.batch_size=2"])
    gone = set(default.state_dict()) - set(sd)
    assert len(gone) == 16 and all("sample.conv." in k for k in gone) and not set(sd) - set(default.state_dict())
    again = run.main(args + ["--steps", "0"])
    with torch.no_grad():
        for p in again.parameters():
            p.add_(0.25)
    res = Trainer(again, gradient_clip_val=1.0).load_checkpoint(path, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert again.global_step == model.global_step
    batch = synthetic.make_batch(2, 64, seed=31)
    noise = synthetic.make_noise(2, 4, seed=32)
    z = torch.randn(2, 16, 4, 4, generator=torch.Generator().manual_seed(33)).to("cuda:0")
    losses, images = [], []
    for m in (model, again):
        m.train()
        m.injected_noise = noise
        losses.append(m.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0).detach())
        with torch.no_grad():
            images.append(m.decode(z))
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])
    assert torch.equal(images[0], images[1]) and images[0].abs().max().item() <= 1.0
