"""Linear attention on the device: ops.linear_attention_qkv (linattn_f32.hip + the batched GEMM), modules.LinAttnBlock and
Encoder / Decoder / PoseAutoencoder with use_linear_attn against the torch restatement of tests/linattn_ref.py.

The core is held to the rule of tests/linattn_ref.py against float64:  |hip - f64|max <= max(8 |torch_f32 - f64|max, floor max(1, |f64|max)).
Module and network tests use the tolerances of tests/test_modules_gpu.py (outputs 1e-3, gradients 3e-3 of max|ref|: the same networks,
the same depth), the checkpoint policies are compared bit for bit as tests/test_model_gpu.py compares them, and bf16 mode follows the rule
of tests/test_bf16_model_gpu.py (no further from the f32 counterpart than twice its CPU autocast, plus that file's floors)."""
import ctypes
import os

import pytest
import torch

import linattn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
YAML = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")
DD = dict(double_z=True, z_channels=4, resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
          attn_resolutions=[8], dropout=0.0)
CORE_CASES = [(n, c, t) for n in (1, 3) for c in (32, 96, 128) for t in (1, 35, 256)]
_REFS = {}


def refs_of(n, c, t, a=0):
    """inputs and references of one case, computed once and shared"""
    key = (n, c, t, a)
    if key not in _REFS:
        q, k, v, do = R.make_qkv(n, c, t, offset=a)
        _REFS[key] = (q, k, v, do, R.core_refs(q, k, v, do))
    return _REFS[key]


def run_core(q, k, v, do):
    """dict as linattn_ref.host_model returns it, from the device"""
    from odvae_amd import ops
    n, c, t = q.shape
    qkv = R.pack(q, k, v).to(DEV).requires_grad_(True)
    o = ops.linear_attention_qkv(qkv)
    _, ctx, stats = o.grad_fn.saved_tensors
    o.backward(do.reshape(o.shape).to(DEV))
    dq, dk, dv = qkv.grad.reshape(n, 3, c, t).unbind(1)
    return dict(out=o.detach().reshape(n, c, t), ctx=ctx, m=stats[0], rinv=stats[1], dq=dq, dk=dk, dv=dv)


def rel_err(a, b):
    a = a.detach().float().cpu().double(); b = b.detach().float().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


@pytest.mark.parametrize("n,c,t", CORE_CASES, ids=lambda v: str(v))
def test_core_matches_float64(hip_lib, n, c, t):
    q, k, v, do, refs = refs_of(n, c, t)
    R.check(R.core_figures(run_core(q, k, v, do), refs), "N%d C%d T%d" % (n, c, t))


def test_core_around_the_context_split(hip_lib):
    """T one below, at and one above the context kernel's split length and at 2 split + 3: one partial, a partial of one token, three."""
    from odvae_amd import ops
    split = ops.LINATTN_CTX_SPLIT
    assert split == hip_lib.odvae_linattn_ctx_split() and split >= 32
    for t in (split - 1, split, split + 1, 2 * split + 3):
        q, k, v, do, refs = refs_of(2, 32, t)
        R.check(R.core_figures(run_core(q, k, v, do), refs), "T%d" % t)


@pytest.mark.parametrize("a", R.OFFSETS)
def test_offset_ladder(hip_lib, a):
    """k = randn + a sign_d: without the column maximum exp overflows f32 at a = 90"""
    q, k, v, do, refs = refs_of(2, 32, 64, a)
    got = run_core(q, k, v, do)
    assert all(torch.isfinite(t).all() for t in got.values())
    R.check(R.core_figures(got, refs), "offset %g" % a)


def test_one_token_is_the_outer_product(hip_lib):
    """T = 1: softmax over one token is 1, so ctx = 1 v^T, out[e] = v[e] sum_d q[d] and dk = 0, exactly representable sums aside."""
    n, c = 2, 32
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randint(-4, 5, (n, c, 1), generator=g).float() for _ in range(4))      # small integers: every sum is exact
    got = run_core(q, k + 0.37, v, do)
    ctx = v.squeeze(-1).unsqueeze(1).expand(n, c, c)
    assert torch.equal(got["ctx"].cpu(), ctx)
    assert torch.equal(got["out"].cpu(), v * q.sum(1, keepdim=True))
    assert torch.equal(got["dk"].cpu(), torch.zeros(n, c, 1))
    assert torch.equal(got["m"].cpu(), (k + 0.37).squeeze(-1)) and torch.equal(got["rinv"].cpu(), torch.ones(n, c))
    assert torch.equal(got["dv"].cpu(), do * q.sum(1, keepdim=True))
    assert torch.equal(got["dq"].cpu(), (v * do).sum(1, keepdim=True).expand(n, c, 1))


def test_two_runs_are_bit_identical(hip_lib):
    from odvae_amd import ops
    q, k, v, do, _ = refs_of(3, 96, 2 * ops.LINATTN_CTX_SPLIT + 3)
    a, b = run_core(q, k, v, do), run_core(q, k, v, do)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_strided_input_is_accepted(hip_lib):
    """an NCHW-contiguous projection (not channels_last) and a channel slice of a wider tensor give the same bits"""
    from odvae_amd import ops
    q, k, v, do, _ = refs_of(3, 32, 35)
    packed = R.pack(q, k, v).to(DEV)
    want = ops.linear_attention_qkv(packed.contiguous(memory_format=torch.channels_last))
    assert torch.equal(ops.linear_attention_qkv(packed.contiguous()), want)
    wide = torch.cat([packed, packed], dim=1)
    assert torch.equal(ops.linear_attention_qkv(wide[:, :96]), want)


def test_no_tensor_grows_with_t_squared(hip_lib):
    """N = 1, C = 64, T = 4096: a T x T f32 tensor is 64 MiB; qkv's gradient, o, dO and the workspace are about 8 MiB"""
    from odvae_amd import ops
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(1, 192, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    do = torch.randn(1, 64, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.linear_attention_qkv(qkv).backward(do)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise %.2f MiB" % (rise / 2 ** 20))
    assert rise < 16 * 2 ** 20, rise
    assert torch.isfinite(qkv.grad).all()


def test_argument_errors(hip_lib):
    """C = 48, T = 0 and null pointers: ODVAE_ERR_ARG before any launch"""
    L = hip_lib
    buf = torch.zeros(4096, device=DEV)
    p, nb = buf.data_ptr(), ctypes.c_size_t(buf.numel() * 4)
    for n, t, c in ((1, 4, 48), (1, 0, 32), (1, 4, 0), (0, 4, 32)):
        assert L.odvae_linattn_colstats_f32(p, 3 * c, t * 3 * c, n, t, c, p, p, p, nb, None) == 1, (n, t, c)
        assert L.odvae_linattn_ctx_f32(p, p, 3 * c, t * 3 * c, p, p, n, t, c, p, p, nb, None) == 1, (n, t, c)
        assert L.odvae_linattn_dkv_f32(p, p, 3 * c, t * 3 * c, p, p, p, p, n, t, c, p, p, 3 * c, t * 3 * c, None) == 1, (n, t, c)
    assert L.odvae_linattn_colstats_f32(None, 96, 96, 1, 1, 32, p, p, p, nb, None) == 1
    assert L.odvae_linattn_ctx_f32(p, None, 96, 96, p, p, 1, 1, 32, p, p, nb, None) == 1
    assert L.odvae_linattn_dkv_f32(p, p, 96, 96, p, p, p, None, 1, 1, 32, p, p, 96, 96, None) == 1
    assert L.odvae_linattn_ctx_f32(p, p, 96, 96, p, p, 1, 1, 32, p, p, ctypes.c_size_t(16), None) == 2      # workspace too small
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
    from odvae_amd import lib, ops
    with pytest.raises(lib.HipLibraryError):
        ops.linear_attention_qkv(torch.zeros(1, 3 * 48, 2, 2, device=DEV))
    with pytest.raises(lib.HipLibraryError):
        ops.linear_attention_qkv(torch.zeros(1, 96, 2, 2))          # no CPU fallback


# ------------------------------------------------------------------------------------------------------------------------------
# module and network level
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w", [(32, 5, 7), (64, 16, 16)])
def test_lin_attn_block_matches_reference_module(hip_lib, c, h, w):
    from odvae_amd import modules
    torch.manual_seed(11)
    ref = R.LinAttnBlock(c)
    net = modules.LinAttnBlock(c)
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(2, c, h, w, generator=g), torch.randn(2, c, h, w, generator=g)
    refs = R.module_refs(ref, x, dy)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    y.backward(dy.to(DEV))
    figs = [R.figure("y", y, refs[64][0], refs[32][0], R.FLOOR_FWD), R.figure("dx", xd.grad, refs[64][1], refs[32][1], R.FLOOR_DX)]
    figs += [R.figure("d " + k, p.grad, refs[64][2][k], refs[32][2][k], R.FLOOR_PARAM) for k, p in net.named_parameters()]
    assert len(figs) == 5
    R.check(figs, "LinAttnBlock C%d %dx%d" % (c, h, w))


def _net_inputs(which):
    g = torch.Generator().manual_seed(1)
    return torch.randn(2, 3, 16, 16, generator=g) if which == "encoder" else torch.randn(2, 4, 8, 8, generator=g)


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_encoder_decoder_with_linear_attention_match_counterpart(hip_lib, which):
    from odvae_amd import modules
    from oracle import ldm_model
    torch.manual_seed(23)
    ref = R.linearize(getattr(ldm_model, which.capitalize())(**DD))
    net = getattr(modules, which.capitalize())(use_linear_attn=True, **DD)
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    x = _net_inputs(which)
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    gy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(2))
    y_ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    assert tuple(y.shape) == tuple(y_ref.shape)
    assert rel_err(y, y_ref) < 1e-3, "forward rel err %.3e" % rel_err(y, y_ref)
    y.backward(gy.to(DEV))
    assert rel_err(xd.grad, xr.grad) < 3e-3, "input grad rel err %.3e" % rel_err(xd.grad, xr.grad)
    ref_params = dict(ref.named_parameters())
    scale = max(p.grad.abs().max().item() for p in ref_params.values())
    worst = ("", 0.0)
    for name, p in net.named_parameters():
        r = ref_params[name].grad.double()
        e = (p.grad.detach().cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, (name, e), key=lambda v: v[1])
    print("%s: forward %.3e, dx %.3e, worst parameter gradient %s %.3e" % (which, rel_err(y, y_ref), rel_err(xd.grad, xr.grad), *worst))
    assert ref_params["mid.attn_1.to_qkv.weight"].grad.abs().max().item() > 0
    assert worst[1] < 3e-3, "param grad %s rel err %.3e" % worst


@pytest.mark.parametrize("dropout", [0.0, 0.25], ids=["nodrop", "drop"])
def test_decoder_checkpoint_policies_are_bit_identical(hip_lib, dropout):
    """activation_checkpoint False / "unit" / "norm" run the same kernels on the same values (with ResnetBlock dropout: the same seeds)"""
    from odvae_amd import modules
    dd = dict(DD, dropout=dropout)
    torch.manual_seed(23)
    nets = {pol: modules.Decoder(use_linear_attn=True, activation_checkpoint=pol, **dd) for pol in (False, "unit", "norm")}
    for pol in ("unit", "norm"):
        nets[pol].load_state_dict(nets[False].state_dict())
    z, outs = _net_inputs("decoder").to(DEV), {}
    for pol, net in nets.items():
        net = net.to(DEV).train()
        torch.manual_seed(77)                # the dropout seeds come from torch's default CPU generator
        zd = z.clone().requires_grad_(True)
        y = net(zd)
        y.backward(torch.ones_like(y) * 0.5)
        outs[pol] = (y.detach(), zd.grad, {k: p.grad for k, p in net.named_parameters()})
    assert outs[False][2]["mid.attn_1.to_qkv.weight"].abs().max().item() > 0
    for pol in ("unit", "norm"):
        assert torch.equal(outs[pol][0], outs[False][0]) and torch.equal(outs[pol][1], outs[False][1]), pol
        for k, gr in outs[pol][2].items():
            assert torch.equal(gr, outs[False][2][k]), (pol, k)


def build_linear_pair(latent_hw=4, ch=32):
    """tests/test_model_gpu.py build_pair with ddconfig.use_linear_attn: the HIP PoseAutoencoder from the yaml and the oracle with its
    attention members replaced by the reference LinAttnBlock, on the same weights"""
    from odvae_amd import modules, synthetic
    from odvae_amd.config import instantiate_from_config
    from oracle.autoencoder import PoseAutoencoder as OraclePA
    torch.manual_seed(23)
    mcfg, cfg = synthetic.model_config(YAML, latent_hw=latent_hw, ch=ch, perceptual_weight=0.0, disc_factor=0.0, phase="vae")
    mcfg.params.ddconfig["use_linear_attn"] = True
    model = instantiate_from_config(mcfg)
    assert isinstance(model.encoder.mid.attn_1, modules.LinAttnBlock) and isinstance(model.decoder.up[2].attn[0], modules.LinAttnBlock)
    model.learning_rate = 12 * cfg.model.base_learning_rate
    p = mcfg.params.to_container()
    ref = OraclePA(p["ddconfig"], dict(p["lossconfig"]["params"]), p["embed_dim"], p["pose_decoder_config"]["params"],
                   p["pose_encoder_config"]["params"], feat_dims=p.get("feat_dims", [16, 16, 16]), dropout_prob_init=p["dropout_prob_init"],
                   dropout_prob_final=p["dropout_prob_final"], dropout_warmup_steps=p["dropout_warmup_steps"],
                   pose_conditioned_generation_steps=p["pose_conditioned_generation_steps"],
                   add_noise_to_z_obj=p["add_noise_to_z_obj"], train_on_yaw=p["train_on_yaw"])
    R.linearize(ref.encoder); R.linearize(ref.decoder)
    res = ref.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ref.learning_rate = model.learning_rate
    return model.to(DEV), ref


def test_training_step_with_linear_attention_matches_counterpart(hip_lib):
    """One PoseAutoencoder (AutoencoderKL) training step from the yaml with use_linear_attn: every loss term, latent, reconstruction and
    every gradient; tolerances of the module tests above (the same network depth)."""
    from test_model_gpu import check_step
    model, ref = build_linear_pair()
    check_step(model, ref, 1, height=64, latent_hw=4, tol_out=1e-3, tol_grad=3e-3)


def test_bf16_step_with_linear_attention_is_as_close_to_f32_as_autocast(hip_lib):
    """the rule of tests/test_bf16_model_gpu.py on the linear-attention counterpart"""
    from test_bf16_model_gpu import flat, rel, run_oracle
    from odvae_amd import synthetic
    model, ref = build_linear_pair()
    model.set_precision("bf16")
    model.train(); ref.train()
    model._global_step = ref.global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    l32, log32, aux32, g32 = run_oracle(ref, batch, noise, False)
    lac, logac, auxac, gac = run_oracle(ref, batch, noise, True)
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0)
    logs = model.logged_metrics
    loss.backward()
    with torch.no_grad():
        dec_obj, _, post, _ = model.forward(model._rescale(batch["patch"].to(DEV)))

    def check(name, got, want, ac, floor):
        e, eac = rel(got, want), rel(ac, want)
        print("%s: hip %.3e autocast %.3e" % (name, e, eac))
        assert e <= 2 * eac + floor, "%s: bf16 HIP path %.3e from the f32 counterpart, autocast %.3e (floor %.0e)" % (name, e, eac, floor)

    check("moments", post.parameters, aux32["posterior"].parameters, auxac["posterior"].parameters, 2e-2)
    check("reconstruction", dec_obj, aux32["dec_obj"], auxac["dec_obj"], 2e-2)
    check("total loss", loss, l32, lac, 1e-2)
    for key in ("kl_loss_obj", "nll_loss", "rec_loss"):
        check(key, torch.as_tensor(float(logs["train/" + key])), torch.as_tensor(log32["train/" + key]), torch.as_tensor(logac["train/" + key]), 1e-2)
    params = dict(model.named_parameters())
    keys = [k for k in g32 if params[k].grad is not None]
    assert any(".to_qkv." in k for k in keys)
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


def test_checkpoint_round_trip_with_the_counterpart(hip_lib, tmp_path):
    """a checkpoint saved here loads (strict) into the counterpart, and one written from the counterpart loads back"""
    from odvae_amd.trainer import Trainer
    model, ref = build_linear_pair()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
    path = trainer.save_checkpoint(os.path.join(tmp_path, "last.ckpt"))
    sd = torch.load(path, map_location="cpu")["state_dict"]
    assert "encoder.mid.attn_1.to_qkv.weight" in sd and "encoder.mid.attn_1.to_qkv.bias" not in sd and "encoder.mid.attn_1.norm.weight" not in sd
    with torch.no_grad():
        for p in ref.parameters():
            p.normal_()
    res = ref.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(ref.decoder.mid.attn_1.to_out.bias, model.decoder.mid.attn_1.to_out.bias.detach().cpu())
    with torch.no_grad():
        for p in ref.parameters():
            p.mul_(0.5)
    back = os.path.join(tmp_path, "ref.ckpt")
    torch.save({"epoch": 0, "global_step": 0, "pytorch-lightning_version": "1.9.0", "state_dict": ref.state_dict()}, back)   # weights only
    res = trainer.load_checkpoint(back)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k].cpu(), v), k
