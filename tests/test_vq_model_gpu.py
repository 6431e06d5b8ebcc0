"""VectorQuantizer, VQLPIPSWithDiscriminator and VQModel on the HIP path against tests/vq_ref.py (the literal CPU restatement of upstream, in
float64), with the geometry of plain_vae_ref.small_ddconfig, double_z off, n_embed = 64, embed_dim = 4.

Bounds: those of tests/test_plain_vae_gpu.py, which holds the same encoder, decoder, discriminator and LPIPS-style net to the same kind
of restatement (4 x the worst figure measured there; profiles/plain_vae.md).  The quantiser adds no rounding of its own to z_q (codebook
rows, copied) and one rounding to the loss, dz and dE.  The device's indices are required to EQUAL the restatement's: tests/test_vq_ref.py
shows that no row of the seed used here can change its code under a latent error of TOL_MODEL_OUT.
"""
import os

import numpy as np
import pytest
import torch

import vq_inputs as V
import vq_ref as R
from test_plain_vae_gpu import (TOL_CURVE, TOL_LOSS_GRAD, TOL_LOSS_GRAD_D, TOL_LOSS_OUT, TOL_MODEL_GRAD, TOL_MODEL_OUT, TOL_ONE_PASS, Worst,
                                compare_param_grads, grad_rel, loss_tensors, quiet, rel)
from test_vq_ref import BATCH_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
VQ_YAML = os.path.join(GOLDEN, "autoencoder_vq_plain.yaml")
TOL_VQ = 4 * 2.0 ** -24 * 8      # quantiser alone against float64: a handful of f32 roundings on values compared relative to the largest entry


def pair(**kw):
    model, ref = R.build_pair(**kw)
    return model.to(DEV), ref


# ---- the quantiser under autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_quantizer_matches_the_literal_form(hip_lib, legacy, layout):
    from odvae_amd.quantize import VectorQuantizer
    g = torch.Generator().manual_seed(7)
    n, d, h, w, k = 3, 4, 9, 7, 64
    q = VectorQuantizer(k, d, 0.25, sane_index_shape=True, legacy=legacy)
    with torch.no_grad():
        q.embedding.weight.copy_(0.7 * torch.randn(k, d, generator=g))
    ref = R.VectorQuantizerRef(k, d, 0.25, sane_index_shape=True, legacy=legacy).double()
    ref.load_state_dict(q.state_dict())
    q = q.to(DEV)
    z0 = torch.randn(n, d, h, w, generator=g)
    gq = torch.randn(n, d, h, w, generator=g)
    gap = torch.topk(ref.distances(z0.double()), 2, dim=1, largest=False).values
    assert (gap[:, 1] - gap[:, 0]).min().item() > 1e-4       # no row near a tie: f32 and float64 must agree on every index
    z = z0.to(DEV)
    if layout == "nhwc":
        z = z.contiguous(memory_format=torch.channels_last)
    z.requires_grad_(True)
    zr = z0.double().requires_grad_(True)
    z_q, loss, (a, b, idx) = q(z)
    zq_r, loss_r, (_, _, idx_r) = ref(zr)
    assert a is None and b is None and idx.shape == (n, h, w) and idx.dtype == torch.int64 and z_q.shape == z.shape and loss.dim() == 0
    assert torch.equal(idx.cpu(), idx_r)
    assert torch.equal(z_q.detach().cpu(), q.embedding.weight.detach().cpu()[idx.cpu()].permute(0, 3, 1, 2))       # codebook rows, in bits
    (z_q * gq.to(DEV)).sum().add(1.5 * loss).backward()
    (zq_r * gq.double()).sum().add(1.5 * loss_r).backward()
    worst = Worst("quantizer legacy=%s %s" % (legacy, layout))
    worst("loss", rel(loss, loss_r))
    worst("dz", rel(z.grad, zr.grad))
    worst("dE", rel(q.embedding.weight.grad, ref.embedding.weight.grad))
    unused = np.setdiff1d(np.arange(k), idx_r.reshape(-1).numpy())
    assert len(unused) > 0 and (q.embedding.weight.grad[torch.tensor(unused, device=DEV)] == 0).all().item()
    entry = q.get_codebook_entry(idx.reshape(-1), (n, h, w, d))
    assert entry.shape == (n, d, h, w) and torch.equal(entry, z_q.detach())
    rows = q.get_codebook_entry(idx.reshape(-1), None)
    assert torch.equal(rows, q.embedding.weight.detach()[idx.reshape(-1)])
    with torch.no_grad():       # forward only under no_grad
        out = q(z.detach())
    assert not out[0].requires_grad and torch.equal(out[2][2], idx)
    flat = VectorQuantizer(k, d, 0.25, legacy=legacy).to(DEV)
    flat.load_state_dict(q.state_dict())
    assert flat(z.detach())[2][2].shape == (n * h * w,)
    worst.check({"": TOL_VQ})


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def loss_pair(disc_loss="hinge", perceptual_weight=1.0, disc_factor=1.0, disc_start=10, n_classes=64):
    from odvae_amd import synthetic
    from odvae_amd.losses import VQLPIPSWithDiscriminator
    from test_plain_vae_gpu import liven_discriminator
    kw = dict(disc_start=disc_start, codebook_weight=0.7, disc_weight=0.5, disc_loss=disc_loss, perceptual_weight=perceptual_weight,
              disc_factor=disc_factor, n_classes=n_classes)
    loss = VQLPIPSWithDiscriminator(**kw)

    class Holder(torch.nn.Module):
        def __init__(self, loss):
            super().__init__()
            self.loss = loss
    synthetic.fill_state_procedural(Holder(loss), seed=23)
    liven_discriminator(loss.discriminator)
    ref = R.VQLossRef(**kw).double()
    ref.load_state_dict(loss.state_dict(), strict=True)
    return loss.to(DEV), ref


def evaluate(loss_mod, x, xr, optimizer_idx, global_step, dtype, device, indices):
    for p in loss_mod.discriminator.parameters():
        p.requires_grad_(optimizer_idx == 1)
    leaf = xr.to(device=device, dtype=dtype).requires_grad_()
    gain = torch.ones(3, device=device, dtype=dtype, requires_grad=True)
    cb = torch.tensor(0.375, device=device, dtype=dtype, requires_grad=True)
    rec = leaf * gain.view(1, 3, 1, 1)
    loss_mod.zero_grad(set_to_none=True)
    total, log = loss_mod(cb * 2.0, x.to(device=device, dtype=dtype), rec, optimizer_idx, global_step, last_layer=gain,
                          predicted_indices=indices.to(device))
    grads = {}
    if total.requires_grad:
        total.backward()
        grads = {"reconstruction": leaf.grad, "codebook_loss": cb.grad}
        grads.update({"D." + n: p.grad for n, p in loss_mod.discriminator.named_parameters()})
        grads = {k: v for k, v in grads.items() if v is not None}
    return total.detach(), log, grads


@pytest.mark.parametrize("disc_factor", [1.0, 0.0], ids=["disc-on", "disc-off"])
@pytest.mark.parametrize("perceptual_weight", [1.0, 0.0], ids=["lpips", "l1-only"])
@pytest.mark.parametrize("disc_loss", ["hinge", "vanilla"])
def test_loss_matches_the_restatement(hip_lib, disc_loss, perceptual_weight, disc_factor):
    ctx = quiet()
    loss, ref = loss_pair(disc_loss, perceptual_weight, disc_factor)
    loss.log_exact_g_loss = True
    x, xr, _, _ = loss_tensors()
    indices = torch.randint(0, 40, (512,), generator=torch.Generator().manual_seed(3))
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    worst = Worst("vq loss %s pw=%g df=%g" % (disc_loss, perceptual_weight, disc_factor))
    seen = set()
    for training in (True, False):
        for optimizer_idx in (0, 1):
            for global_step in (9, 10):
                where = "%s opt%d step%d" % ("train" if training else "eval", optimizer_idx, global_step)
                loss.train(training); ref.train(training)
                loss.discriminator.load_state_dict(d_state); ref.discriminator.load_state_dict(d_state)
                got = evaluate(loss, x, xr, optimizer_idx, global_step, torch.float32, DEV, indices)
                want = evaluate(ref, x, xr, optimizer_idx, global_step, torch.float64, "cpu", indices)
                worst("out total", rel(got[0], want[0]), where)
                assert set(got[1]) == set(want[1]), (where, sorted(set(got[1]) ^ set(want[1])))
                seen |= set(got[1])
                for k in want[1]:
                    worst("out " + k.split("/")[1], abs(float(got[1][k]) - float(want[1][k])) / max(1.0, abs(float(want[1][k]))), where)
                assert set(got[2]) == set(want[2]), (where, sorted(set(got[2]) ^ set(want[2])))
                for group in ("reconstruction", "codebook_loss", "D."):
                    names = [k for k in want[2] if k.startswith(group)]
                    if names:
                        scale = max(want[2][k].abs().max().item() for k in names)
                        for k in names:
                            worst("grad " + group.rstrip("."), grad_rel(got[2][k], want[2][k], scale), where + " " + k)
                if optimizer_idx == 0:
                    assert float(want[2]["codebook_loss"]) == pytest.approx(2.0 * 0.7)
                    assert (float(want[1]["train/d_weight"]) > 0) == (disc_factor > 0)
                    assert float(got[1]["train/cluster_usage"]) == float(want[1]["train/cluster_usage"]) == indices.unique().numel()
    assert seen == {"train/" + k for k in ("total_loss", "quant_loss", "nll_loss", "rec_loss", "p_loss", "d_weight", "disc_factor", "g_loss",
                                           "perplexity", "cluster_usage", "disc_loss", "logits_real", "logits_fake")}
    ctx.__exit__(None, None, None)
    worst.check({"out": TOL_LOSS_OUT, "grad reconstruction": TOL_LOSS_GRAD, "grad codebook_loss": TOL_LOSS_GRAD, "grad D": TOL_LOSS_GRAD_D})


def test_loss_one_pass_shortcut_and_optional_usage(hip_lib):
    ctx = quiet()
    x, xr, _, _ = loss_tensors()
    indices = torch.randint(0, 64, (512,), generator=torch.Generator().manual_seed(4))
    loss, _ = loss_pair()
    loss.train()
    d_state = {k: v.clone() for k, v in loss.discriminator.state_dict().items()}
    out = {}
    for one_pass in (True, False):
        loss.ONE_PASS = one_pass
        loss.discriminator.load_state_dict(d_state)
        out[one_pass] = evaluate(loss, x, xr, 0, 10, torch.float32, DEV, indices)
    del loss.ONE_PASS
    assert type(loss).ONE_PASS is True
    a, b = out[True], out[False]
    worst = Worst("vq loss: one pass vs three passes")
    worst("total", rel(a[0], b[0]))
    for k in b[1]:
        worst(k, abs(float(a[1][k]) - float(b[1][k])) / max(1.0, abs(float(b[1][k]))))
    assert set(a[2]) == set(b[2]) == {"reconstruction", "codebook_loss"}
    for k in b[2]:
        worst("grad " + k, rel(a[2][k], b[2][k]))
    # disc_factor == 0: the discriminator does not run, g_loss logs 0, nothing else changes against the exact form
    off, _ = loss_pair(disc_factor=0.0)
    off.train()
    d0 = {k: v.clone() for k, v in off.discriminator.state_dict().items()}
    short = evaluate(off, x, xr, 0, 10, torch.float32, DEV, indices)
    assert all(torch.equal(v, d0[k].to(DEV)) for k, v in off.discriminator.state_dict().items())
    off.log_exact_g_loss = True
    exact = evaluate(off, x, xr, 0, 10, torch.float32, DEV, indices)
    assert float(short[1]["train/g_loss"]) == 0.0 and float(exact[1]["train/g_loss"]) != 0.0 and torch.equal(short[0], exact[0])
    assert all(torch.equal(short[2][k], exact[2][k]) for k in exact[2])
    # without n_classes the two usage figures are not logged, with or without indices
    plain, _ = loss_pair(n_classes=None)
    plain.train()
    log = evaluate(plain, x, xr, 0, 10, torch.float32, DEV, indices)[1]
    assert "train/perplexity" not in log and "train/cluster_usage" not in log and "train/quant_loss" in log
    ctx.__exit__(None, None, None)
    worst.check({"": TOL_ONE_PASS})


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def test_training_step_matches_the_restatement(hip_lib):
    from odvae_amd import synthetic
    ctx = quiet()
    model, ref = pair()
    model.train(); ref.train()
    batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED)
    model._global_step = ref.global_step = 1
    worst = Worst("vq training_step")
    d_state = {k: v.clone() for k, v in model.loss.discriminator.state_dict().items()}
    for optimizer_idx in (0, 1):
        model.loss.discriminator.load_state_dict(d_state); ref.loss.discriminator.load_state_dict(d_state)
        for m in (model, ref):
            for n, p in m.named_parameters():
                if not n.startswith("loss.perceptual_loss"):
                    p.requires_grad_(n.startswith("loss.discriminator") == (optimizer_idx == 1))
            m.zero_grad(set_to_none=True)
        loss = model.training_step(dict(batch), 0, optimizer_idx)
        loss_ref, log_ref, aux = ref.training_step(batch, optimizer_idx)
        logs = dict(model.logged_metrics)
        where = "opt%d" % optimizer_idx
        worst("out total", rel(loss, loss_ref), where)
        for k in log_ref:
            worst("out " + k.split("/")[1], abs(float(logs[k]) - float(log_ref[k])) / max(1.0, abs(float(log_ref[k]))), where)
        if optimizer_idx == 0:
            with torch.no_grad():
                xrec, qloss, ind = model(model.get_input(batch, "image"), return_pred_indices=True)
                h = model.encode_to_prequant(model.get_input(batch, "image"))
            assert torch.equal(ind.cpu(), aux["indices"]), "%d indices differ" % (ind.cpu() != aux["indices"]).sum().item()
            diff_ref = aux["reconstructions"] - aux["inputs"]
            assert (torch.sign(xrec.cpu().double() - aux["inputs"]) != torch.sign(diff_ref)).sum().item() == 0      # no L1 sign in doubt
            worst("out reconstruction", rel(xrec, aux["reconstructions"]), where)
            worst("out latent", rel(h, ref.encode_to_prequant(aux["inputs"]).detach()), where)
            worst("out qloss", rel(qloss, aux["qloss"]), where)
            assert float(log_ref["train/d_weight"]) > 0 and "train/perplexity" in log_ref
        loss.backward(); loss_ref.backward()
        compared = compare_param_grads(worst, model, ref, where)
        want = {"encoder", "decoder", "quantize", "quant_conv", "post_quant_conv"} if optimizer_idx == 0 else {"loss.discriminator"}
        assert compared == want, compared
        if optimizer_idx == 0:
            ge, ge_ref = model.quantize.embedding.weight.grad.cpu(), ref.quantize.embedding.weight.grad
            unused = np.setdiff1d(np.arange(R.N_EMBED), aux["indices"].numpy())
            assert len(unused) > 0 and (ge[unused] == 0).all() and (ge_ref[unused] == 0).all()
            assert ge.abs().max() > 0
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT, grad=TOL_MODEL_GRAD)


def ref_optimizer_step(ref, opts, batch, idx, indices, clip=1.0):
    """one optimizer's share of plain_vae_ref.train_batch -- forward, zero_grad, backward, clip, step -- with the restatement's quantiser
    taking `indices` in place of its own argmin; returns the loss and the argmin it would have taken"""
    opt = opts[idx]
    others = [p for j, o in enumerate(opts) if j != idx for g in o.param_groups for p in g["params"]]
    for p in others:
        p.requires_grad = False
    ref.quantize.forced_indices = indices
    loss, _, aux = ref.training_step(batch, idx)
    ref.quantize.forced_indices = None
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip)
    opt.step()
    for p in others:
        p.requires_grad = True
    ref.global_step += 1
    return loss.detach(), ref.quantize.natural_indices


def test_three_batches_under_adam_with_clipping(hip_lib):
    """Three batches, two optimizers, clip 1.0, against the same loop on the restatement with torch.optim.Adam, as
    tests/test_plain_vae_gpu.py holds the plain model: all six losses to TOL_CURVE and every trained weight to 2.2 lr per step + 5e-3 of the
    tensor's largest entry.  Only the first forward is gap-checked (tests/test_vq_ref.py), and there the device's indices must equal the
    restatement's own.  Once the weights have moved a row may sit on a decision boundary, so from then on the reference is taken AT THE
    DEVICE'S INDICES (the restatement's quantiser is handed them, as the C-ABI tests on Gaussian operands do): no discontinuity in the
    reference, nothing left out of the comparison.  At every forward the device's indices must pass the acceptance rule of
    tests/vq_inputs.py on the device's own latent and codebook; how many rows the restatement's argmin would have placed elsewhere is
    printed."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, ref = pair()
    model.train(); ref.train()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
    ref_opts = ref.configure_optimizers()
    worst = Worst("vq three batches")
    moved = []
    for step in range(3):
        batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED + step)
        for idx in (0, 1):
            with torch.no_grad():
                x = model.get_input(batch, "image")
                ind = model(x, return_pred_indices=True)[2].cpu()
                h_rows = model.encode_to_prequant(x).permute(0, 2, 3, 1).reshape(-1, R.EMBED_DIM).cpu().numpy()
                codes = model.quantize.embedding.weight.detach().cpu().numpy()
            # the device's indices under the acceptance rule of tests/vq_inputs.py, on the device's own latent and codebook
            assert len(V.index_violations(h_rows, codes, ind.numpy())[0]) == 0, (step, idx)
            trainer.optimizer_indices = (idx,)
            got = trainer.training_batch(dict(batch), step)[0]
            want, natural = ref_optimizer_step(ref, ref_opts, batch, idx, ind)
            differ = (ind != natural).nonzero().reshape(-1)
            moved.append(differ.numel())
            if step == 0 and idx == 0:
                assert differ.numel() == 0, "the gap-checked forward: %d indices differ" % differ.numel()
            worst("loss", rel(got, want), "batch %d opt%d" % (step, idx))
    print("vq three batches: rows placed elsewhere by the restatement's own argmin, per forward: %s" % moved)
    assert model.global_step == ref.global_step == 6
    ref_sd = ref.state_dict()
    lr = model.learning_rate
    trained = {k for k, _ in model.named_parameters()}      # (BatchNorm's running statistics are sums of activations: no lr bounds them)
    checked = 0
    for k, v in model.state_dict().items():
        if k in trained and k.startswith(("encoder", "decoder", "quant", "post_quant", "loss.discriminator")):
            diff = (v.detach().cpu().double() - ref_sd[k]).abs().max().item()
            assert diff <= 2.2 * lr * 3 + 5e-3 * ref_sd[k].abs().max().item(), (k, diff)
            checked += 1
    assert checked > 50
    ctx.__exit__(None, None, None)
    worst.check(loss=TOL_CURVE)


@pytest.mark.parametrize("use_ema", [False, True])
def test_validation_step(hip_lib, use_ema):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, ref = pair(use_ema=use_ema)
    model.train(); ref.eval()
    model.loss.log_exact_g_loss = True
    batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED)
    trainer = Trainer(model, gradient_clip_val=1.0)
    metrics = trainer.validate([dict(batch)])
    with torch.no_grad():
        want = ref.validation_step(batch)
    keys = {"val/" + k for k in ("total_loss", "quant_loss", "nll_loss", "rec_loss", "p_loss", "d_weight", "disc_factor", "g_loss", "perplexity",
                                 "cluster_usage", "disc_loss", "logits_real", "logits_fake", "aeloss")}
    assert set(want) == keys
    assert set(metrics) == keys | ({k.replace("val/", "val_ema/") for k in keys} if use_ema else set())
    worst = Worst("vq validate ema=%s" % use_ema)
    for k in want:
        worst("out " + k.split("/")[1], abs(float(metrics[k]) - float(want[k])) / max(1.0, abs(float(want[k]))))
        if use_ema:      # no update yet: the averaged weights are the weights
            assert float(metrics[k.replace("val/", "val_ema/")]) == pytest.approx(float(metrics[k]), rel=1e-5, abs=1e-6), k
    assert model.training and not model._in_ema_scope
    if use_ema:
        # past the first update: on_train_batch_end moves the average (decay (1 + n) / (10 + n) = 2 / 11 at the first update), validation runs
        # under both sets of weights and leaves the trained ones exactly as they were
        trainer.training_batch(dict(batch), 0)
        assert int(model.model_ema.num_updates) == 1
        before = {k: v.clone() for k, v in model.state_dict().items()}
        again = trainer.validate([dict(batch)])
        assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items() if not k.startswith("loss.discriminator")), "ema_scope left other weights behind"
        assert all(torch.isfinite(torch.as_tensor(v)).all() for v in again.values())
        assert float(again["val_ema/rec_loss"]) != float(again["val/rec_loss"]) and float(again["val_ema/quant_loss"]) != float(again["val/quant_loss"])
        assert not model._in_ema_scope
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT)


def test_log_images_decode_code_and_interface(hip_lib):
    from odvae_amd import synthetic
    from odvae_amd.autoencoder import VQModelInterface
    ctx = quiet()
    model, ref = pair(use_ema=True)
    model.eval(); ref.eval()
    batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED)
    got, want = model.log_images(dict(batch)), ref.log_images(batch)
    assert set(got) == set(want) == {"inputs", "reconstructions"}
    worst = Worst("vq log_images")
    for k in want:
        assert got[k].shape == (2, 3, 32, 32) and got[k].is_cuda and not got[k].requires_grad, k
        worst("out " + k, rel(got[k], want[k]))
    assert list(model.log_images(dict(batch), only_inputs=True)) == ["inputs"]
    ema = model.log_images(dict(batch), plot_ema=True)
    assert set(ema) == {"inputs", "reconstructions", "reconstructions_ema"} and torch.equal(ema["reconstructions_ema"], ema["reconstructions"])
    with torch.no_grad():
        x = model.get_input(batch, "image")
        quant, emb_loss, (_, _, ind) = model.encode(x)
        dec = model.decode(quant)
        assert torch.equal(model.decode_code(ind.reshape(2, 16, 16)), dec)
        worst("out decode_code", rel(model.decode_code(ind.reshape(2, 16, 16)), ref.decode_code(ind.cpu().reshape(2, 16, 16))))
        # the inference face: encode stops before the quantiser, decode quantises (unless told not to)
        p = dict(ddconfig=R.small_vq_ddconfig(R.EMBED_DIM), lossconfig={"target": "odvae_amd.losses.VQLPIPSWithDiscriminator",
                                                                          "params": dict(R.LOSS_KW)}, n_embed=R.N_EMBED)
        face = VQModelInterface(R.EMBED_DIM, **p)
        face.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("model_ema.")})
        face = face.to(DEV).eval()
        h = face.encode(x)
        assert torch.equal(h, model.encode_to_prequant(x))
        assert torch.equal(face.decode(h), dec)
        assert torch.equal(face.decode(quant, force_not_quantize=True), dec)
    ctx.__exit__(None, None, None)
    worst.check(out=TOL_MODEL_OUT)


def test_checkpoint_round_trip_with_the_restatement(hip_lib, tmp_path):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    ctx = quiet()
    model, ref = pair()
    model.train()
    trainer = Trainer(model, gradient_clip_val=1.0)
    batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED)
    trainer.training_batch(dict(batch), 0)
    path = trainer.save_checkpoint(str(tmp_path / "vq.ckpt"))
    saved = torch.load(path, map_location="cpu")["state_dict"]
    assert tuple(saved["quantize.embedding.weight"].shape) == (R.N_EMBED, R.EMBED_DIM) and not any("logvar" in k for k in saved)
    res = ref.float().load_state_dict(saved, strict=True)       # the Lightning-layout checkpoint loads into the restatement ...
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(ref.quantize.embedding.weight.detach(), model.quantize.embedding.weight.detach().cpu())
    torch.save({"state_dict": ref.state_dict()}, str(tmp_path / "ref.ckpt"))      # ... and the reverse, through ckpt_path
    from odvae_amd.autoencoder import VQModel
    fresh = VQModel(R.small_vq_ddconfig(R.EMBED_DIM), {"target": "odvae_amd.losses.VQLPIPSWithDiscriminator", "params": dict(R.LOSS_KW)},
                    R.N_EMBED, R.EMBED_DIM, ckpt_path=str(tmp_path / "ref.ckpt"))
    assert all(torch.equal(v, saved[k]) for k, v in fresh.state_dict().items())
    other, _ = pair(seed=99)
    other.train()
    resumed = Trainer(other, gradient_clip_val=1.0)
    res = resumed.load_checkpoint(path)
    assert not res.missing_keys and not res.unexpected_keys and other.global_step == 2
    a = trainer.training_batch(dict(batch), 1)
    b = resumed.training_batch(dict(batch), 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ctx.__exit__(None, None, None)


def test_launcher_trains_the_vq_yaml(hip_lib, capsys):
    from odvae_amd import autoencoder, run
    ctx = quiet()
    model = run.main(["-b", VQ_YAML, "--height", "32", "--steps", "2"])
    ctx.__exit__(None, None, None)
    assert type(model) is autoencoder.VQModel and model.global_step == 4
    out = capsys.readouterr().out.splitlines()
    lines = [l for l in out if l.startswith("batch ")]
    assert len(lines) == 2
    for line in lines:
        words = line.split()
        ae, disc = float(words[words.index("aeloss") + 1]), float(words[words.index("discloss") + 1])
        assert abs(ae) < float("inf") and abs(disc) < float("inf"), line
    val = [l for l in out if l.startswith("validation ")]
    assert len(val) == 1 and "val/rec_loss" in val[0] and "val/aeloss" in val[0]
    assert model.quantize.embedding.weight.grad is None or torch.isfinite(model.quantize.embedding.weight.grad).all()
    assert all(torch.isfinite(v).all() for k, v in model.logged_metrics.items() if torch.is_tensor(v))


def test_bf16_keeps_the_quantiser_in_f32(hip_lib):
    """precision "bf16": the latent reaches the quantiser in f32, the quantiser's outputs are f32.  The f32 run's indices on the gap-checked
    seed are compared and the number of rows that differ is REPORTED: a bf16 encoder moves the latent by about 1e-2 of its largest entry, far
    more than this seed's smallest gap (a third of which a 1.2e-5 error can already move) allows for, so equality cannot be required of it."""
    from odvae_amd import synthetic
    ctx = quiet()
    model, _ = pair()
    model.eval()
    batch = synthetic.make_image_batch(2, 32, seed=BATCH_SEED)
    with torch.no_grad():
        x = model.get_input(batch, "image")
        ind32 = model(x, return_pred_indices=True)[2]
        model.set_precision("bf16")
        assert model.encoder.compute_dtype == torch.bfloat16
        h = model.encode_to_prequant(x)
        xrec, qloss, ind16 = model(x, return_pred_indices=True)
    assert h.dtype == torch.float32 and xrec.dtype == torch.float32 and qloss.dtype == torch.float32 and ind16.dtype == torch.int64
    differ = (ind16 != ind32).sum().item()
    print("bf16 against f32: %d of %d indices differ" % (differ, ind32.numel()))
    assert ((ind16 >= 0) & (ind16 < R.N_EMBED)).all().item()
    model.train()
    model.training_step(dict(batch), 0, 0).backward()
    assert model.quantize.embedding.weight.grad.dtype == torch.float32 and torch.isfinite(model.quantize.embedding.weight.grad).all()
    ctx.__exit__(None, None, None)
