"""PatchGAN / LPIPS-style kernels and modules vs torch CPU fp32 (oracle/losses.py modules with the same state_dict).
Tolerances: per-op forward 2e-4, backward 5e-4 (relative to max|ref|); whole networks 1e-3 / 5e-3."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(a, b, tol, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    ref = max(1e-6, b.abs().max().item())
    assert err <= tol * ref, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, ref)


@pytest.mark.parametrize("n,cin,cout,h,w,stride,bias", [(2, 3, 64, 32, 32, 2, True), (2, 64, 128, 16, 16, 2, False),
                                                        (1, 32, 64, 9, 7, 1, False), (2, 64, 1, 8, 8, 1, True)])
def test_conv4x4(hip_lib, n, cin, cout, h, w, stride, bias):
    from odvae_amd import ops
    g = torch.Generator().manual_seed(cin * cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 4, 4, generator=g) / math.sqrt(16 * cin)
    b = torch.randn(cout, generator=g) if bias else None
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    y_ref = F.conv2d(xr, wr, br, stride=stride, padding=1)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    xd, wd = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.conv4x4(xd, wd, bd, stride)
    close(y, y_ref, 2e-4, "conv4x4 fwd")
    y.backward(gy.to(DEV))
    close(xd.grad, xr.grad, 5e-4, "conv4x4 dx")
    close(wd.grad, wr.grad, 5e-4, "conv4x4 dw")
    if bias:
        close(bd.grad, br.grad, 5e-4, "conv4x4 db")


@pytest.mark.parametrize("train", [True, False])
def test_batchnorm_lrelu(hip_lib, train):
    from odvae_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 128, 6, 5, generator=g) * 2 + 1
    bn_ref = torch.nn.BatchNorm2d(128)
    with torch.no_grad():
        bn_ref.weight.copy_(torch.randn(128, generator=g)); bn_ref.bias.copy_(torch.randn(128, generator=g))
        bn_ref.running_mean.copy_(torch.randn(128, generator=g) * 0.1); bn_ref.running_var.copy_(torch.rand(128, generator=g) + 0.5)
    import copy
    bn = copy.deepcopy(bn_ref).to(DEV)
    bn_ref.train(train); bn.train(train)
    xr = x.clone().requires_grad_(True)
    y_ref = F.leaky_relu(bn_ref(xr), 0.2)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.batchnorm_lrelu(xd, bn, 0.2)
    close(y, y_ref, 2e-4, "bn fwd")
    y.backward(gy.to(DEV))
    close(xd.grad, xr.grad, 5e-4, "bn dx")
    close(bn.weight.grad, bn_ref.weight.grad, 5e-4, "bn dgamma")
    close(bn.bias.grad, bn_ref.bias.grad, 5e-4, "bn dbeta")
    close(bn.running_mean, bn_ref.running_mean, 1e-5, "running_mean")
    close(bn.running_var, bn_ref.running_var, 1e-5, "running_var")
    assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked)


def test_small_ops(hip_lib):
    from odvae_amd import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 8, 6, generator=g)
    xr = x.clone().requires_grad_(True)
    gy = torch.randn(2, 64, 8, 6, generator=g)
    F.leaky_relu(xr, 0.2).backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.leaky_relu(xd, 0.2)
    close(y, F.leaky_relu(x, 0.2), 1e-6, "lrelu")
    y.backward(gy.to(DEV))
    close(xd.grad, xr.grad, 1e-6, "lrelu bwd")
    # max pool with ties (post-ReLU zeros): gradient goes to the first maximum, like torch
    xp = torch.relu(torch.randn(2, 64, 8, 8, generator=g))
    xpr = xp.clone().requires_grad_(True)
    yp_ref = F.max_pool2d(xpr, 2, 2)
    gp = torch.randn(yp_ref.shape, generator=g)
    yp_ref.backward(gp)
    xpd = xp.to(DEV).requires_grad_(True)
    yp = ops.maxpool2x2(xpd)
    close(yp, yp_ref, 1e-6, "maxpool")
    yp.backward(gp.to(DEV))
    close(xpd.grad, xpr.grad, 1e-6, "maxpool bwd")
    # scaling layer
    shift = torch.tensor([-.030, -.088, -.188])[None, :, None, None]; scale = torch.tensor([.458, .448, .450])[None, :, None, None]
    xs = torch.randn(2, 3, 8, 8, generator=g)
    xsr = xs.clone().requires_grad_(True)
    ((xsr - shift) / scale).backward(torch.ones(2, 3, 8, 8))
    xsd = xs.to(DEV).requires_grad_(True)
    ys = ops.scale_shift(xsd, shift.to(DEV), scale.to(DEV))
    close(ys, (xs - shift) / scale, 1e-6, "scaling")
    ys.backward(torch.ones(2, 3, 8, 8, device=DEV))
    close(xsd.grad, xsr.grad, 1e-6, "scaling bwd")
    # conv3x3 + fused ReLU
    wt = torch.randn(64, 64, 3, 3, generator=g) / 24
    b = torch.randn(64, generator=g)
    xc = torch.randn(2, 64, 8, 8, generator=g)
    xcr = xc.clone().requires_grad_(True)
    yc_ref = F.relu(F.conv2d(xcr, wt, b, padding=1))
    gc = torch.randn(yc_ref.shape, generator=g)
    yc_ref.backward(gc)
    xcd = xc.to(DEV).requires_grad_(True)
    yc = ops.conv3x3(xcd, wt.to(DEV), b.to(DEV), None, 0, relu=True)
    close(yc, yc_ref, 2e-4, "conv+relu")
    yc.backward(gc.to(DEV))
    close(xcd.grad, xcr.grad, 5e-4, "conv+relu dx")


def _lpips_reference(f0, f1, w, gw, dt):
    f0, w, gw = f0.to(dt), w.to(dt), gw.to(dt)
    f1r = f1.to(dt).clone().requires_grad_(True)
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1r / (torch.sqrt(torch.sum(f1r ** 2, dim=1, keepdim=True)) + 1e-10)
    ref = F.conv2d((n0 - n1) ** 2, w).mean([1, 2, 3])
    (ref * gw).sum().backward()
    return ref.detach(), f1r.grad


# the last two: one pixel per image (the mean over pixels is the pixel itself), and a pixel count that is no multiple of any block size
@pytest.mark.parametrize("c,h,w", [(64, 6, 5), (128, 6, 5), (512, 6, 5), (256, 1, 1), (64, 1, 1031)], ids=["64", "128", "512", "256-hw1", "64-hw1031"])
def test_lpips_layer_distance(hip_lib, c, h, w):
    """Against torch f32 at the per-op tolerances, and against float64 under the acceptance rule of gn_offset_inputs with the
    distances in units of their float64 values (they are of size 1e-2) and the gradient in units of its largest float64 entry.
    relu(randn) over >= 64 channels leaves no pixel whose feature vector is all zero (torch's own gradient there is NaN)."""
    import gn_offset_inputs as G
    from odvae_amd import ops
    g = torch.Generator().manual_seed(c + 7 * (h * w - 30))
    f0 = torch.relu(torch.randn(2, c, h, w, generator=g))
    f1 = torch.relu(torch.randn(2, c, h, w, generator=g))
    assert (f0.sum(1) > 0).all() and (f1.sum(1) > 0).all()
    wt = torch.rand(1, c, 1, 1, generator=g) / c
    gw = torch.randn(2, generator=g)
    ref, grad = _lpips_reference(f0, f1, wt, gw, torch.float32)
    ref64, grad64 = _lpips_reference(f0, f1, wt, gw, torch.float64)
    f1d = f1.to(DEV).requires_grad_(True)
    out = ops.lpips_layer_distance(f0.to(DEV), f1d, wt.to(DEV))
    close(out, ref, 2e-5, "lpips dist")
    (out * gw.to(DEV)).sum().backward()
    close(f1d.grad, grad, 2e-4, "lpips dist bwd")
    gmax = grad64.abs().max()
    G.check([G.figure("distance / d64", out.cpu().double() / ref64, torch.ones_like(ref64), ref.double() / ref64, G.FLOOR_FWD),
             G.figure("gradient / max |g64|", f1d.grad.cpu().double() / gmax, grad64 / gmax, grad.double() / gmax, G.FLOOR_DX)],
            "lpips layer distance C=%d HW=%d" % (c, h * w))


def test_discriminator_matches_oracle(hip_lib):
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(5)
    ref = RefD().apply(weights_init)
    net = NLayerDiscriminator()
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    ref.train(); net.train()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    assert tuple(y_ref.shape) == (2, 1, 6, 6)
    gy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(7))
    y_ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    close(y, y_ref, 1e-3, "D fwd")
    y.backward(gy.to(DEV))
    close(xd.grad, xr.grad, 5e-3, "D dx")
    refp = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        close(p.grad, refp[name].grad, 5e-3, "D grad " + name)
    refb = dict(ref.named_buffers())
    for name, b in net.named_buffers():
        close(b.float(), refb[name].float(), 1e-4, "D buffer " + name)


def test_lpips_style_matches_oracle(hip_lib):
    from odvae_amd.gan import LPIPSStyle
    from oracle.losses import LPIPSStyle as RefL
    net = LPIPSStyle()
    ref = RefL()
    res = ref.load_state_dict(net.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).eval(); ref.eval()
    g = torch.Generator().manual_seed(8)
    x0 = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    x1 = (x0 + 0.3 * torch.randn(2, 3, 32, 32, generator=g)).clamp(-1, 1)
    x1r = x1.clone().requires_grad_(True)
    d_ref = ref(x0, x1r)
    assert tuple(d_ref.shape) == (2, 1, 1, 1)
    d_ref.sum().backward()
    x1d = x1.to(DEV).requires_grad_(True)
    d = net(x0.to(DEV), x1d)
    close(d, d_ref, 1e-3, "lpips fwd")
    d.sum().backward()
    close(x1d.grad, x1r.grad, 5e-3, "lpips dx")


def test_lpips_from_upstream_keyed_checkpoint(hip_lib, tmp_path):
    """A checkpoint carrying `loss.perceptual_loss.*` in the UPSTREAM key scheme goes through `ckpt_path` into the HIP model and
    straight into the oracle; both then give the same perceptual distance and input gradient (reference:
    src/modules/losses/contperceptual.py:3,5; src/models/autoencoder.py:97-98)."""
    import os
    import warnings
    from test_checkpoint import YAML, _oracle, synthetic_upstream_lpips_state
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    sd = synthetic_upstream_lpips_state(seed=21)
    torch.manual_seed(4)
    ref = _oracle()
    full = ref.state_dict()
    for k, v in sd.items():
        full["loss.perceptual_loss." + k] = v
    path = os.path.join(tmp_path, "last.ckpt")
    torch.save({"state_dict": full}, path)
    ref.load_state_dict(torch.load(path)["state_dict"], strict=True)
    mcfg, _ = synthetic.model_config(YAML, latent_hw=4, ch=32, perceptual_weight=1.0)
    mcfg.params["ckpt_path"] = path
    model = instantiate_from_config(mcfg).to(DEV)
    lp, lp_ref = model.loss.perceptual_loss.eval(), ref.loss.perceptual_loss.eval()
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # real (loaded) weights: the synthetic-weights warning must stay quiet
        model.loss._check_perceptual_weights()
    g = torch.Generator().manual_seed(9)
    x0 = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    x1 = (x0 + 0.25 * torch.randn(2, 3, 64, 64, generator=g)).clamp(-1, 1)
    x1r = x1.clone().requires_grad_(True)
    d_ref = lp_ref(x0, x1r)
    d_ref.sum().backward()
    x1d = x1.to(DEV).requires_grad_(True)
    d = lp(x0.to(DEV), x1d)
    close(d, d_ref, 1e-3, "lpips(ckpt) fwd")
    d.sum().backward()
    close(x1d.grad, x1r.grad, 5e-3, "lpips(ckpt) dx")
    # and a fresh loss with perceptual_weight > 0 on the stand-in weights does warn
    mcfg2, _ = synthetic.model_config(YAML, latent_hw=4, ch=32, perceptual_weight=1.0)
    model2 = instantiate_from_config(mcfg2).to(DEV)
    with pytest.warns(RuntimeWarning, match="SYNTHETIC"):
        model2.loss._check_perceptual_weights()


@pytest.mark.parametrize("ckpt", [False, "unit", "norm"], ids=["no-ckpt", "ckpt-unit", "ckpt-norm"])
@pytest.mark.parametrize("precision", [32, "bf16"], ids=["f32", "bf16"])
def test_one_pass_adaptive_weight_equals_the_three_pass_form(hip_lib, precision, ckpt):
    """The generator step's adaptive weight from ONE traversal of the LPIPS-style VGG stack and the discriminator (losses.PoseLoss,
    ODVAE_ADAPTIVE_WEIGHT_ONE_PASS, the default) against the reference's three backward passes ([UPSTREAM] calculate_adaptive_weight:
    two partial passes to decoder.conv_out.weight, then the full one; contperceptual.py:294-301) on the SAME model, batch and noise:
    d_weight, the total, and the gradient of every autoencoder parameter and of loss.logvar.  Backpropagation is linear in the incoming
    gradient, so the two differ by summation order at the reconstruction only: f32 1e-5 (every tensor holding >= 1e-4 of the gradient energy,
    relative to its largest entry; and the relative L2 difference of the whole gradient); under bf16 activations that f32 difference flips
    bf16 roundings downstream (5e-2 per tensor as in tests/test_bf16_model_gpu.py, 2e-2 on the whole gradient).  With every decoder checkpoint policy, because the 'norm'
    policy re-makes conv_out's input on each of the backward calls.  The discriminator and the frozen LPIPS-style net get NO gradient in
    the one-pass form (under [PL-1.9] toggle_optimizer they are requires_grad = False during optimizer 0 anyway); both forms are held
    to the reference's own outputs in tests/test_reference_glue_gpu.py."""
    import os
    from test_model_gpu import build_pair
    from odvae_amd import synthetic
    yaml_noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=31)
    batch = synthetic.make_batch(2, 64, seed=30)
    grads, scalars = {}, {}
    for one_pass in (True, False):
        model, _ = build_pair(perceptual_weight=1.0, disc_factor=1.0, activation_checkpoint=ckpt)
        model.set_precision(precision)
        model.train()
        model.loss.ONE_PASS = one_pass
        model._global_step = 2
        model.injected_noise = yaml_noise
        loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0)
        loss.backward()
        torch.cuda.synchronize()
        scalars[one_pass] = (float(loss), float(model.logged_metrics["train/d_weight"]), float(model.logged_metrics["train/g_loss"]))
        grads[one_pass] = {k: (p.grad.detach().float().cpu().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
        if one_pass:
            for k, g in grads[True].items():
                if k.startswith("loss.discriminator") or k.startswith("loss.perceptual_loss"):
                    assert g is None, k
            assert grads[True]["loss.logvar"] is not None
    tol, tol_l2 = (1e-5, 1e-5) if precision == 32 else (5e-2, 2e-2)     # measured: f32 2.0e-6 / 9.7e-7; bf16 1.7e-2 / 8.7e-3
    for a, b in zip(scalars[True], scalars[False]):
        assert abs(a - b) <= tol * max(1.0, abs(b)), (scalars[True], scalars[False])
    assert scalars[False][1] > 0.0                                  # the weight is live, not the eval-mode 0
    # per tensor: every tensor that holds >= 1e-4 of the gradient energy, relative to its own largest entry (a conv bias in front of a GroupNorm
    # has a near-zero gradient made of cancellation noise: such tensors are judged through the whole-gradient measures below only)
    keys = [k for k, g in grads[False].items() if g is not None and not (k.startswith("loss.discriminator") or k.startswith("loss.perceptual_loss"))]
    for k in keys:
        assert grads[True][k] is not None, k
    energy = {k: float(grads[False][k].double().pow(2).sum()) for k in keys}
    total = sum(energy.values())
    errs = sorted(((float((grads[True][k].double() - grads[False][k].double()).abs().max()) / max(float(grads[False][k].abs().max()), 1e-30), k)
                   for k in keys if energy[k] >= 1e-4 * total), reverse=True)
    a = torch.cat([grads[True][k].double().reshape(-1) for k in keys])
    b = torch.cat([grads[False][k].double().reshape(-1) for k in keys])
    rel_l2 = float((a - b).norm() / b.norm())
    print("one-pass vs three-pass adaptive weight (%s, ckpt=%s): %d tensors, %d above 1e-4 of the energy, worst of those %.2e (%s); whole gradient "
          "relative L2 difference %.2e" % (precision, ckpt, len(keys), len(errs), errs[0][0], errs[0][1], rel_l2))
    assert len(keys) > 200 and len(errs) >= 20
    assert errs[0][0] <= tol and rel_l2 <= tol_l2, (errs[:3], rel_l2)
