"""The opt-in implicit-GEMM form of the f32 PatchGAN convolutions (ops.DISC_F32_IMPLICIT, ops._Conv4x4I) through the op layer, the
discriminator, PoseLoss and the trainer, with the switch monkeypatched on.  The yardstick is always torch on the host / the oracle, at
the tolerances the same comparisons use with the switch off (tests/test_gan_lpips_gpu.py, tests/test_model_gpu.py,
tests/test_actnorm_model_gpu.py) -- never the switched-off path.  What the switch changes besides the kernels: a conv saves its input
and nothing else (no [N Ho Wo, 16 Cin] matrix), a discriminator weight is packed once per batch, and a GAN batch makes none of the
im2col / col2im / reorder calls.  On the parent commit everything here fails: ops has no DISC_F32_IMPLICIT."""
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLICIT = {"odvae_conv4x4_f32", "odvae_conv4x4_wgrad_f32"}
IM2COL = {"odvae_im2col4x4_f32", "odvae_col2im4x4_f32", "odvae_weight4x4_reorder_f32"}


@pytest.fixture
def implicit(hip_lib, monkeypatch):
    from odvae_amd import ops
    assert ops.DISC_F32_IMPLICIT is False, "the switch must be off by default"
    monkeypatch.setattr(ops, "DISC_F32_IMPLICIT", True)
    return ops


def close(a, b, tol, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    ref = max(1e-6, b.abs().max().item())
    print("%s: max err %.3e = %.2e of max|ref|" % (what, err, err / ref))
    assert err <= tol * ref, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, ref)


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


class _Recorder:
    """the loaded library with every odvae_* call noted by name"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("odvae_"):
            return f
        log = self._log

        def noted(*a):
            log.append(name)
            return f(*a)
        return noted


def recording(monkeypatch, fn):
    """the names of the C-ABI calls fn() makes"""
    from odvae_amd import lib
    log = []
    with monkeypatch.context() as mp:
        rec = _Recorder(lib.load(), log)
        mp.setattr(lib, "load", lambda: rec)
        fn()
    return log


# ------------------------------------------------------------------------------------------------------------------------------
# the op
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,h,w,stride,bias", [(2, 3, 64, 32, 32, 2, True), (2, 64, 128, 16, 16, 2, False),
                                                        (1, 32, 64, 9, 7, 1, False), (2, 64, 1, 8, 8, 1, True)])
def test_conv4x4_parity(implicit, monkeypatch, n, cin, cout, h, w, stride, bias):
    """tests/test_gan_lpips_gpu.py::test_conv4x4 with the switch on: random normal operands against CPU F.conv2d, 2e-4 / 5e-4 of max|ref|"""
    ops = implicit
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
    out = {}

    def run():
        out["y"] = ops.conv4x4(xd, wd, bd, stride)
        out["y"].backward(gy.to(DEV))
    calls = recording(monkeypatch, run)
    assert calls.count("odvae_conv4x4_f32") == 2 and calls.count("odvae_conv4x4_wgrad_f32") == 1 and not IM2COL & set(calls), calls
    assert not any(c.startswith("odvae_gemm") for c in calls)
    close(out["y"], y_ref, 2e-4, "conv4x4 fwd")
    close(xd.grad, xr.grad, 5e-4, "conv4x4 dx")
    close(wd.grad, wr.grad, 5e-4, "conv4x4 dw")
    if bias:
        close(bd.grad, br.grad, 5e-4, "conv4x4 db")


def test_weight_gradient_only_and_inputs_without_gradient_skip_the_data_gradient(implicit, monkeypatch):
    ops = implicit
    g = torch.Generator().manual_seed(3)
    x, wt = torch.randn(2, 8, 10, 12, generator=g), torch.randn(12, 8, 4, 4, generator=g)
    wd = wt.to(DEV).requires_grad_(True)
    calls = recording(monkeypatch, lambda: ops.conv4x4(x.to(DEV), wd, None, 2).sum().backward())
    assert calls.count("odvae_conv4x4_f32") == 1 and calls.count("odvae_conv4x4_wgrad_f32") == 1       # the input needs no gradient
    xd = x.to(DEV).requires_grad_(True)
    y = ops.conv4x4(xd, wd, None, 2)

    def probe():
        with ops.weight_gradient_only():
            torch.autograd.grad(y, wd, torch.ones_like(y))
    calls = recording(monkeypatch, probe)
    assert calls.count("odvae_conv4x4_f32") == 0 and calls.count("odvae_conv4x4_wgrad_f32") == 1


def test_backward_after_a_weight_update_is_refused(implicit):
    ops = implicit
    wd = torch.nn.Parameter(torch.randn(8, 8, 4, 4, device=DEV))
    xd = torch.randn(1, 8, 8, 8, device=DEV).requires_grad_(True)
    y = ops.conv4x4(xd, wd, None, 1)
    ops.PACK_CACHE.bump(stepped=[wd])         # an optimizer step on this weight between forward and backward
    with pytest.raises(RuntimeError, match="weight was updated"):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------------------------------------
# the discriminator
# ------------------------------------------------------------------------------------------------------------------------------
def discriminator_pair(seed=5):
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(seed)
    ref = RefD().apply(weights_init)
    net = NLayerDiscriminator()
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    ref.train(); net.train()
    return net, ref


@pytest.mark.parametrize("h,w", [(64, 64), (36, 44), (72, 72)], ids=lambda v: str(v))
def test_discriminator_matches_oracle(implicit, monkeypatch, h, w):
    """tests/test_gan_lpips_gpu.py::test_discriminator_matches_oracle with the switch on: 1e-3 forward, 5e-3 gradients, buffers 1e-4"""
    net, ref = discriminator_pair()
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(6))
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    gy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(7))
    y_ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    out = {}

    def run():
        out["y"] = net(xd)
        out["y"].backward(gy.to(DEV))
    calls = recording(monkeypatch, run)
    assert calls.count("odvae_conv4x4_f32") == 10 and calls.count("odvae_conv4x4_wgrad_f32") == 5 and not IM2COL & set(calls)
    close(out["y"], y_ref, 1e-3, "D fwd")
    close(xd.grad, xr.grad, 5e-3, "D dx")
    refp = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        close(p.grad, refp[name].grad, 5e-3, "D grad " + name)
    refb = dict(ref.named_buffers())
    for name, b in net.named_buffers():
        close(b.float(), refb[name].float(), 1e-4, "D buffer " + name)


def test_actnorm_discriminator_matches_the_restatement(implicit, hip_lib, monkeypatch):
    """`use_actnorm=True` (its convs carry biases), held to tests/actnorm_ref.py by the very comparison of
    tests/test_actnorm_model_gpu.py, run here with the switch on"""
    import test_actnorm_model_gpu as TA
    calls = recording(monkeypatch, lambda: TA.test_discriminator_matches_the_restatement(hip_lib, 64))
    assert calls.count("odvae_conv4x4_f32") == 2 * 10 and calls.count("odvae_conv4x4_wgrad_f32") == 2 * 5 and not IM2COL & set(calls)


def test_a_conv_saves_its_input_and_no_cols_matrix(implicit):
    from odvae_amd.gan import Conv4x4
    net, _ = discriminator_pair()
    n, h, w = 2, 64, 64
    xd = torch.randn(n, 3, h, w, device=DEV).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = net(xd)
    convs = [m for m in net.main if isinstance(m, Conv4x4)]
    assert len(convs) == 5
    cols_shapes, size = set(), (h, w)
    for m in convs:
        cin, stride = m.weight.shape[1], m.stride[0]
        size = tuple((s - 2) // stride + 1 for s in size)
        cols_shapes.add((n * size[0] * size[1], 16 * cin))
    assert not [tuple(t.shape) for t in saved if t.dim() == 2 and tuple(t.shape) in cols_shapes], "a cols matrix was saved"
    assert not [tuple(t.shape) for t in saved if t.dim() == 2 and t.shape[1] % 16 == 0 and t.shape[1] >= 48], "a GEMM operand was saved"
    # each conv node saves exactly its input: walk the graph, collect the nodes of the implicit Function
    nodes, stack, seen = [], [y.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "_Conv4x4I" in type(fn).__name__:
            nodes.append(fn)
        stack.extend(f for f, _ in fn.next_functions)
    assert len(nodes) == 5
    expect, size = [], (h, w)
    for m in convs:
        expect.append((n, m.weight.shape[1], size[0], size[1]))
        size = tuple((s - 2) // m.stride[0] + 1 for s in size)
    got = sorted(tuple(tuple(t.shape) for t in fn.saved_tensors) for fn in nodes)
    assert got == sorted((e,) for e in expect), got
    y.sum().backward()
    assert torch.isfinite(xd.grad).all()


# ------------------------------------------------------------------------------------------------------------------------------
# PoseLoss through the trainer
# ------------------------------------------------------------------------------------------------------------------------------
def test_both_gan_steps_match_oracle(implicit, monkeypatch):
    """tests/test_model_gpu.py::test_gan_lpips_training_batch_matches_oracle (narrow-64) with the switch on: generator step with the
    adaptive weight, then the discriminator step, two batches; its tolerances"""
    from test_model_gpu import build_pair
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    from oracle.autoencoder import train_batch
    height, latent_hw = 64, 4
    model, ref = build_pair(perceptual_weight=1.0, disc_factor=1.0, ch=32, latent_hw=latent_hw)
    model.train(); ref.train()
    ref.loss.perceptual_loss.eval()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
    ref_opts = ref.configure_optimizers()
    calls = []
    for step in range(2):
        batch = synthetic.make_batch(2, height, seed=300 + step)
        noises = {0: synthetic.make_noise(2, latent_hw, dropout_p=0.7, seed=400 + 2 * step),
                  1: synthetic.make_noise(2, latent_hw, dropout_p=0.7, seed=401 + 2 * step)}
        got = []
        for idx in (0, 1):   # one optimizer at a time so each forward sees its own injected noise
            model.injected_noise = noises[idx]
            trainer.optimizer_indices = (idx,)
            calls += recording(monkeypatch, lambda: got.append(
                trainer.training_batch({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, step)[0]))
            if idx == 0:
                logs = dict(model.logged_metrics)
        out = train_batch(ref, ref_opts, batch, noises, optimizer_indices=(0, 1), clip=1.0)
        for idx in (0, 1):
            a, b = got[idx].item(), out[idx][0].item()
            print("step %d optimizer %d: loss %.6f oracle %.6f" % (step, idx, a, b))
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (step, idx, a, b)
        for key in ("g_loss", "d_weight", "nll_loss", "rec_loss"):
            assert rel(logs["train/" + key], out[0][1]["train/" + key]) < 5e-3, (step, key, logs["train/" + key], out[0][1]["train/" + key])
    assert IMPLICIT <= set(calls) and not IM2COL & set(calls)
    assert model.global_step == 4 and ref.global_step == 4
    ref_sd = ref.state_dict()
    lr, steps = model.learning_rate, 2
    for k, v in model.state_dict().items():
        if v.dtype == torch.float32 and k.startswith(("decoder", "loss.discriminator")):
            diff = (v.detach().cpu().double() - ref_sd[k].double()).abs().max().item()
            assert diff <= 2.2 * lr * steps + 5e-3 * ref_sd[k].abs().max().item(), (k, diff)


def _trainer_and_batch(seed=23):
    from test_model_gpu import YAML
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(seed)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=1.0, disc_factor=1.0, disc_start=0).to(DEV).train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
    batch = synthetic.make_batch(2, 64, seed=seed)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step(i):
        b = dict(batch)
        b["pose_6d"] = batch["pose_6d"].clone()
        return trainer.training_batch(b, i)
    return model, trainer, step


def test_gan_batch_never_synchronises_the_host_and_packs_each_weight_once(implicit, monkeypatch):
    """After two warm-up batches a whole generator + discriminator batch issues without one host synchronisation, and each discriminator
    weight is packed once per batch although three discriminator forwards read it and the generator's optimizer steps in between"""
    from test_lpips_bf16_gpu import count_packs
    from odvae_amd.gan import Conv4x4
    ops = implicit
    model, trainer, step = _trainer_and_batch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(2):
            step(i)
        torch.cuda.synchronize()
        seen = count_packs(monkeypatch, ops)
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = step(2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(l).all() for l in losses)
    convs = [m for m in model.loss.discriminator.main if isinstance(m, Conv4x4)]
    assert len(convs) == 5
    for m in convs:
        assert seen.count(id(m.weight)) == 1, "discriminator weight %s packed %d times in one batch" % (tuple(m.weight.shape), seen.count(id(m.weight)))


def test_call_sequence_with_the_switch_on_and_off_again(hip_lib, monkeypatch):
    """The C-ABI calls of one GAN batch.  Switch on: none of the im2col / col2im / reorder calls; three forwards of five layers, data
    gradients five on the generator side (down to the image) and four each for real and fake (their inputs are detached), weight gradients
    for the discriminator step's two branches.  Switch off again: the sequence of a model that never had it on."""
    from odvae_amd import ops
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, step_plain = _trainer_and_batch()
        _, _, step = _trainer_and_batch()
        assert ops.DISC_F32_IMPLICIT is False
        for i in range(2):
            step_plain(i)
            with monkeypatch.context() as mp:
                mp.setattr(ops, "DISC_F32_IMPLICIT", True)
                step(i)
        plain = recording(monkeypatch, lambda: step_plain(2))
        with monkeypatch.context() as mp:
            mp.setattr(ops, "DISC_F32_IMPLICIT", True)
            on = recording(monkeypatch, lambda: step(2))
        off = recording(monkeypatch, lambda: step(3))
    assert not IMPLICIT & set(plain) and IM2COL <= set(plain)
    assert not IM2COL & set(on)
    assert on.count("odvae_conv4x4_f32") == 3 * 5 + 5 + 2 * 4 and on.count("odvae_conv4x4_wgrad_f32") == 2 * 5
    assert on.count("odvae_conv4x4_pack_f32") == 5
    assert off == plain, "switch off: %d calls against %d; first difference at %s" % (
        len(off), len(plain), next((i, a, b) for i, (a, b) in enumerate(zip(off + [None], plain + [None])) if a != b))
