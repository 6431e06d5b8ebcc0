"""Fused f32 attention (flash_attn_f32.hip, ops._FlashAttentionF32, switch ODVAE_ATTN_F32_FUSED): parity with the materialised
formula in float64 on the CPU, bit-reproducibility, peaked rows, the memory it saves, the dispatch, and the module / model level.

Tolerances: o within TOL_O * max(1, max|ref|); dq, dk, dv each within TOL_G of their own largest magnitude, floored at dv's: where the
exact dq and dk vanish (T = 1, saturated rows -- softmax is invariant to a shift of a row's scores) both paths leave f32 rounding noise of
dP - delta there.  Worst margins measured on the MI355X: o 6.7e-6 (peaked rows; 9.3e-7 on the parity shapes), gradients 2.7e-5 (dv,
peaked rows; 2.8e-6 on the parity shapes).
With Gaussian q and k one key is 1/T of an output, so these tolerances cannot see a dropped or duplicated key, a mask taken on the wrong
side of a clamped row, or lse2 / delta of the neighbouring query; tests/test_flash_attn_f32_exact_gpu.py pins the three kernels on
inputs with closed-form answers."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

YAML = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")
TOL_O = 1e-5
TOL_G = 5e-5


def ref_attention(qkv):
    n, c3, h, w = qkv.shape
    c = c3 // 3
    q, k, v = qkv.reshape(n, 3, c, h * w).unbind(1)            # [n, c, t]
    s = torch.bmm(q.transpose(1, 2), k) * (float(c) ** -0.5)     # [n, tq, tk]
    p = torch.softmax(s, dim=2)
    return torch.bmm(v, p.transpose(1, 2)).reshape(n, c, h, w)  # o[c, tq] = sum_k v[c, k] p[tq, k]


def fused(monkeypatch):
    from odvae_amd import ops
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", True)
    return ops


def run_device(ops, qkv, do):
    x = qkv.detach().to("cuda:0").clone().requires_grad_(True)
    o = ops.attention_qkv(x)
    o.backward(do.to("cuda:0"))
    torch.cuda.synchronize()
    return o.detach(), x.grad.detach(), o.grad_fn


def run_reference(qkv, do):
    x = qkv.double().requires_grad_(True)
    o = ref_attention(x)
    o.backward(do.double())
    return o.detach(), x.grad.detach()


def errors(o, dqkv, o_ref, dqkv_ref):
    """(o error against max(1, max|ref|), [dq, dk, dv] errors each against its own largest magnitude floored at dv's)"""
    o = o.cpu().double()
    eo = (o - o_ref).abs().max().item() / max(1.0, o_ref.abs().max().item())
    c = o_ref.shape[1]
    return eo, grad_errors(dqkv.cpu().double(), dqkv_ref, c)


def grad_errors(dqkv, dqkv_ref, c):
    parts = [(dqkv[:, i * c:(i + 1) * c], dqkv_ref[:, i * c:(i + 1) * c]) for i in range(3)]
    floor = parts[2][1].abs().max().item()
    return [(a - b).abs().max().item() / max(floor, b.abs().max().item()) for a, b in parts]


def inputs(n, c, h, w, seed, peaked=0.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * c, h, w, generator=g)
    if peaked:
        q, k = qkv[:, :c], qkv[:, c:2 * c]
        q.mul_(peaked)
        k.mul_(peaked)
        t = h * w
        perm = torch.randperm(t, generator=g)
        kf = k.reshape(n, c, t)
        kf[:, :, perm] += 0.5 * q.reshape(n, c, t)       # key perm[i] aligned with query i: one dominant key per row
    do = torch.randn(n, c, h, w, generator=g)
    return qkv, do


SHAPES = [(2, 64, 16, 16), (1, 128, 5, 9), (2, 256, 12, 11), (1, 256, 64, 64), (2, 512, 8, 8), (3, 64, 1, 1), (8, 128, 6, 7)]


@pytest.mark.parametrize("n,c,h,w", SHAPES)
def test_parity_with_float64_reference(hip_lib, monkeypatch, n, c, h, w):
    ops = fused(monkeypatch)
    qkv, do = inputs(n, c, h, w, seed=n * 1000 + c + h * w)
    o, dqkv, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_FlashAttentionF32Backward"
    eo, eg = errors(o, dqkv, *run_reference(qkv, do))
    assert eo < TOL_O, eo
    assert max(eg) < TOL_G, eg


def test_two_runs_are_bit_identical(hip_lib, monkeypatch):
    ops = fused(monkeypatch)
    qkv, do = inputs(2, 256, 12, 11, seed=7)
    o0, g0, _ = run_device(ops, qkv, do)
    o1, g1, _ = run_device(ops, qkv, do)
    assert torch.equal(o0, o1) and torch.equal(g0, g1)


@pytest.mark.parametrize("factor,c,hw", [(6.0, 64, 16), (10.0, 128, 9), (8.0, 256, 7)])
def test_peaked_rows(hip_lib, monkeypatch, factor, c, hw):
    ops = fused(monkeypatch)
    sentinel = object()
    monkeypatch.setattr(ops, "_ATTN_LAST_FLAG", sentinel)
    qkv, do = inputs(2, c, hw, hw, seed=11, peaked=factor)
    o, dqkv, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_FlashAttentionF32Backward"
    assert ops._ATTN_LAST_FLAG is sentinel          # the GEMM path's row-bound fallback never ran
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    o_ref, g_ref = run_reference(qkv, do)
    eo, eg = errors(o, dqkv, o_ref, g_ref)
    assert eo < TOL_O, eo
    assert max(eg) < TOL_G, eg


def _attention_peak(ops, qkv, do):
    x = qkv.to("cuda:0").requires_grad_(True)
    dod = do.to("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.attention_qkv(x).backward(dod)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_no_score_tensor_in_device_memory(hip_lib, monkeypatch):
    """N = 4, T = 4096, C = 64: one materialised P is 256 MiB; the fused forward + backward stays below 64 MiB above the baseline."""
    from odvae_amd import ops
    qkv, do = inputs(4, 64, 64, 64, seed=3)
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", False)
    off = _attention_peak(ops, qkv, do)
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", True)
    on = _attention_peak(ops, qkv, do)
    assert on < 64 * 2 ** 20, on
    assert off > 256 * 2 ** 20, off


def test_dispatch(hip_lib, monkeypatch):
    from odvae_amd import ops
    qkv, do = inputs(2, 64, 8, 8, seed=5)
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", False)
    _, _, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_AttentionBackward"
    monkeypatch.setattr(ops, "ATTN_SCORE_BUDGET", 64 * 64 * 4)
    _, _, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_AttentionRecomputeBackward"
    monkeypatch.undo()
    ops = fused(monkeypatch)
    _, _, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_FlashAttentionF32Backward"
    # a width the fused kernels do not take: today's path, still correct
    assert not hip_lib.odvae_flash_attn_f32_supported(2, 64, 48)
    qkv48, do48 = inputs(2, 48, 8, 8, seed=6)
    o, dqkv, fn = run_device(ops, qkv48, do48)
    assert type(fn).__name__ == "_AttentionBackward"
    eo, eg = errors(o, dqkv, *run_reference(qkv48, do48))
    assert eo < 2e-4 and max(eg) < 5e-4, (eo, eg)
    # bf16 keeps its own kernels
    x = qkv.to("cuda:0", torch.bfloat16).requires_grad_(True)
    assert type(ops.attention_qkv(x).grad_fn).__name__ == "_FlashAttentionBackward"


def rel_err(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


def test_attn_block_16384_tokens_matches_oracle(hip_lib, monkeypatch):
    """modules.AttnBlock against oracle/ldm_model.AttnBlock at T = 16 384, C = 64, B = 2 (test_modules_gpu.py runs the same case through
    the score budget): the fused path never holds one image's P (1 GiB)."""
    from odvae_amd import modules
    from oracle import ldm_model
    fused(monkeypatch)
    torch.manual_seed(5)
    c, hw = 64, 128
    ref = ldm_model.AttnBlock(c)
    net = modules.AttnBlock(c)
    assert not net.load_state_dict(ref.state_dict(), strict=True).missing_keys
    net = net.to("cuda:0")
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, c, hw, hw, generator=g)
    gy = torch.randn(2, c, hw, hw, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    y_ref.backward(gy)
    xd = x.to("cuda:0").requires_grad_(True)
    gyd = gy.to("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = net(xd)
    y.backward(gyd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 2 ** 30, "%.2f GiB" % (peak / 2 ** 30)
    assert rel_err(y, y_ref) < 1e-3
    assert rel_err(xd.grad, xr.grad) < 3e-3
    scale = max(pr.grad.abs().max().item() for pr in ref.parameters())
    for (name, p), (_, pr) in zip(net.named_parameters(), ref.named_parameters()):
        err = (p.grad.detach().cpu().double() - pr.grad.double()).abs().max().item() / max(1e-3 * scale, pr.grad.abs().max().item())
        assert err < 3e-3, (name, err)


def _model_step(ops, monkeypatch, on, ckpt):
    from odvae_amd import synthetic
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", on)
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32).to("cuda:0").train()
    if ckpt:
        model.decoder.activation_checkpoint = ckpt
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    model.zero_grad(set_to_none=True)
    model._global_step = 1
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("ckpt", [None, "unit", "norm"])
def test_training_step_fused_vs_gemm_path(hip_lib, monkeypatch, ckpt):
    from odvae_amd import ops
    calls = []
    orig = ops._FlashAttentionF32.forward
    monkeypatch.setattr(ops._FlashAttentionF32, "forward", staticmethod(lambda ctx, qkv: calls.append(1) or orig(ctx, qkv)))
    l0, g0 = _model_step(ops, monkeypatch, False, ckpt)
    assert not calls
    l1, g1 = _model_step(ops, monkeypatch, True, ckpt)
    assert calls
    assert abs(l1.item() - l0.item()) <= 1e-5 * abs(l0.item())
    assert g0.keys() == g1.keys()
    # a parameter whose exact gradient is ~0 (a conv bias in front of a GroupNorm) holds rounding noise on both sides: every parameter is
    # measured against at least 1e-3 of the largest gradient, as in test_modules_gpu.py
    floor = 1e-3 * max(g.abs().max().item() for g in g0.values())
    for k in g0:
        err = (g1[k] - g0[k]).abs().max().item() / max(floor, g0[k].abs().max().item())
        assert err < 1e-4, (k, err)


@pytest.mark.parametrize("n,hw", [(32, 64), (2, 128)])
def test_full_size_against_gemm_path(hip_lib, monkeypatch, n, hw):
    """The headline block (T = 4096, C = 256, N = 32) and T = 16 384, N = 2: fused against today's GEMM path, both on the device."""
    from odvae_amd import ops
    c = 256
    g = torch.Generator(device="cuda:0").manual_seed(13)
    qkv = torch.randn(n, 3 * c, hw, hw, generator=g, device="cuda:0")
    do = torch.randn(n, c, hw, hw, generator=g, device="cuda:0")
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", False)
    o_ref, g_ref, _ = run_device(ops, qkv, do)
    o_ref, g_ref = o_ref.double(), g_ref.double()
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", True)
    o, dqkv, fn = run_device(ops, qkv, do)
    assert type(fn).__name__ == "_FlashAttentionF32Backward"
    eo = (o.double() - o_ref).abs().max().item() / max(1.0, o_ref.abs().max().item())
    assert eo < TOL_O, eo
    eg = grad_errors(dqkv.double(), g_ref, c)
    assert max(eg) < TOL_G, eg
