"""track_grad_norm / gradient_clip_algorithm on the device: the segmented-norm entry point (odvae_grad_seg_norms_f32) against the float64
reference of tests/grad_norms_inputs.py -- bit for bit where every sum is exact, within the f32 rounding otherwise --, the clamped Adam step
(odvae_adam_step_clamp_f32) bit for bit against the plain step on torch.clamp'ed gradients, FusedAdam.grad_norms / clip_grad_value_, and
Trainer(track_grad_norm=, gradient_clip_algorithm=) on the narrow two-optimizer model; the runner in a child process."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_norms_inputs as gi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
DEV = "cuda:0"
GUARD = 777.0


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _flags(counts, n):
    return None if counts is None else (ctypes.c_ubyte * n)(*[1 if c else 0 for c in counts])


def _need(L, lengths):
    return int(L.odvae_grad_seg_norms_workspace_bytes(_i64(lengths), len(lengths)))


def _run(L, arena, offs, lengths, counts, p, n=None, ws=None, ws_bytes=None, out=None, n_seg=None):
    """One call on a workspace of exactly the queried size and a NaN-filled out with 8 guard floats behind it.  Returns (rc, out [n_seg + 9], ws)."""
    from odvae_amd import lib
    kind, pp = gi.kind_of(p) if not isinstance(p, tuple) else p
    count = len(offs) if n_seg is None else n_seg
    if out is None:
        out = torch.full((len(offs) + 9,), float("nan"), device=DEV)
        out[len(offs) + 1:] = GUARD
    if ws is None:
        ws = torch.zeros(max(_need(L, lengths), 16), dtype=torch.uint8, device=DEV)
    rc = L.odvae_grad_seg_norms_f32(arena.data_ptr() if arena is not None else None, arena.numel() if n is None else n, _i64(offs), _i64(lengths),
                                    _flags(counts, len(offs)), count, kind, pp, out.data_ptr(), ws.data_ptr(),
                                    ws.numel() if ws_bytes is None else ws_bytes, lib.stream_ptr())
    return rc, out, ws


def _norms(L, arena_np, offs, lengths, counts, p):
    """Two launches on the same buffers: the same bits, the guards untouched.  Returns the f32 [n_seg + 1] result on the host."""
    arena = torch.from_numpy(arena_np).to(DEV)
    assert arena.data_ptr() % 256 == 0
    rc, out, ws = _run(L, arena, offs, lengths, counts, p)
    torch.cuda.synchronize()
    assert rc == 0, L.odvae_last_error()
    first = out.cpu().numpy().copy()
    rc, out, ws = _run(L, arena, offs, lengths, counts, p, ws=ws, out=out)
    torch.cuda.synchronize()
    assert rc == 0, L.odvae_last_error()
    again = out.cpu().numpy()
    n = len(offs)
    assert gi.same_bits(first, again)
    assert (again[n + 1:] == GUARD).all()
    assert gi.same_bits(arena.cpu().numpy(), arena_np)                # (the arena is an input)
    return again[:n + 1]


def _check(got, want, p, exact_total=False):
    if p in (1, 2, "inf"):
        assert gi.same_bits(got[:-1], want[:-1]), np.nonzero(gi.ulps(got[:-1], want[:-1]))[0][:8]
        assert gi.ulps(got[-1:], want[-1:]).max() <= (1 if (p == 2 and not exact_total) else 0), (got[-1], want[-1])
    else:
        assert gi.ulps(got, want).max() <= 2, gi.ulps(got, want).max()


# ---- exact inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, "inf", 0.5, 3])
def test_edge_lengths_in_one_arena(hip_lib, p):
    L = hip_lib
    assert int(L.odvae_grad_seg_norms_segments_per_launch()) == gi.SEGS_PER_LAUNCH
    text = open(os.path.join(ROOT, "generative-detection_amd", "csrc", "elementwise.hip")).read()
    assert int(re.search(r"constexpr\s+int\s+kSegNormChunk\s*=\s*(\d+)\s*;", text).group(1)) == gi.CHUNK
    lengths = gi.EDGE_LENGTHS
    offs, total = gi.layout(lengths, lead=64)
    arena = gi.fill(lengths, offs, total, gi.whole_numbers(1))       # NaN in front, in every gap and behind the last segment
    counts = [i % 3 != 1 for i in range(len(lengths))]
    want = gi.reference(arena, offs, lengths, counts, p)
    assert np.isfinite(want).all()
    _check(_norms(L, arena, offs, lengths, counts, p), want, p)
    _check(_norms(L, arena, offs, lengths, None, p), gi.reference(arena, offs, lengths, None, p), p)
    none = _norms(L, arena, offs, lengths, [False] * len(lengths), p)
    assert none[-1] == 0.0 and gi.same_bits(none[:-1], _norms(L, arena, offs, lengths, None, p)[:-1])


@pytest.mark.parametrize("n_seg", [1, 129, 357])
def test_segment_counts_past_one_table(hip_lib, n_seg):
    rng = np.random.RandomState(n_seg)
    lengths = [int(v) for v in rng.choice(gi.EDGE_LENGTHS[:8] + [257, 1000], size=n_seg)]
    offs, total = gi.layout(lengths, gap=1)
    arena = gi.fill(lengths, offs, total, gi.whole_numbers(n_seg))
    counts = [bool(v) for v in rng.randint(0, 2, size=n_seg)] if n_seg > 1 else None
    for p in (1, 2, "inf", 3):
        _check(_norms(hip_lib, arena, offs, lengths, counts, p), gi.reference(arena, offs, lengths, counts, p), p)


def test_one_segment_of_two_to_the_24_plus_8_ones(hip_lib):
    big = (1 << 24) + 8
    offs, total = gi.layout([big], lead=64)
    arena = gi.fill([big], offs, total, lambda i, n: np.ones(n, dtype=np.float32))
    l1 = _norms(hip_lib, arena, offs, [big], None, 1)
    assert l1[0] == np.float32(16777224.0) and l1[1] == np.float32(16777224.0)      # a single f32 running sum stops at 16 777 216
    l2 = _norms(hip_lib, arena, offs, [big], None, 2)
    assert gi.same_bits(l2, np.array([np.sqrt(float(big))] * 2, dtype=np.float32))
    assert list(_norms(hip_lib, arena, offs, [big], None, "inf")) == [1.0, 1.0]


def test_l2_total_bit_for_bit_on_perfect_squares(hip_lib):
    lengths = [1, 3, 64, 65, 4097, 8193, 2]
    offs, total = gi.layout(lengths)
    arena = gi.fill(lengths, offs, total, lambda i, n: gi.perfect_square_segment(n, i + 1))
    want = gi.reference(arena, offs, lengths, None, 2)
    assert list(want[:-1]) == [1.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0]
    _check(_norms(hip_lib, arena, offs, lengths, None, 2), want, 2, exact_total=True)
    ones = [k * k for k in (1, 2, 3, 8, 64, 65)]                     # k^2 ones: norm k
    offs, total = gi.layout(ones)
    arena = gi.fill(ones, offs, total, lambda i, n: np.ones(n, dtype=np.float32))
    want = gi.reference(arena, offs, ones, None, 2)
    assert list(want[:-1]) == [1.0, 2.0, 3.0, 8.0, 64.0, 65.0]
    _check(_norms(hip_lib, arena, offs, ones, None, 2), want, 2, exact_total=True)


# ---- random gradients at the headline layout, scaled down ------------------------------------------------------------------------------------
def _headline_like_layout():
    """357 segments, about 1 M floats: the headline generator arena's mix (3x3 conv weights, biases, norm scales, one 3- and one 1-element
    parameter) at about 1/60 of its size."""
    rng = np.random.RandomState(357)
    lengths = [3, 1]
    while len(lengths) < 357:
        kind = len(lengths) % 6
        lengths.append(int({0: rng.choice([16, 32, 64]) ** 2 * 9, 1: rng.choice([16, 32, 64, 128]), 2: rng.choice([16, 32, 64, 128]),
                            3: rng.choice([32, 64]) ** 2, 4: rng.choice([16, 32, 64, 128]), 5: rng.choice([7, 100, 1000, 5000])}[kind]))
    return lengths


def test_random_gradients_against_float64_and_against_torch(hip_lib):
    lengths = _headline_like_layout()
    offs, total = gi.layout(lengths, gap=0)
    assert len(lengths) == 357 and 5e5 < sum(lengths) < 2e6
    rng = np.random.RandomState(7)
    arena = gi.fill(lengths, offs, total, lambda i, n: (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1)).astype(np.float32))
    t = torch.from_numpy(arena)
    for p in (2, 1, "inf"):
        want = gi.reference(arena, offs, lengths, None, p)
        got = _norms(hip_lib, arena, offs, lengths, None, p)
        u = gi.ulps(got, want)
        print("p = %s: worst segment %d ulp, total %d ulp" % (p, u[:-1].max(), u[-1]))
        assert u[:-1].max() <= 1 and u[-1] <= 2
        # torch's own f32 result is no closer to the unrounded float64 value than this kernel's, segment by segment
        norm = float("inf") if p == "inf" else float(p)
        exact = np.array([float(t[o:o + n].double().norm(norm)) for o, n in zip(offs, lengths)])
        torch32 = np.array([float(t[o:o + n].norm(norm)) for o, n in zip(offs, lengths)])
        mine_err, torch_err = np.abs(got[:-1].astype(np.float64) - exact), np.abs(torch32 - exact)
        print("       distance from float64: this kernel %.3e (sum), torch f32 %.3e (sum)" % (mine_err.sum(), torch_err.sum()))
        assert (mine_err <= torch_err).all(), np.nonzero(mine_err > torch_err)[0][:8]
        tot_exact = float(torch.from_numpy(got[:-1].copy()).double().norm(norm))
        tot_torch = float(torch.from_numpy(got[:-1].copy()).norm(norm))
        assert abs(float(got[-1]) - tot_exact) <= abs(tot_torch - tot_exact)


# ---- non-finite ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, "inf", 3])
def test_nonfinite_values(hip_lib, p):
    lengths = gi.EDGE_LENGTHS
    offs, total = gi.layout(lengths, lead=64)
    a = gi.fill(lengths, offs, total, gi.whole_numbers(2))
    a[offs[3] + 2] = np.nan
    a[offs[3] + 3] = 100.0                                           # after the NaN: a max that forgets NaN would answer 100
    a[offs[5] + 7] = np.inf
    a[offs[9] + 4096] = -np.inf                                      # the one element of a last partial chunk
    a[offs[7]:offs[7] + lengths[7]] = 0.0
    got = _norms(hip_lib, a, offs, lengths, None, p)
    assert np.isnan(got[3]) and np.isnan(got[-1]) and got[5] == np.inf and got[9] == np.inf and got[7] == 0.0
    assert np.isfinite(np.delete(got[:-1], [3, 5, 9])).all()         # nothing else caught it
    counts = [i not in (3, 5, 9) for i in range(len(lengths))]
    quiet = _norms(hip_lib, a, offs, lengths, counts, p)
    assert np.isnan(quiet[3]) and quiet[5] == np.inf and np.isfinite(quiet[-1])
    assert gi.ulps(quiet, gi.reference(a, offs, lengths, counts, p)).max() <= (2 if p == 3 else 1 if p == 2 else 0)
    counts[5] = True
    assert _norms(hip_lib, a, offs, lengths, counts, p)[-1] == np.inf


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(hip_lib):
    L = hip_lib
    lengths, offs = [64, 5, 100], [0, 64, 128]
    arena = torch.ones(256, device=DEV)
    out = torch.full((12,), GUARD, device=DEV)
    need = _need(L, lengths)
    assert need > 0
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    inf, nan = float("inf"), float("nan")
    bad = [dict(arena=None, n=256), dict(n_seg=0), dict(n_seg=-1),
           dict(lengths=[64, 0, 100]), dict(lengths=[64, -5, 100]),
           dict(offs=[0, 65, 128]), dict(offs=[0, 66, 128]), dict(offs=[0, -64, 128]),
           dict(lengths=[64, 5, 129]), dict(offs=[0, 64, 256]), dict(n=227),
           dict(p=(gi.P, 0.0)), dict(p=(gi.P, -1.0)), dict(p=(gi.P, inf)), dict(p=(gi.P, nan)), dict(p=(7, 2.0)),
           dict(ws_bytes=need - 1)]
    for kw in bad:
        args = dict(arena=arena, offs=offs, lengths=lengths, counts=None, p=2, ws=ws, out=out)
        args.update(kw)
        rc, _, _ = _run(L, **args)
        assert rc != 0, kw
        assert len(L.odvae_last_error()) > 0
    from odvae_amd import lib
    for null in ("out", "off", "len", "ws"):
        rc = L.odvae_grad_seg_norms_f32(arena.data_ptr(), 256, None if null == "off" else _i64(offs), None if null == "len" else _i64(lengths), None, 3,
                                        gi.L2, 0.0, None if null == "out" else out.data_ptr(), None if null == "ws" else ws.data_ptr(), need,
                                        lib.stream_ptr())
        assert rc != 0, null
    assert int(L.odvae_grad_seg_norms_workspace_bytes(_i64([64, 0]), 2)) == 0 and int(L.odvae_grad_seg_norms_workspace_bytes(_i64([64]), 0)) == 0
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (ws == 0x5A).all() and (arena == 1.0).all()
    rc, _, _ = _run(L, arena, offs, lengths, None, 2, ws=ws, out=out, ws_bytes=need)      # the same buffers, a good call
    torch.cuda.synchronize()
    assert rc == 0 and out[:4].tolist() == [8.0, np.float32(np.sqrt(5.0)), 10.0, np.float32(np.sqrt(np.float64(8.0) ** 2 + np.float64(np.float32(np.sqrt(5.0))) ** 2 + 100.0))]
    assert (out[4:] == GUARD).all() and (ws[need:] == 0x5A).all()


# ---- Adam with the element-wise clamp ------------------------------------------------------------------------------------------------------
def _adam(L, name, p, g, m, v, step, last):
    from odvae_amd import lib
    return getattr(L, name)(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1e-3, 0.5, 0.9, 1e-8, step, last, lib.stream_ptr())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 8192 * 256 * 4 + 4099])
def test_clamped_step_is_the_plain_step_on_clamped_gradients(hip_lib, n):
    L, c = hip_lib, 0.75
    g_np = gi.clamp_inputs(n, n % 5, c)
    if n > 16:
        assert np.isnan(g_np).any() and np.isinf(g_np).any() and np.signbit(g_np[g_np == 0]).any() and (np.abs(g_np[g_np != 0]) < 1e-38).any()
    gen = torch.Generator().manual_seed(n % 97)
    p0, m0, v0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01
    g = torch.from_numpy(g_np).to(DEV)
    g_ref = torch.clamp(g, -c, c)
    assert gi.same_bits(g_ref.cpu().numpy(), gi.clamp_model(g_np, c))      # torch.clamp on the device follows the same rules
    state = []
    for name, grad, last in (("odvae_adam_step_clamp_f32", g, ctypes.c_float(c)), ("odvae_adam_step_f32", g_ref, None)):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        for step in (1, 2):
            assert _adam(L, name, p, grad, m, v, step, last) == 0, L.odvae_last_error()
        torch.cuda.synchronize()
        state.append([t.cpu().numpy() for t in (p, m, v)])
    assert gi.same_bits(g.cpu().numpy(), g_np)                        # the gradients are not rewritten
    for a, b, what in zip(state[0], state[1], "pmv"):
        assert gi.same_bits(a, b), what
    assert np.isnan(state[0][0]).sum() == np.isnan(g_np).sum()         # NaN went through to the parameter, and only there


def test_clamped_step_refuses_a_bound_that_is_not_positive(hip_lib):
    L = hip_lib
    p, g, m, v = (torch.ones(64, device=DEV) for _ in range(4))
    for c in (0.0, -1.0, float("nan")):
        assert _adam(L, "odvae_adam_step_clamp_f32", p, g, m, v, 1, ctypes.c_float(c)) != 0
        assert len(L.odvae_last_error()) > 0
    torch.cuda.synchronize()
    assert all((t == 1.0).all() for t in (p, g, m, v))


# ---- FusedAdam -------------------------------------------------------------------------------------------------------------------------------
def test_fused_adam_grad_norms_and_clip_grad_value(hip_lib):
    from odvae_amd.optim import FusedAdam
    shapes = [(3,), (64,), (5, 7), (1000,), (4097,), (1,)]
    rng = np.random.RandomState(3)

    def make():
        params = [torch.nn.Parameter(torch.full(s, 0.5, device=DEV)) for s in shapes]
        opt = FusedAdam(params, lr=1e-2, betas=(0.5, 0.9))
        opt.materialize()
        opt.zero_grad(set_to_none=True)
        return params, opt
    params, opt = make()
    grads = [rng.randint(-8, 9, size=s).astype(np.float32) for s in shapes]
    for i, (q, g) in enumerate(zip(params, grads)):
        if i != 3:                                                   # parameter 3 gets no gradient: written as 0, outside the total
            q.grad = torch.from_numpy(g).to(DEV)
            opt._touched.add(i)
    f = opt.materialize()
    for p in (2, 1, "inf", 3):
        vec = opt.grad_norms(p)
        assert vec.shape == (len(shapes) + 1,) and vec.data_ptr() == opt.grad_norms(p).data_ptr()      # one buffer per optimizer
        flat = np.zeros(f["total"], dtype=np.float32)
        for i, (o, g) in enumerate(zip(f["offsets"], grads)):
            if i != 3:
                flat[o:o + g.size] = g.reshape(-1)
        want = gi.reference(flat, f["offsets"], [g.size for g in grads], [i != 3 for i in range(len(shapes))], p)
        assert want[3] == 0.0
        _check(vec.cpu().numpy(), want, p)
    with pytest.raises(ValueError):
        opt.grad_norms(0)
    with pytest.raises(ValueError):
        opt.grad_norms("max")
    # clip_grad_value_: armed for one step, applied in the kernel, .grad left alone; the twin clamps by hand
    c = 2.5
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt.clip_grad_value_(bad)
    opt.clip_grad_norm_(1.0)
    with pytest.raises(RuntimeError):
        opt.clip_grad_value_(c)
    opt.discard_window()
    assert not opt._clip_armed and opt._touched == set()
    opt._touched.update({0, 1, 2, 4, 5})
    opt.clip_grad_value_(c)
    with pytest.raises(RuntimeError):
        opt.clip_grad_norm_(1.0)
    opt.discard_window()
    assert opt._clamp is None
    opt._touched.update({0, 1, 2, 4, 5})
    opt.clip_grad_value_(c)
    before = [q.grad.clone() for i, q in enumerate(params)]
    opt.step()
    assert opt._clamp is None
    assert all(torch.equal(a, q.grad) for a, q in zip(before, params)) and max(float(b.abs().max()) for b in before) > c
    params2, opt2 = make()
    for i, (q, g) in enumerate(zip(params2, grads)):
        if i != 3:
            q.grad = torch.clamp(torch.from_numpy(g).to(DEV), -c, c)
            opt2._touched.add(i)
    opt2.step()
    torch.cuda.synchronize()
    for a, b in zip(params, params2):
        assert gi.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    assert torch.equal(params[3].detach(), torch.full(shapes[3], 0.5, device=DEV))
    opt.zero_grad(set_to_none=True)
    for q, g in zip(params, grads):
        q.grad = torch.from_numpy(g).to(DEV)
    opt._touched.update(range(len(shapes)))
    opt.step()                                                       # the next step is unclamped again
    opt2.zero_grad(set_to_none=True)
    for q, g in zip(params2, grads):
        q.grad = torch.from_numpy(g).to(DEV)
    opt2._touched.update(range(len(shapes)))
    opt2.step()
    torch.cuda.synchronize()
    for a, b in zip(params, params2):
        assert gi.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


# ---- Trainer on the narrow two-optimizer model ------------------------------------------------------------------------------------------------
def _model(seed=23):
    from odvae_amd import synthetic
    torch.manual_seed(seed)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=1.0, disc_factor=1.0)
    model = model.to(DEV).train()
    model._global_step = 1
    return model


def _feed(model, trainer, steps):
    from odvae_amd import synthetic
    for i in range(steps):
        torch.manual_seed(900 + i)
        model.injected_noise = synthetic.make_noise(2, 4, seed=70 + i)
        trainer.training_batch(synthetic.make_batch(2, 64, seed=50 + i), i)
    torch.cuda.synchronize()


def _state(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items() if v.dtype == torch.float32}


def test_tracking_changes_no_bit_and_logs_the_arena_norms(hip_lib):
    from odvae_amd.trainer import Trainer
    off = _model()
    _feed(off, Trainer(off, gradient_clip_val=1.0), 3)
    on = _model()
    trainer = Trainer(on, gradient_clip_val=1.0, track_grad_norm=2)
    names = {id(q): n for n, q in on.named_parameters()}
    seen = []

    def log_dict(d, *a, **k):
        if any(key.startswith("grad_") for key in d):                # called between the backward and the clip: .grad are the arena views
            want = {}
            for idx, opt in enumerate(trainer.optimizers):
                mine = {"grad_2.0_norm/%s" % names[id(q)]: q.grad.double().norm(2).float() for i, q in enumerate(opt.materialize()["params"])
                        if i in opt._touched and q.grad is not None}
                if mine and set(mine) & set(d):
                    want = mine
            seen.append(({k: v.clone() for k, v in d.items()}, {k: v.clone() for k, v in want.items()}))
    on.log_dict = log_dict
    _feed(on, trainer, 3)
    a, b = _state(off), _state(on)
    assert set(a) == set(b) and all(gi.same_bits(a[k], b[k]) for k in a)
    assert len(seen) == 6
    gen_keys = {k for k in seen[0][0]}
    disc_keys = {k for k in seen[1][0]}
    assert any("encoder.conv_in.weight" in k for k in gen_keys) and not any("discriminator" in k for k in gen_keys)
    assert all("discriminator" in k or k.endswith("_total") for k in disc_keys)
    for got, want in seen:
        assert set(got) == set(want) | {"grad_2.0_norm_total"}       # exactly the reached parameters of the stepped optimizer
        for k, v in want.items():
            assert got[k].dim() == 0 and got[k].device.type == "cuda"
            assert gi.ulps(got[k].cpu().numpy().reshape(1), v.cpu().numpy().reshape(1)).max() <= 1, k      # (p.grad.norm(2) taken in float64 and rounded once: the 1-ulp rule)
        vals = torch.stack([got[k] for k in want]).double()
        assert gi.ulps(got["grad_2.0_norm_total"].cpu().numpy().reshape(1), vals.norm(2).float().cpu().numpy().reshape(1)).max() <= 1
    logged0, vec0 = trainer.grad_norms[0]
    logged1, vec1 = trainer.grad_norms[1]
    assert ["grad_2.0_norm/%s" % n for n in logged0] == [k for k in seen[-2][0] if "/" in k] and vec0.numel() == len(logged0) + 1
    assert ["grad_2.0_norm/%s" % n for n in logged1] == [k for k in seen[-1][0] if "/" in k] and vec1.numel() == len(logged1) + 1
    assert torch.equal(vec0[-1], seen[-2][0]["grad_2.0_norm_total"]) and torch.equal(vec1[-1], seen[-1][0]["grad_2.0_norm_total"])


@pytest.mark.parametrize("precision", [None, "bf16"])
def test_value_clipping_is_the_clamp_applied_by_hand(hip_lib, precision):
    from odvae_amd.trainer import Trainer
    c = 1e-4
    auto = _model()
    _feed(auto, Trainer(auto, gradient_clip_val=c, gradient_clip_algorithm="value", precision=precision), 1)
    hand = _model()
    trainer = Trainer(hand, gradient_clip_val=None, precision=precision)
    bitten = []
    for opt in trainer.optimizers:
        def step(opt=opt, plain=opt.step):
            opt._ensure_grad_views()                                 # the gradients, captured in the arena ...
            g = opt.flat_grad
            bitten.append(float(g.abs().max()))
            g.clamp_(-c, c)                                          # ... clamped by torch, then the unclamped step (odvae_adam_step_f32)
            assert opt._clamp is None and not opt._clip_armed
            return plain()
        opt.step = step
    _feed(hand, trainer, 1)
    assert len(bitten) == 2 and min(bitten) > c
    a, b = _state(auto), _state(hand)
    assert set(a) == set(b) and all(gi.same_bits(a[k], b[k]) for k in a)
    unclipped = _model()
    _feed(unclipped, Trainer(unclipped, gradient_clip_val=None, precision=precision), 1)
    u = _state(unclipped)
    assert any(not gi.same_bits(a[k], u[k]) for k in a)


def test_runner_takes_both_keys_as_dotlist_overrides(hip_lib):
    """A fresh child process (its own HIP context) with a time limit: three batches with tracking on and value clipping."""
    cmd = [sys.executable, "-m", "odvae_amd.run", "-b", os.path.join("tests", "golden", "autoencoder_kl_16x16x16.yaml"), "--steps", "3",
           "--height", "64", "model.params.ddconfig.ch=32", "model.params.lossconfig.params.disc_start=0",
           "model.params.lossconfig.params.encoder_pretrain_steps=0", "data.params.batch_size=2",
           "lightning.trainer.track_grad_norm=2", "lightning.trainer.gradient_clip_algorithm=value"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"batch (\d+)\s+global_step (\d+)\s+aeloss (\S+)\s+discloss (\S+)", r.stdout)
    assert [int(l[0]) for l in lines] == [0, 1, 2] and int(lines[-1][1]) == 6, r.stdout[-2000:]
    for l in lines:
        assert torch.isfinite(torch.tensor([float(l[2]), float(l[3])])).all(), l
