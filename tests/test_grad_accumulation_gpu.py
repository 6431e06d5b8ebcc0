"""Gradient accumulation on the device: the multi-tensor `arena += fresh gradient` kernel (odvae_grad_accumulate_f32) bit for bit against torch CPU
f32 adds, FusedAdam.gather_grads(accumulate=True) on hand-planted gradients, and Trainer(accumulate_grad_batches=N) on the real PoseAutoencoder
against the CPU oracle run micro-batch by micro-batch (it is NOT one batch of N * B: `_rescale`'s min / max, BatchNorm statistics and the
mask divisors are per micro-batch on both sides)."""
import ctypes
import os
import re

import pytest
import torch

from test_model_gpu import YAML, build_pair  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk():
    """Floats per chunk of the accumulate kernel, read from its source."""
    text = open(os.path.join(ROOT, "generative-detection_amd", "csrc", "elementwise.hip")).read()
    m = re.search(r"constexpr\s+int\s+kGradAccChunk\s*=\s*(\d+)\s*;", text)
    assert m, "kGradAccChunk not found in csrc/elementwise.hip"
    return int(m.group(1))


def _exact(n, gen):
    """n exact binary fractions +-(1 + k/8) * 2^e, e in [-20, 19], i.e. magnitudes in [2^-20, 2^20), with a few +0 / -0: sums and differences
    of two of them are multiples of 2^-23 -- never subnormal."""
    mant = 1.0 + torch.randint(0, 8, (n,), generator=gen).float() / 8
    v = mant * torch.exp2(torch.randint(-20, 20, (n,), generator=gen).float())
    v = v * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    z = torch.randint(0, 16, (n,), generator=gen)
    v = torch.where(z == 0, torch.zeros(n), v)
    return torch.where(z == 1, -torch.zeros(n), v)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _call(L, arena, offs, srcs, numels, count=None, arena_numel=None):
    from odvae_amd import lib
    n = len(offs)
    return L.odvae_grad_accumulate_f32(arena.data_ptr(), arena.numel() if arena_numel is None else arena_numel, (ctypes.c_int64 * n)(*offs),
                                       (ctypes.c_void_p * n)(*srcs), (ctypes.c_int64 * n)(*numels), n if count is None else count, lib.stream_ptr())


def test_accumulate_entry_point_bit_for_bit(hip_lib):
    L = hip_lib
    K, chunk = int(L.odvae_grad_accumulate_segments_per_launch()), _chunk()
    assert K >= 1 and chunk >= 64
    edge = [1, 3, 4, 5, 63, 64, 65, 1023, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    count = 2 * K + 1                                        # crosses two launch boundaries
    sizes = (edge * (count // len(edge) + 1))[:count]
    gen = torch.Generator().manual_seed(3)
    offs, off = [], 128
    for i, n in enumerate(sizes):
        offs.append(off)
        off += (n + 63) // 64 * 64 + 64 * (1 + i % 3)        # 64-float aligned slices with gaps of 64 ... 192 floats (+ the padding)
    offs[7] += 1                                             # one destination off the 16-byte grid (the scalar path on the arena side)
    total = off + 128
    sentinel = 12345.0
    arena_cpu = torch.full((total,), sentinel)
    srcs_cpu = []
    for i, (o, n) in enumerate(zip(offs, sizes)):
        arena_cpu[o:o + n] = _exact(n, gen)
        srcs_cpu.append(_exact(n, gen))
    srcs_cpu[11][2 * chunk + 1] = float("nan")               # in the tail of a two-chunk segment
    srcs_cpu[9][17] = float("inf")
    arena = arena_cpu.to("cuda:0")
    srcs_dev = [s.to("cuda:0") for s in srcs_cpu]
    # one source starts one float into a larger buffer: 4-byte aligned only
    big = torch.zeros(sizes[10] + 8, device="cuda:0")
    big[1:1 + sizes[10]] = srcs_dev[10]
    srcs_dev[10] = big[1:1 + sizes[10]]
    assert srcs_dev[10].data_ptr() % 16 == 4 and arena.data_ptr() % 256 == 0
    want = arena_cpu.clone()
    for o, n, s in zip(offs, sizes, srcs_cpu):
        want[o:o + n] = want[o:o + n] + s                    # torch CPU f32: one rounding per element
    rc = _call(L, arena, offs, [s.data_ptr() for s in srcs_dev], sizes)
    torch.cuda.synchronize()
    assert rc == 0, L.odvae_last_error()
    got = arena.cpu()
    nan_at = offs[11] + 2 * chunk + 1
    assert torch.isnan(got[nan_at]) and torch.isnan(want[nan_at])
    assert got[offs[9] + 17] == float("inf")
    got[nan_at] = want[nan_at] = 0.0                         # (NaN payloads are not under test)
    assert torch.equal(_bits(got), _bits(want))              # segments bit for bit (signs of zeros included), every guard float untouched
    inside = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        inside[o:o + n] = True
    assert (got[~inside] == sentinel).all() and int((~inside).sum()) > 64 * count


def test_accumulate_entry_point_rejects_bad_segments_before_any_launch(hip_lib):
    L = hip_lib
    arena = torch.full((1024,), 7.0, device="cuda:0")
    before = _bits(arena)
    a, b = torch.ones(64, device="cuda:0"), torch.ones(64, device="cuda:0")
    assert _call(L, arena, [0], [a.data_ptr()], [64], count=0) == 0                       # count = 0: success, nothing done
    bad = [([0, 1000], [a.data_ptr(), b.data_ptr()], [64, 64]),                            # past arena_numel
           ([0, 128], [a.data_ptr(), None], [64, 64]),                                     # null source
           ([0, 128], [a.data_ptr(), b.data_ptr()], [64, 0]),                              # empty segment
           ([0, -64], [a.data_ptr(), b.data_ptr()], [64, 64])]                             # negative offset
    for offs, srcs, numels in bad:
        assert _call(L, arena, offs, srcs, numels) != 0
        assert len(L.odvae_last_error()) > 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena), before)                 # the valid first segment was not launched either
    assert _call(L, arena, [0, 128], [a.data_ptr(), b.data_ptr()], [64, 64]) == 0
    torch.cuda.synchronize()
    assert (arena[:64] == 8.0).all() and (arena[64:128] == 7.0).all() and (arena[128:192] == 8.0).all() and (arena[192:] == 7.0).all()


def test_fused_adam_gather_accumulate_on_planted_gradients(hip_lib):
    from odvae_amd.optim import FusedAdam
    K = int(hip_lib.odvae_grad_accumulate_segments_per_launch())
    gen = torch.Generator().manual_seed(4)
    shapes = [(3,), (64,), (5, 7), (1000,), (4097,)]
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda:0")) for s in shapes]
    opt = FusedAdam(params, lr=1e-3)
    f = opt.materialize()
    opt.zero_grad()                                          # arena = 0, every .grad its arena view
    reached = [[0, 1, 2, 4], [0, 2, 3, 4], [0, 1, 2, 3, 4]]  # parameter 1 sits out round 2, parameter 3 is first reached in round 2
    sums = [torch.zeros(s) for s in shapes]
    first3 = None
    for rnd, idxs in enumerate(reached):
        opt.begin_microbatch()
        assert all(p.grad is None for p in params)
        for i in idxs:
            g = _exact(params[i].numel(), gen).view(shapes[i])
            if rnd == 1 and i == 3:
                first3 = g.clone()
            sums[i] = sums[i] + g                            # sequential f32 sums
            params[i].grad = g.to("cuda:0")
        calls = opt.accumulate_calls
        opt.gather_grads(accumulate=True)
        assert opt.accumulate_calls - calls == (len(idxs) + K - 1) // K
        for i, p in enumerate(params):
            if i in idxs:
                assert p.grad is not None and p.grad.data_ptr() == f["gviews"][i].data_ptr() and p.grad.shape == p.shape
            else:
                assert p.grad is None                        # left alone: the slice keeps its running sum
        torch.cuda.synchronize()
        arena = opt.flat_grad.cpu()
        for i, (p, o, n) in enumerate(opt.param_slices()):
            assert torch.equal(_bits(arena[o:o + n]), _bits(sums[i].reshape(-1))), (rnd, i)
        if rnd == 1:
            o, n = opt.param_slices()[3][1:]
            assert torch.equal(arena[o:o + n], first3.reshape(-1))
    calls = opt.accumulate_calls
    opt.gather_grads(accumulate=True)                        # nothing fresh: no launch
    assert opt.accumulate_calls == calls


def test_fused_adam_window_keeps_the_sums_through_clip_and_step(hip_lib):
    """The trap: clip_grad_norm_ / step gather with copy semantics.  Inside a window they must add what the last backward left fresh, keep the
    slice of a parameter only an earlier micro-batch reached, and step exactly the parameters the window reached."""
    from odvae_amd.optim import FusedAdam
    params = [torch.nn.Parameter(torch.full((n,), 0.5, device="cuda:0")) for n in (5, 64, 130, 7)]
    opt = FusedAdam(params, lr=1e-2, betas=(0.5, 0.9))
    opt.materialize()
    opt.zero_grad(set_to_none=True)
    (params[0].sum() * 2 + (params[1] * 3).sum()).backward()
    opt.gather_grads()                                       # window start: copy, unreached slices zeroed
    opt.begin_microbatch()
    ((params[1] * 0.25).sum() + (params[2] * 4).sum()).backward()
    norm = opt.clip_grad_norm_(1e9)
    want = [2.0, 3.25, 4.0, 0.0]
    for (p, o, n), w in zip(opt.param_slices(), want):
        assert (opt.flat_grad[o:o + n] == w).all(), (n, w)
        assert p.grad.data_ptr() == opt.flat_grad[o:o + 1].data_ptr()
    assert abs(norm.item() - (5 * 4.0 + 64 * 3.25 ** 2 + 130 * 16.0) ** 0.5) < 1e-3
    opt.step()
    assert opt._counts == [1, 1, 1, 0]
    assert (params[3] == 0.5).all() and all((p < 0.5).all() for p in params[:3])


# ---- the real model -------------------------------------------------------------------------------------------------------------------
def _clone(batch):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _grad_deviation(opt, model, ref):
    """check_step's metric (tests/test_model_gpu.py): per parameter max|g - g_ref| / max(max|g_ref|, 1e-3 * largest reference gradient)."""
    torch.cuda.synchronize()
    arena = opt.flat_grad.detach().cpu().double()
    name_of = {id(p): n for n, p in model.named_parameters()}
    ref_params = dict(ref.named_parameters())
    scale = max(p.grad.abs().max().item() for p in ref_params.values() if p.grad is not None)
    worst, compared = ("", 0.0), set()
    for p, o, n in opt.param_slices():
        name = name_of[id(p)]
        rg = ref_params[name].grad
        got = arena[o:o + n]
        if rg is None:
            assert got.abs().max().item() == 0.0, name
            continue
        compared.add(name.split(".")[0])
        e = (got - rg.double().reshape(-1)).abs().max().item() / max(rg.abs().max().item(), 1e-3 * scale)
        if e > worst[1]:
            worst = (name, e)
    assert {"encoder", "decoder", "quant_conv_obj", "post_quant_conv"} <= compared, compared
    return worst


MICRO = [(5, 6), (105, 106)]       # (batch seed, noise seed) of the two micro-batches; (5, 6) is check_step's own pair


def test_accumulated_gradient_matches_oracle(hip_lib):
    """ch = 32, 64 x 64, B = 2 per micro-batch, N = 3 with two micro-batches run: the window stays open, nothing is stepped, and the arena holds
    g_1 / 3 + g_2 / 3.  Bound: check_step's narrow-64 gradient tolerance 4.4e-4 -- accumulation adds one f32 rounding (2^-24 relative) per element
    and micro-batch, nothing on top is due.  Each micro-batch alone is held to the same bound through the N = 1 path first."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    tol = 4.4e-4
    model, ref = build_pair()
    model.train(); ref.train()
    model._global_step = ref.global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), accumulate_grad_batches=3)
    opt = trainer.optimizers[0]
    data = [(synthetic.make_batch(2, 64, seed=b), synthetic.make_noise(2, 4, dropout_p=0.7, seed=n)) for b, n in MICRO]
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for batch, noise in data:                                # each micro-batch alone, the parent's path: backward, one copy-gather
        model.injected_noise = noise
        loss = model.training_step(_clone(batch), 0, 0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.gather_grads()
        ref.zero_grad(set_to_none=True)
        ref.training_step(batch, 0, noise)[0].backward()
        worst = _grad_deviation(opt, model, ref)
        print("single micro-batch, N = 1 path: worst %s %.3e" % worst)
        assert worst[1] < tol, worst
    calls = opt.accumulate_calls
    ref.zero_grad(set_to_none=True)
    for i, (batch, noise) in enumerate(data):
        model.injected_noise = noise
        trainer.training_batch(_clone(batch), i)
        (ref.training_step(batch, 0, noise)[0] / 3).backward()
    assert trainer.accumulation_index == 2 and model.global_step == 1
    # the second micro-batch went through the accumulate kernel: every parameter it reached in one pass of ceil(reached / K) launches
    K = int(hip_lib.odvae_grad_accumulate_segments_per_launch())
    reached = sum(p.grad is not None for p, _, _ in opt.param_slices())
    assert reached > K and opt.accumulate_calls - calls == (reached + K - 1) // K, (reached, K, opt.accumulate_calls - calls)
    assert all(torch.equal(sd0[k], v) for k, v in model.state_dict().items())      # nothing stepped
    worst = _grad_deviation(opt, model, ref)
    print("accumulated over two micro-batches (N = 3): worst %s %.3e" % worst)
    assert worst[1] < tol, worst


def _oracle_window_loop(ref, ref_opts, data, n_acc, indices, clip=1.0):
    """oracle.autoencoder.train_batch stretched over windows of n_acc batches (PL-1.9): zero_grad at the window start, (loss / N).backward() per
    batch, clip + step + global_step on the window's last batch."""
    out, pos = [], 0
    for batch, noise in data:
        final = pos + 1 == n_acc
        row = []
        for idx in indices:
            opt = ref_opts[idx]
            others = [p for j, o in enumerate(ref_opts) if j != idx for g in o.param_groups for p in g["params"]]
            for p in others:
                p.requires_grad = False
            loss, log, aux = ref.training_step(batch, idx, noise)
            if pos == 0:
                opt.zero_grad()
            (loss / n_acc).backward()
            if final:
                if clip:
                    torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip)
                opt.step()
            for p in others:
                p.requires_grad = True
            if final:
                ref.global_step += 1
            row.append(loss.detach())
        out.append(row)
        pos = 0 if final else pos + 1
    return out


@pytest.mark.parametrize("gan", [False, True], ids=["rec+KL", "gan+lpips"])
def test_two_windows_of_two_match_oracle(hip_lib, gan):
    """N = 2, four batches = two optimizer steps per optimizer.  Bounds of the existing step tests (tests/test_model_gpu.py): per-micro-batch losses
    4e-6 (rec+KL) / 2e-3 (GAN), weights 2.2 lr per step + 5e-3 max|w|."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    indices = (0, 1) if gan else (0,)
    model, ref = build_pair(perceptual_weight=1.0, disc_factor=1.0) if gan else build_pair()
    model.train(); ref.train()
    if gan:
        ref.loss.perceptual_loss.eval()                      # as in test_gan_lpips_training_batch_matches_oracle
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=indices, accumulate_grad_batches=2)
    ref_opts = ref.configure_optimizers()
    data = [(synthetic.make_batch(2, 64, seed=500 + s), synthetic.make_noise(2, 4, dropout_p=0.7, seed=600 + s)) for s in range(4)]
    want = _oracle_window_loop(ref, ref_opts, data, 2, indices)
    owned = ("encoder", "decoder", "quant", "post_quant", "pose_", "loss.discriminator")
    got = []
    for i, (batch, noise) in enumerate(data):
        before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(owned) and v.dtype == torch.float32 and "running_" not in k}
        model.injected_noise = noise                         # (both optimizers' forwards see the same draws, on both sides)
        got.append(trainer.training_batch(_clone(batch), i))
        sd = model.state_dict()
        if i in (0, 2):                                      # first micro-batch of a window: no parameter moved
            assert all(torch.equal(before[k], sd[k]) for k in before), i
        else:
            assert any(not torch.equal(before[k], sd[k]) for k in before), i
    tol = 2e-3 if gan else 4e-6
    for i, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            print("batch %d: loss %.7f oracle %.7f" % (i, a.item(), b.item()))
            assert abs(a.item() - b.item()) <= tol * max(1.0, abs(b.item())), (i, a.item(), b.item())
    assert model.global_step == ref.global_step == 2 * len(indices)
    assert trainer.accumulation_index == 0
    ref_sd = ref.state_dict()
    lr, steps = model.learning_rate, 2
    keys = ("decoder", "loss.discriminator") if gan else ("encoder", "decoder", "quant", "post_quant", "pose_")
    checked = 0
    for k, v in model.state_dict().items():
        if v.dtype == torch.float32 and k.startswith(keys):
            diff = (v.detach().cpu().double() - ref_sd[k].double()).abs().max().item()
            assert diff <= 2.2 * lr * steps + 5e-3 * ref_sd[k].abs().max().item(), (k, diff)
            checked += 1
    assert checked > 20


def _shard(rank, step=0):
    """As in tests/test_00_parallel_gpu.py: every sample carries a pixel at 0 and one at 1, so `_rescale`'s batch min / max is the same on a
    micro-batch and on the concatenated batch."""
    from odvae_amd import synthetic
    batch = synthetic.make_batch(2, 64, seed=50 + 10 * step + rank)
    batch["patch"][:, :, 0, 0] = 0.0
    batch["patch"][:, :, 0, 1] = 1.0
    return batch, synthetic.make_noise(2, 4, seed=70 + 10 * step + rank)


def test_window_of_two_against_one_batch_of_four(hip_lib):
    """The parent's own path as the reference: two B = 2 micro-batches at N = 2 against their concatenation as one B = 4 batch at N = 1 (rec+KL,
    pinned pixels; lr = 0 and no clip in both, so the gradient arenas survive the step).  Mean of two half-batch means = full-batch mean up to the
    summation split: 2e-3 of each parameter's scale, the data-parallel bound of tests/test_00_parallel_gpu.py for the same comparison."""
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    arenas = []
    shards = [_shard(0), _shard(1)]
    for n_acc in (2, 1):
        torch.manual_seed(23)
        model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32)
        model.learning_rate = 0.0
        model = model.to("cuda:0").train()
        model._global_step = 1
        trainer = Trainer(model, gradient_clip_val=None, optimizer_indices=(0,), accumulate_grad_batches=n_acc)
        if n_acc == 2:
            for i, (batch, noise) in enumerate(shards):
                model.injected_noise = noise
                trainer.training_batch(_clone(batch), i)
        else:
            full = {k: (torch.cat([s[0][k] for s in shards], 0) if torch.is_tensor(shards[0][0][k]) else sum([s[0][k] for s in shards], []))
                    for k in shards[0][0]}
            model.injected_noise = {k: torch.cat([s[1][k] for s in shards], 0) for k in shards[0][1]}
            trainer.training_batch(full, 0)
        assert model.global_step == 2 and trainer.accumulation_index == 0
        torch.cuda.synchronize()
        arenas.append(trainer.optimizers[0].flat_grad.detach().cpu().double())
        slices = [(o, n) for _, o, n in trainer.optimizers[0].param_slices()]
    acc, full = arenas
    gmax = full.abs().max().item()
    assert gmax > 0
    worst = 0.0
    for o, n in slices:
        ref = full[o:o + n]
        err = (acc[o:o + n] - ref).abs().max().item()
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err / scale)
        assert err <= 2e-3 * scale, (o, n, err, scale)
    print("N = 2 x B = 2 against N = 1 x B = 4: worst per-parameter deviation %.2e of its scale" % worst)


def test_bf16_window_runs_and_steps_once(hip_lib):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32).to("cuda:0").train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), precision="bf16", accumulate_grad_batches=2)
    opt = trainer.optimizers[0]
    owned = [p for p, _, _ in opt.param_slices()]
    w0 = [p.detach().clone() for p in owned]
    losses = []
    for i in range(2):
        batch, noise = _shard(i)
        model.injected_noise = noise
        losses.append(trainer.training_batch(batch, i)[0])
        if i == 0:
            assert all(torch.equal(a, p.detach()) for a, p in zip(w0, owned)) and model.global_step == 1
            assert opt.flat_grad.dtype == torch.float32
    assert model.global_step == 2 and trainer.accumulation_index == 0 and opt.accumulate_calls >= 1
    assert any(not torch.equal(a, p.detach()) for a, p in zip(w0, owned))
    assert all(torch.isfinite(p).all() for p in owned) and all(torch.isfinite(l).all() for l in losses)
    assert max(opt._counts) == 1
