"""model.params.ema_decay on the device: the three EMA kernels through the C ABI bit for bit against the CPU restatement of LitEma
(tests/ema_ref.py), then the model, the trainer, ema_scope, validation, log_images and the checkpoint round trip on the plain yaml at
height 32, batch 2, with injected noise.

"Bit for bit" means the same 32 bits wherever the restatement's result is a number (signed zeros, infinities and denormals included) and
a NaN wherever it is a NaN: which NaN an operation returns (sign, payload) is the processor's choice, and x86 and gfx950 choose
differently (Inf - Inf is 0xffc00000 on the one and 0x7fc00000 on the other).  The swap kernel moves bits and is compared on the raw
words, NaN payloads included."""
import ctypes
import os

import pytest
import torch

import ema_ref as E

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PLAIN_YAML = os.path.join(GOLDEN, "autoencoder_kl_plain.yaml")
DEV = "cuda:0"
SMALL = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
         "model.params.ddconfig.resolution=32", "model.params.ddconfig.z_channels=4", "model.params.embed_dim=4",
         "model.params.lossconfig.params.disc_start=0", "model.params.lossconfig.params.kl_weight=0.01"]

LENGTHS = [1, 3, 4, 63, 64, 65, 255, 256, 257, 1025]
GRID_CAP_THREADS = 8192 * 256                      # csrc/common.h grid_1d: at most 8 192 blocks of 256 threads
WRAPS = 4 * GRID_CAP_THREADS + 4 * 300 + 3         # float4 items past the cap: the stride loop runs a second time for 300 threads, + a tail of 3
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (3, 1)]      # floats from a 16-byte boundary: (parameter side, shadow side)
PAD = 8                                            # canary floats on either side of every array handed to a kernel
CANARY = 12345.6789

_INF, _NAN, _DEN, _MIN = float("inf"), float("nan"), 1e-40, 1.4e-45
SPECIAL_PAIRS = [(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (_INF, 1.0), (1.0, _INF), (-_INF, 2.0), (_INF, _INF), (_INF, -_INF),
                 (_NAN, 1.0), (1.0, _NAN), (_NAN, _NAN), (_DEN, 0.0), (0.0, _DEN), (_DEN, -_DEN), (_MIN, _MIN), (-_MIN, 2 * _MIN), (_MIN, 1.0),
                 (1.0, 1.0), (-3.5, -3.5), (1e-38, 1.1e-38), (3e38, -3e38), (_DEN, 3 * _DEN)]      # (shadow, parameter)


def pair_inputs(n, seed):
    """shadow, parameter [n]: N(0, 1) with every third element taken from SPECIAL_PAIRS (signed zeros, infinities, NaN, f32 denormals,
    s == p, differences that underflow or overflow), starting at a pair that depends on the seed"""
    g = torch.Generator().manual_seed(1000 + seed)
    s, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
    idx = torch.arange(0, n, 3)
    table = torch.tensor(SPECIAL_PAIRS, dtype=torch.float32)
    rows = table[(idx // 3 + seed) % len(SPECIAL_PAIRS)]
    s[idx], p[idx] = rows[:, 0], rows[:, 1]
    eq = torch.arange(1, n, 7)                      # and ordinary values with s == p
    p[eq] = s[eq]
    return s, p


def same_bits(got, want):
    """the same words wherever `want` is a number, a NaN wherever it is a NaN"""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]))


def raw_equal(a, b):
    return bool(torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)))


def placed(values, offset):
    """A device buffer with `values` at `offset` floats past a 16-byte boundary and canaries around them -> (buffer, first index)"""
    buf = torch.full((values.numel() + 2 * PAD + 4,), CANARY, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    start = PAD + offset
    buf[start:start + values.numel()] = values.to(DEV)
    return buf, start


def canaries_intact(buf, start, n):
    c = buf.new_tensor(CANARY)
    return bool((buf[:start] == c).all()) and bool((buf[start + n:] == c).all())


def ptr(buf, start):
    return buf.data_ptr() + 4 * start


def device_state(omd):
    return torch.stack([omd, 1 - omd]).to(DEV)


def last_error(L):
    return L.odvae_last_error().decode()


# ---- the update kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.9999])
def test_update_kernel_bit_for_bit(hip_lib, decay):
    from odvae_amd import lib
    L = hip_lib
    stream = lib.stream_ptr()
    _, _, omd = E.schedule(torch.tensor(decay, dtype=torch.float32), torch.tensor(-1, dtype=torch.int32))      # 1 - decay in f32
    _, _, omd_early = E.schedule(torch.tensor(decay, dtype=torch.float32), torch.tensor(0, dtype=torch.int32))  # 1 - 2 / 11
    assert omd.item() != omd_early.item()
    cases = [(n, 0, 0, omd) for n in LENGTHS] + [(n, a, b, omd) for n in (3, 65, 1025) for a, b in OFFSETS[1:]] + [(257, 0, 0, omd_early), (1025, 1, 1, omd_early)]
    specials_seen = 0
    for i, (n, off_p, off_s, w) in enumerate(cases):
        s, p = pair_inputs(n, i)
        want = E.update_(s.clone(), p, w)
        specials_seen += int((~torch.isfinite(want)).sum()) + int((want == 0).sum())
        pbuf, p0 = placed(p, off_p)
        sbuf, s0 = placed(s, off_s)
        state = device_state(w)
        lib.check(L.odvae_ema_update_f32(ptr(pbuf, p0), ptr(sbuf, s0), n, state.data_ptr(), stream), "ema_update")
        torch.cuda.synchronize()
        assert same_bits(sbuf[s0:s0 + n], want), "n=%d offsets (%d, %d) decay %g" % (n, off_p, off_s, decay)
        assert canaries_intact(sbuf, s0, n) and raw_equal(pbuf[p0:p0 + n], p) and canaries_intact(pbuf, p0, n), (n, off_p, off_s)
    assert specials_seen > 100


def test_update_kernel_where_the_stride_loop_wraps(hip_lib):
    from odvae_amd import lib
    n = WRAPS
    assert n // 4 > GRID_CAP_THREADS
    s, p = pair_inputs(n, 5)
    _, _, omd = E.schedule(torch.tensor(0.9999, dtype=torch.float32), torch.tensor(-1, dtype=torch.int32))
    want = E.update_(s.clone(), p, omd)
    for off in ((0, 0), (1, 1)):
        pbuf, p0 = placed(p, off[0])
        sbuf, s0 = placed(s, off[1])
        lib.check(hip_lib.odvae_ema_update_f32(ptr(pbuf, p0), ptr(sbuf, s0), n, device_state(omd).data_ptr(), lib.stream_ptr()), "ema_update")
        torch.cuda.synchronize()
        assert same_bits(sbuf[s0:s0 + n], want), off
        assert canaries_intact(sbuf, s0, n) and canaries_intact(pbuf, p0, n)


# ---- the tick: counter and schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.9, 0.9999, 0.5])
def test_tick_schedule_and_counter(hip_lib, decay):
    from odvae_amd import lib
    starts = list(range(0, 101)) + [10 ** 6, -1]
    dec = torch.tensor(decay, dtype=torch.float32)
    d_decay = dec.to(DEV)
    counters = torch.tensor(starts, dtype=torch.int32, device=DEV)
    states = torch.full((len(starts), 2), -7.0, dtype=torch.float32, device=DEV)
    for i in range(len(starts)):
        lib.check(hip_lib.odvae_ema_tick(d_decay.data_ptr(), counters.data_ptr() + 4 * i, states.data_ptr() + 8 * i, lib.stream_ptr()), "ema_tick")
    # a chain on one counter: 120 ticks, each state kept
    chain_counter = torch.zeros((), dtype=torch.int32, device=DEV)
    chain_states = torch.zeros(120, 2, dtype=torch.float32, device=DEV)
    for i in range(120):
        lib.check(hip_lib.odvae_ema_tick(d_decay.data_ptr(), chain_counter.data_ptr(), chain_states.data_ptr() + 8 * i, lib.stream_ptr()), "ema_tick")
    counters, states, chain_states, chain_counter = counters.cpu(), states.cpu(), chain_states.cpu(), chain_counter.cpu()      # the one read-back
    for i, start in enumerate(starts):
        n, d, omd = E.schedule(dec, torch.tensor(start, dtype=torch.int32))
        assert int(counters[i]) == int(n) == (start + 1 if start >= 0 else -1), start
        assert raw_equal(states[i], torch.stack([omd, d])), "start %d: got %s want %s" % (start, states[i].tolist(), [omd.item(), d.item()])
    n = torch.tensor(0, dtype=torch.int32)
    for i in range(120):
        n, d, omd = E.schedule(dec, n)
        assert raw_equal(chain_states[i], torch.stack([omd, d])), i
    assert int(chain_counter) == 120
    if decay == 0.9:       # the cap takes over at num_updates = 80
        assert chain_states[78, 1] < dec and raw_equal(chain_states[79, 1], dec) and raw_equal(chain_states[119, 1], dec)
    assert float(d_decay.cpu()) == float(dec)


# ---- the swap kernel -------------------------------------------------------------------------------------------------------------------------
def test_swap_kernel_exchanges_and_a_second_swap_restores(hip_lib):
    from odvae_amd import lib
    cases = [(n, 0, 0) for n in LENGTHS] + [(n, a, b) for n in (3, 65, 1025) for a, b in OFFSETS[1:]] + [(WRAPS, 0, 0), (WRAPS, 1, 1)]
    for i, (n, off_a, off_b) in enumerate(cases):
        a, b = pair_inputs(n, 40 + i)
        abuf, a0 = placed(a, off_a)
        bbuf, b0 = placed(b, off_b)
        lib.check(hip_lib.odvae_ema_swap_f32(ptr(abuf, a0), ptr(bbuf, b0), n, lib.stream_ptr()), "ema_swap")
        torch.cuda.synchronize()
        assert raw_equal(abuf[a0:a0 + n], b) and raw_equal(bbuf[b0:b0 + n], a), (n, off_a, off_b)
        lib.check(hip_lib.odvae_ema_swap_f32(ptr(abuf, a0), ptr(bbuf, b0), n, lib.stream_ptr()), "ema_swap")
        torch.cuda.synchronize()
        assert raw_equal(abuf[a0:a0 + n], a) and raw_equal(bbuf[b0:b0 + n], b), (n, off_a, off_b)
        assert canaries_intact(abuf, a0, n) and canaries_intact(bbuf, b0, n), (n, off_a, off_b)


# ---- argument errors: a code and a message, nothing launched ---------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch(hip_lib):
    from odvae_amd import lib
    L = hip_lib
    stream = lib.stream_ptr()
    p = torch.arange(64, dtype=torch.float32, device=DEV)
    s = torch.arange(64, dtype=torch.float32, device=DEV) * 2
    state = torch.tensor([0.5, 0.5], device=DEV)
    decay = torch.tensor(0.5, device=DEV)
    counter = torch.zeros((), dtype=torch.int32, device=DEV)
    keep = (p.clone(), s.clone(), state.clone(), counter.clone())
    bad = [
        (L.odvae_ema_update_f32, (None, s.data_ptr(), 64, state.data_ptr(), stream), "ema_update"),
        (L.odvae_ema_update_f32, (p.data_ptr(), None, 64, state.data_ptr(), stream), "ema_update"),
        (L.odvae_ema_update_f32, (p.data_ptr(), s.data_ptr(), 64, None, stream), "ema_update"),
        (L.odvae_ema_update_f32, (p.data_ptr(), s.data_ptr(), 0, state.data_ptr(), stream), "ema_update"),
        (L.odvae_ema_update_f32, (p.data_ptr(), s.data_ptr(), -4, state.data_ptr(), stream), "ema_update"),
        (L.odvae_ema_update_f32, (p.data_ptr() + 2, s.data_ptr(), 32, state.data_ptr(), stream), "4-byte aligned"),
        (L.odvae_ema_update_f32, (s.data_ptr() + 64, s.data_ptr(), 32, state.data_ptr(), stream), "overlap"),
        (L.odvae_ema_swap_f32, (None, s.data_ptr(), 64, stream), "ema_swap"),
        (L.odvae_ema_swap_f32, (p.data_ptr(), None, 64, stream), "ema_swap"),
        (L.odvae_ema_swap_f32, (p.data_ptr(), s.data_ptr(), 0, stream), "ema_swap"),
        (L.odvae_ema_swap_f32, (p.data_ptr(), s.data_ptr() + 1, 32, stream), "4-byte aligned"),
        (L.odvae_ema_swap_f32, (p.data_ptr(), p.data_ptr() + 4 * 31, 32, stream), "overlap"),
        (L.odvae_ema_swap_f32, (p.data_ptr(), p.data_ptr(), 32, stream), "overlap"),
        (L.odvae_ema_tick, (None, counter.data_ptr(), state.data_ptr(), stream), "ema_tick"),
        (L.odvae_ema_tick, (decay.data_ptr(), None, state.data_ptr(), stream), "ema_tick"),
        (L.odvae_ema_tick, (decay.data_ptr(), counter.data_ptr(), None, stream), "ema_tick"),
    ]
    for fn, args, word in bad:
        rc = fn(*args)
        assert rc != 0 and word in last_error(L), (args, rc, last_error(L))
        with pytest.raises(lib.HipLibraryError, match=word):
            lib.check(rc, "ema")
    torch.cuda.synchronize()
    assert all(raw_equal(a, b) for a, b in zip((p, s, state), keep[:3])) and int(counter) == 0
    # adjacent, not overlapping: fine
    lib.check(L.odvae_ema_swap_f32(p.data_ptr(), p.data_ptr() + 4 * 32, 32, stream), "ema_swap")
    torch.cuda.synchronize()
    assert torch.equal(p[:32].cpu(), torch.arange(32, 64, dtype=torch.float32))


def test_ops_surface_reports_its_bytes(hip_lib):
    from odvae_amd import lib, ops
    s, p = pair_inputs(1025, 3)
    ds, dp = s.to(DEV), p.to(DEV)
    decay, counter, state = torch.tensor(0.9, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    ev = ops.KERNEL_EVENTS
    was = (ev.on, ev.extra, ev.rec, ev.issued)
    ev.enable()
    ev.extra = True
    try:
        ops.ema_tick(decay, counter, state)
        ops.ema_update(dp, ds, state)
        ops.ema_swap(dp, ds, 100)
        got = {k: ev.summary(k) for k in ("ema_tick", "ema_update", "ema_swap")}
    finally:
        ev.on, ev.extra, ev.rec, ev.issued = was
    _, d, omd = E.schedule(torch.tensor(0.9), torch.tensor(0, dtype=torch.int32))
    want = E.update_(s.clone(), p, omd)
    assert raw_equal(state, torch.stack([omd, d])) and int(counter) == 1
    assert same_bits(torch.cat([dp[:100], ds[100:]]), want) and raw_equal(ds[:100], p[:100])
    assert got["ema_update"]["launches"] == 1 and got["ema_update"]["bytes_per_launch"] == 12.0 * 1025
    assert got["ema_swap"]["bytes_per_launch"] == 16.0 * 100 and got["ema_tick"]["launches"] == 1
    with pytest.raises(lib.HipLibraryError):
        ops.ema_update(p, s, state)
    with pytest.raises(ValueError):
        ops.ema_swap(dp, ds, 2000)
    with pytest.raises(lib.HipLibraryError):
        ops.ema_tick(decay, counter.float(), state)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------
def build(ema_decay=0.999, seed=23, extra=()):
    from odvae_amd.config import Config, instantiate_from_config
    dots = SMALL + list(extra) + ([] if ema_decay is None else ["model.params.ema_decay=%r" % ema_decay])
    config = Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(dots))
    torch.manual_seed(seed)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (the synthetic-LPIPS-weights warning)
        model = instantiate_from_config(config.model)
    model.learning_rate = 2 * config.model.base_learning_rate
    return model.to(DEV).train()


def make_batch(step):
    from odvae_amd import synthetic
    return synthetic.make_image_batch(2, 32, seed=300 + step)


def make_noise(step):
    g = torch.Generator().manual_seed(400 + step)
    return {"posterior_eps": torch.randn(2, 4, 16, 16, generator=g), "samples_eps": torch.randn(2, 4, 16, 16, generator=g)}


def trainable(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters() if n in model.model_ema.m_name2s_name}


def shadows(model):
    return {k: v.detach().cpu().clone() for k, v in model.model_ema.state_dict().items()}


def run_batches(model, trainer, steps, ref=None, first=0):
    for step in range(first, first + steps):
        model.injected_noise = make_noise(step)
        trainer.training_batch(make_batch(step), step)
        if ref is not None:
            ref(trainable(model))
            got = shadows(model)
            assert int(got["num_updates"]) == int(ref.num_updates) == step + 1
            bad = [k for k, v in ref.shadow.items() if not same_bits(got[k], v)]
            assert not bad, "after batch %d the shadows of %s differ from the restatement's" % (step, bad[:5])


def test_four_batches_follow_the_restatement_bit_for_bit(hip_lib):
    from odvae_amd import ops
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1))
    ema = model.model_ema
    assert len(ema.arenas) == 2 and [a[0].data_ptr() for a in ema.arenas] == [o._flat["p"].data_ptr() for o in trainer.optimizers]
    assert ema.encoderconv_inweight.data_ptr() == ema.arenas[0][1].data_ptr()       # the buffers are views of the shadow arena, same offsets
    start = trainable(model)
    ref = E.LitEmaRef(start, 0.999)
    assert all(raw_equal(v, ref.shadow[k]) for k, v in shadows(model).items() if k not in ("decay", "num_updates"))
    ev = ops.KERNEL_EVENTS
    was = (ev.on, ev.extra, ev.rec, ev.issued)
    ev.enable()
    ev.extra = True
    try:
        run_batches(model, trainer, 4, ref)
        launches = {k: len(v) for k, v in ev.rec.items() if k.startswith("ema_")}
    finally:
        ev.on, ev.extra, ev.rec, ev.issued = was
    assert launches == {"ema_tick": 4, "ema_update": 4 * 3}, launches      # per batch: one tick, one launch per arena, one for loss.logvar
    assert model.global_step == 8
    end, sh = trainable(model), shadows(model)
    moved = [n for n in end if not torch.equal(end[n], start[n])]
    assert len(moved) > 50 and any(n.startswith("loss.discriminator.") for n in moved) and "loss.logvar" not in moved
    assert all(not torch.equal(sh[E.shadow_name(n)], end[n]) for n in moved[:20])      # an average, not a copy
    assert raw_equal(sh["losslogvar"], end["loss.logvar"])


def test_one_update_per_batch_inside_an_accumulation_window(hip_lib):
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0, accumulate_grad_batches=2)
    ref = E.LitEmaRef(trainable(model), 0.999)
    run_batches(model, trainer, 4, ref)
    assert int(model.model_ema.num_updates) == 4
    assert [o._steps for o in trainer.optimizers] == [2, 2] and model.global_step == 4


def test_an_unstepped_discriminator_keeps_shadows_equal_to_its_parameters(hip_lib):
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
    start = trainable(model)
    ref = E.LitEmaRef(start, 0.999)
    run_batches(model, trainer, 3, ref)
    end, sh = trainable(model), shadows(model)
    disc = [n for n in end if n.startswith("loss.discriminator.")]
    assert len(disc) == 13 and all(raw_equal(end[n], start[n]) and raw_equal(sh[E.shadow_name(n)], end[n]) for n in disc)
    assert not torch.equal(sh["encoderconv_inweight"], end["encoder.conv_in.weight"])


def count_ema_launches(fn):
    from odvae_amd import ops
    ev = ops.KERNEL_EVENTS
    was = (ev.on, ev.extra, ev.rec, ev.issued)
    ev.enable()
    ev.extra = True
    try:
        fn()
        return {k: len(v) for k, v in ev.rec.items() if k.startswith("ema_")}
    finally:
        ev.on, ev.extra, ev.rec, ev.issued = was


def test_before_materialize_the_update_launches_per_parameter(hip_lib):
    """LitEma on its own, no Trainer: the same bits, one launch per shadowed parameter; and upstream's store / copy_to / restore"""
    from odvae_amd.ema import LitEma
    model = build(0.9)
    ema = model.model_ema
    assert ema.arenas == [] and isinstance(ema, LitEma)
    ref = E.LitEmaRef(trainable(model), 0.9)
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            if p.requires_grad:
                p.add_(0.01 * (i % 7 - 3))
    launches = count_ema_launches(lambda: ema(model))
    ref(trainable(model))
    got = shadows(model)
    assert launches == {"ema_tick": 1, "ema_update": len(ref.shadow)} and len(ref.shadow) == 168
    assert int(got["num_updates"]) == 1 and all(same_bits(got[k], v) for k, v in ref.shadow.items())
    # without the counter the decay is constant
    fixed = LitEma(model, decay=0.5, use_num_upates=False).to(DEV)
    ref_fixed = E.LitEmaRef(trainable(model), 0.5, use_num_upates=False)
    with torch.no_grad():
        model.encoder.conv_in.weight.mul_(3.0)
    fixed(model)
    ref_fixed(trainable(model))
    assert int(fixed.num_updates) == -1 and same_bits(fixed.encoderconv_inweight, ref_fixed.shadow["encoderconv_inweight"])
    # upstream's three methods
    before = trainable(model)
    params = [p for p in model.parameters() if p.requires_grad]
    ema.store(params)
    ema.copy_to(model)
    assert all(raw_equal(v, got[E.shadow_name(n)]) for n, v in trainable(model).items())
    ema.restore(params)
    assert all(raw_equal(v, before[n]) for n, v in trainable(model).items()) and ema.collected_params == []


def test_learn_logvar_moves_logvar_into_the_arena(hip_lib):
    from odvae_amd.trainer import Trainer
    model = build(0.999, extra=["model.params.learn_logvar=True"])
    trainer = Trainer(model, gradient_clip_val=1.0)
    assert model.loss.logvar.data_ptr() == trainer.optimizers[0]._flat["p"].data_ptr() + 4 * trainer.optimizers[0]._flat["offsets"][-1]
    ref = E.LitEmaRef(trainable(model), 0.999)
    launches = count_ema_launches(lambda: run_batches(model, trainer, 2, ref))
    assert launches == {"ema_tick": 2, "ema_update": 2 * 2}, launches      # no stray parameter is left
    assert float(model.loss.logvar.detach()) != 0.0 and not raw_equal(model.model_ema.losslogvar, model.loss.logvar)


@pytest.fixture(scope="module")
def trained(hip_lib):
    """a model three batches into training (shadows and parameters differ), its trainer"""
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0)
    run_batches(model, trainer, 3)
    return model, trainer


def forward_bits(model, x):
    model.injected_noise = make_noise(77)
    with torch.no_grad():
        xrec, post = model(x)
    return xrec.detach().clone(), post.parameters.detach().clone()


def test_ema_scope_swaps_in_the_average_and_restores_the_exact_bits(trained):
    from odvae_amd import ops
    model, _ = trained
    x = model.get_input(make_batch(50), "image")
    before, sh = trainable(model), shadows(model)
    out_before = forward_bits(model, x)
    # a twin without the average whose weights ARE the shadows
    twin = build(None, seed=5)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("model_ema.")}
    for n in before:
        sd[n] = sh[E.shadow_name(n)]
    assert not twin.load_state_dict(sd, strict=True).missing_keys
    out_twin = forward_bits(twin, x)
    assert not raw_equal(out_twin[0], out_before[0])
    epoch = ops.PACK_CACHE.epoch
    with model.ema_scope("test"):
        assert ops.PACK_CACHE.epoch == epoch + 1
        inside = trainable(model)
        assert all(raw_equal(inside[n], sh[E.shadow_name(n)]) for n in inside)
        held = shadows(model)
        assert all(raw_equal(held[E.shadow_name(n)], before[n]) for n in before)      # the trained weights wait in the shadows
        out_inside = forward_bits(model, x)
        assert raw_equal(out_inside[0], out_twin[0]) and raw_equal(out_inside[1], out_twin[1])      # the weight packs were refreshed
        with pytest.raises(RuntimeError, match="already inside"):
            with model.ema_scope():
                pass
    assert ops.PACK_CACHE.epoch == epoch + 2
    after = trainable(model)
    assert all(raw_equal(after[n], before[n]) for n in before)
    assert all(raw_equal(v, sh[k]) for k, v in shadows(model).items())
    out_after = forward_bits(model, x)
    assert raw_equal(out_after[0], out_before[0]) and raw_equal(out_after[1], out_before[1])
    # an exception inside the scope
    with pytest.raises(KeyError, match="boom"):
        with model.ema_scope():
            raise KeyError("boom")
    after = trainable(model)
    assert all(raw_equal(after[n], before[n]) for n in before) and all(raw_equal(v, sh[k]) for k, v in shadows(model).items())
    assert raw_equal(forward_bits(model, x)[0], out_before[0])


def test_a_graph_from_outside_the_scope_cannot_be_back_propagated_inside(trained):
    model, _ = trained
    x = model.get_input(make_batch(51), "image")
    model.injected_noise = make_noise(78)
    xrec, _ = model(x)
    loss = xrec.square().mean()
    with model.ema_scope():
        with pytest.raises(RuntimeError, match="weights were updated"):
            loss.backward()
    model.zero_grad(set_to_none=True)


def test_validation_logs_the_ema_pass(hip_lib):
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0)
    model.injected_noise = make_noise(60)
    first = trainer.validate([make_batch(60)])
    names = ("total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss", "disc_loss", "logits_real", "logits_fake")
    assert set(first) == {"val/" + k for k in names} | {"val_ema/" + k for k in names}
    for k in names:      # before any training step the shadows are the parameters
        assert raw_equal(first["val_ema/" + k], first["val/" + k]), k
    assert model.training and model.validation_step(make_batch(60), 0) == model.log_dict
    run_batches(model, trainer, 3)
    model.injected_noise = make_noise(60)
    later = trainer.validate([make_batch(60)])
    assert torch.isfinite(later["val_ema/rec_loss"]) and torch.isfinite(later["val/rec_loss"])
    assert later["val_ema/rec_loss"] != later["val/rec_loss"] and later["val_ema/kl_loss"] != later["val/kl_loss"]
    assert later["val/rec_loss"] != first["val/rec_loss"] and trainer.callback_metrics["val_ema/rec_loss"] == later["val_ema/rec_loss"]


def test_log_images_adds_the_ema_pictures(trained):
    model, _ = trained
    model.injected_noise = make_noise(61)
    before = trainable(model)
    log = model.log_images(make_batch(61))
    assert set(log) == {"inputs", "reconstructions", "samples", "reconstructions_ema", "samples_ema"}
    for k, v in log.items():
        assert v.shape == (2, 3, 32, 32) and v.is_cuda and not v.requires_grad and torch.isfinite(v).all(), k
    assert not torch.equal(log["reconstructions_ema"], log["reconstructions"]) and not torch.equal(log["samples_ema"], log["samples"])
    after = trainable(model)
    assert all(raw_equal(after[n], before[n]) for n in before)
    assert list(model.log_images(make_batch(61), only_inputs=True)) == ["inputs"]
    # without the average: log_ema asks for the keys, the pass runs on the weights themselves
    plain = build(None)
    plain.injected_noise = make_noise(61)
    assert set(plain.log_images(make_batch(61))) == {"inputs", "reconstructions", "samples"}
    both = plain.log_images(make_batch(61), log_ema=True)
    assert set(both) == set(log) and torch.equal(both["reconstructions_ema"], both["reconstructions"])


def test_checkpoint_round_trip(hip_lib, tmp_path):
    from odvae_amd.trainer import Trainer
    model = build(0.999)
    trainer = Trainer(model, gradient_clip_val=1.0)
    run_batches(model, trainer, 2)
    path = trainer.save_checkpoint(str(tmp_path / "ema.ckpt"))
    saved = torch.load(path, map_location="cpu")["state_dict"]
    assert {k for k in saved if k.startswith("model_ema.")} == {"model_ema." + k for k in shadows(model)} and int(saved["model_ema.num_updates"]) == 2

    other = build(0.5, seed=99)
    resumed = Trainer(other, gradient_clip_val=1.0)
    res = resumed.load_checkpoint(path)
    assert not res.missing_keys and not res.unexpected_keys and len(other.model_ema.arenas) == 2
    a, b = shadows(model), shadows(other)
    assert set(a) == set(b) and all(raw_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert int(b["num_updates"]) == 2 and float(b["decay"]) == float(torch.tensor(0.999, dtype=torch.float32))
    run_batches(model, trainer, 2, first=2)
    run_batches(other, resumed, 2, first=2)
    pa, pb, a, b = trainable(model), trainable(other), shadows(model), shadows(other)
    assert all(raw_equal(pa[n], pb[n]) for n in pa) and all(raw_equal(a[k], b[k]) for k in a) and int(b["num_updates"]) == 4

    # a checkpoint written without the average: strict=False leaves the shadows as constructed
    bare = build(None, seed=7)
    bare_trainer = Trainer(bare, gradient_clip_val=1.0)
    bare_path = bare_trainer.save_checkpoint(str(tmp_path / "bare.ckpt"))
    fresh = build(0.999, seed=11)
    built = shadows(fresh)
    fresh_trainer = Trainer(fresh, gradient_clip_val=1.0)
    with pytest.raises(RuntimeError, match="model_ema"):
        fresh_trainer.load_checkpoint(bare_path)
    res = fresh_trainer.load_checkpoint(bare_path, strict=False)
    assert set(res.missing_keys) == {"model_ema." + k for k in built} and not res.unexpected_keys
    assert all(raw_equal(v, built[k]) for k, v in shadows(fresh).items())
    assert raw_equal(fresh.encoder.conv_in.weight, bare.encoder.conv_in.weight) and not raw_equal(fresh.model_ema.encoderconv_inweight, bare.encoder.conv_in.weight)


def test_without_ema_decay_no_ema_kernel_runs(hip_lib):
    from odvae_amd import ops
    from odvae_amd.trainer import Trainer
    model = build(None)
    assert not model.use_ema and not hasattr(model, "model_ema")
    trainer = Trainer(model, gradient_clip_val=1.0)
    ev = ops.KERNEL_EVENTS
    was = (ev.on, ev.extra, ev.rec, ev.issued)
    ev.enable()
    ev.extra = True
    try:
        model.injected_noise = make_noise(0)
        trainer.training_batch(make_batch(0), 0)
        trainer.validate([make_batch(1)])
        names = sorted(ev.rec)
    finally:
        ev.on, ev.extra, ev.rec, ev.issued = was
    assert names and not [k for k in names if k.startswith("ema_")], names
    with model.ema_scope():      # nothing to swap: the scope is empty
        pass


def test_launcher_trains_validates_and_writes_the_average(hip_lib, capsys, tmp_path):
    from odvae_amd import run
    import warnings
    path = str(tmp_path / "run.ckpt")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = run.main(["-b", PLAIN_YAML, "--height", "32", "--steps", "4", "--checkpoint", path, "data.params.batch_size=2", "model.params.ema_decay=0.999"]
                         + SMALL[:4] + SMALL[6:7])
    out = capsys.readouterr().out
    assert model.use_ema and int(model.model_ema.num_updates) == 4 and model.global_step == 8
    line = [l for l in out.splitlines() if l.startswith("validation ")]
    assert len(line) == 1 and "val_ema/rec_loss" in line[0] and "ema updates 4" in line[0]
    saved = torch.load(path, map_location="cpu")["state_dict"]
    assert int(saved["model_ema.num_updates"]) == 4 and "model_ema.decoderconv_outweight" in saved
    assert not torch.equal(saved["model_ema.decoderconv_outweight"], saved["decoder.conv_out.weight"])
