"""Device-side latent noise on the GPU (model.params.device_noise): the seeded fill against the numpy mirror, the fused latent stage bit
for bit against the chain of kernels it replaces, and the two models with the option on and off.

The normals are compared with the float64 mirror under a bound measured on an MI355X (latent_noise_checks.NORMAL_ABS_BOUND,
profiles/device_noise.md); everything else here is a comparison of bits.  On the parent commit every test but the last fails: the entry
points, the `device_noise` key and the mirror module do not exist there."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PLAIN_YAML = os.path.join(GOLDEN, "autoencoder_kl_plain.yaml")
POSE_YAML = os.path.join(GOLDEN, "autoencoder_kl_16x16x16.yaml")
DEV = "cuda:0"
PAD = 8      # NaN canaries on both sides of every kernel output
SAMPLE, DROPOUT, NOISE = 1, 2, 4


@pytest.fixture(scope="module")
def env(hip_lib):
    from odvae_amd import latent_noise as ln
    from odvae_amd import lib
    import latent_noise_checks as chk
    return hip_lib, lib, ln, chk


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(n):
    """(buffer, view of its n inner floats): NaN everywhere, so an element the kernel skips and a write outside both show"""
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[PAD:PAD + n]


def canaries_intact(buf, n):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())


def fill(env, n, first, draw, kind=0, p=0.0):
    L, lib = env[0], env[1]
    buf, out = guarded(n)
    lib.check(L.odvae_noise_fill_f32(out.data_ptr(), n, first, draw.key, draw.step, draw.tag, kind, p, lib.stream_ptr()), "noise_fill")
    assert canaries_intact(buf, n), "noise_fill wrote outside its %d elements (first = %d)" % (n, first)
    return out


# ---- the fill against the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1, 2, 3, 2 ** 34 - 6])
def test_fill_matches_the_mirror(env, first):
    ln, chk = env[2], env[3]
    worst = 0.0
    for n in (1, 3, 4, 5, 1023):
        for step, tag in chk.WORDS:
            draw = chk.draw_of(step, tag)
            worst = max(worst, chk.assert_normals_match_mirror(fill(env, n, first, draw).cpu().numpy(), draw, first))
            for p in (0.0, 0.3, 0.7, 0.999, 1.0):
                chk.assert_dropout_matches_mirror(fill(env, n, first, draw, kind=1, p=p).cpu().numpy(), draw, first, p)
    print("first = %d: worst |device - float64 mirror| = %.3e" % (first, worst))


def test_fill_past_the_grid_cap(env):
    """One thread per quad under grid_1d's cap of 8192 blocks of 256: past 4 * 8192 * 256 elements the grid-stride loop takes a second trip"""
    chk = env[3]
    n, first = 4 * 8192 * 256 + 5, 1
    draw = chk.draw_of(7, 0x50000005)
    worst = chk.assert_normals_match_mirror(fill(env, n, first, draw).cpu().numpy(), draw, first)
    print("n = %d: worst |device - float64 mirror| = %.3e" % (n, worst))
    chk.assert_dropout_matches_mirror(fill(env, n, first, draw, kind=1, p=0.3).cpu().numpy(), draw, first, 0.3)


def test_fill_statistics_on_the_device(env):
    ln, chk = env[2], env[3]
    got = {}
    worst = 0.0
    for step, tag in chk.WORDS:
        draw = chk.draw_of(step, tag)
        got[(step, tag)] = x = fill(env, chk.N_STATS, 0, draw).cpu().numpy()
        chk.assert_normal_statistics(x, "device step %d tag %#x" % (step, tag))
        worst = max(worst, chk.assert_normals_match_mirror(x, draw, 0))
    print("2^20 normals x 3: worst |device - float64 mirror| = %.3e, largest |x| = %.4f" % (worst, max(np.abs(x).max() for x in got.values())))
    other_stream = fill(env, chk.N_STATS, 0, ln.with_stream(chk.draw_of(7, 0), "z_noise")).cpu().numpy()
    for what, a, b in (("two streams", got[(7, 0)], other_stream), ("two steps", got[(7, 0)], got[(0, 0)])):
        assert abs(chk.correlation_se(a, b)) <= chk.CAP_SE, what
    for p in (0.3, 0.7, 0.999):
        m = fill(env, chk.N_STATS, 0, ln.with_stream(chk.draw_of(7, 0), "dropout"), kind=1, p=p).cpu().numpy()
        assert abs(((m > 0).mean() - (1.0 - p)) / np.sqrt(p * (1.0 - p) / m.size)) <= chk.CAP_SE, p


def test_fill_refuses_bad_words(env):
    L, lib = env[0], env[1]
    out = torch.empty(4, device=DEV)
    for args in ((4, 0, 1, 1 << 32, 0, 0, 0.0), (4, 0, 1, 0, 1 << 32, 0, 0.0), (4, 0, 1, 0, 0, 2, 0.0), (4, 0, 1, 0, 0, 1, 1.5), (0, 0, 1, 0, 0, 0, 0.0)):
        assert L.odvae_noise_fill_f32(out.data_ptr(), *args, lib.stream_ptr()) == 1, args


# ---- the fused stage against the chain it replaces -----------------------------------------------------------------------------------------
def make_inputs(n, hw, cz, seed):
    g = torch.Generator().manual_seed(seed)
    mom = torch.randn(n * hw, 2 * cz, generator=g)
    for i, v in enumerate([-31.0, -30.0, 20.0, 21.0][:n * hw * cz]):      # logvar outside and on the clamp's two ends: the first entries
        mom[i // cz, cz + i % cz] = v
    add = torch.randn(n * hw * cz, generator=g)
    dz = torch.randn(n * hw * cz, generator=g)
    return mom.reshape(-1).to(DEV), add.to(DEV), dz.to(DEV)


def chain(env, mom, add, dz, n, hw, cz, draw, flags, p):
    """z and dmoments of today's kernels fed the fill's tensors: gaussian_sample -> latent_combine(mask) -> latent_combine(add = noise)
    -> latent_combine(add), and the backward autograd runs for it (latent_combine(dz, mask), gaussian_bwd)"""
    L, lib, ln = env[0], env[1], env[2]
    st = lib.stream_ptr()
    total = n * hw * cz
    new = lambda: torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
    eps = fill(env, total, 0, ln.with_stream(draw, 0)) if flags & SAMPLE else None
    m = fill(env, total, 0, ln.with_stream(draw, 1), kind=1, p=p) if flags & DROPOUT else None
    nz = fill(env, total, 0, ln.with_stream(draw, 2)) if flags & NOISE else None
    if flags & SAMPLE:
        z = new()
        lib.check(L.odvae_gaussian_sample_f32(mom.data_ptr(), eps.data_ptr(), z.data_ptr(), n, hw, cz, st), "gaussian_sample")
    else:
        z = mom.view(n * hw, 2 * cz)[:, :cz].contiguous().view(-1)      # mode(): the mean
    for mask, plus in ((m, None), (None, nz), (None, add)):
        if mask is not None or plus is not None:
            out = new()
            lib.check(L.odvae_latent_combine_f32(z.data_ptr(), lib.ptr(mask), lib.ptr(plus), out.data_ptr(), total, st), "latent_combine")
            z = out
    g = dz
    if m is not None:
        g = new()
        lib.check(L.odvae_latent_combine_f32(dz.data_ptr(), m.data_ptr(), None, g.data_ptr(), total, st), "latent_combine bwd")
    if flags & SAMPLE:
        dm = torch.full((2 * total,), float("nan"), dtype=torch.float32, device=DEV)
        lib.check(L.odvae_gaussian_bwd_f32(mom.data_ptr(), eps.data_ptr(), g.data_ptr(), None, dm.data_ptr(), n, hw, cz, st), "gaussian_bwd")
    else:
        dm = torch.cat([g.view(n * hw, cz), torch.zeros(n * hw, cz, device=DEV)], dim=1).view(-1)      # the gradient of a chunk
    return z, dm


def fused(env, mom, add, dz, n, hw, cz, draw, flags, p):
    L, lib = env[0], env[1]
    total = n * hw * cz
    zbuf, z = guarded(total)
    dbuf, dm = guarded(2 * total)
    lib.check(L.odvae_latent_stage_f32(mom.data_ptr(), lib.ptr(add), z.data_ptr(), n, hw, cz, draw.key, draw.step, draw.tag, flags, p,
                                       lib.stream_ptr()), "latent_stage")
    lib.check(L.odvae_latent_stage_bwd_f32(mom.data_ptr(), dz.data_ptr(), dm.data_ptr(), n, hw, cz, draw.key, draw.step, draw.tag, flags, p,
                                           lib.stream_ptr()), "latent_stage_bwd")
    assert canaries_intact(zbuf, total) and canaries_intact(dbuf, 2 * total), "latent_stage wrote outside its outputs"
    return z, dm


VARIATIONS = ([(SAMPLE | (DROPOUT if p > 0 else 0) | (NOISE if noise else 0), p, with_add)
               for p in (0.0, 0.3, 0.7, 1.0) for noise in (False, True) for with_add in (False, True)]
              + [(0, 0.0, False), (DROPOUT | NOISE, 0.3, True)])      # mode instead of sample


@pytest.mark.parametrize("n,hw,cz", [(1, 1, 3), (2, 5, 4), (3, 16, 16), (2, 256, 16), (33, 4096, 16)])
def test_fused_stage_is_the_chain_bit_for_bit(env, n, hw, cz):
    ln = env[2]
    mom, add, dz = make_inputs(n, hw, cz, seed=n * 1000 + hw + cz)
    draw = ln.make_draw(1234, 0, 7, True, 5)
    minus_zero = 0
    for flags, p, with_add in VARIATIONS:
        a = add if with_add else None
        z_ref, dm_ref = chain(env, mom, a, dz, n, hw, cz, draw, flags, p)
        z, dm = fused(env, mom, a, dz, n, hw, cz, draw, flags, p)
        what = "flags %d p %g add %s" % (flags, p, with_add)
        assert not torch.isnan(z).any() and not torch.isnan(dm).any(), what
        assert same_bits(z, z_ref), "z: %s, %d elements differ" % (what, int((bits(z) != bits(z_ref)).sum()))
        assert same_bits(dm, dm_ref), "dmoments: %s, %d elements differ" % (what, int((bits(dm) != bits(dm_ref)).sum()))
        minus_zero += int((bits(dm_ref) == -2 ** 31).sum())
        if flags & SAMPLE:      # the clamp: no logvar gradient at -31 and 21, one at -30 and 20 (where the dropout kept the element)
            dlv = dm.view(n * hw, 2 * cz)[:, cz:].reshape(-1)
            assert dlv[0].item() == 0.0 and (dlv.numel() < 4 or dlv[3].item() == 0.0)
            if p == 0.0 and dlv.numel() >= 4:
                assert dlv[1].item() != 0.0 and dlv[2].item() != 0.0
    print("(%d, %d, %d): %d variations, %d gradients of -0 in the chain's output" % (n, hw, cz, len(VARIATIONS), minus_zero))


def test_fused_stage_repeats_and_moves_with_the_call(env):
    ln = env[2]
    n, hw, cz = 3, 16, 16
    mom, add, dz = make_inputs(n, hw, cz, seed=3)
    flags, p = SAMPLE | DROPOUT | NOISE, 0.3
    draw = ln.make_draw(1234, 0, 7, True, 5)
    z0, dm0 = fused(env, mom, add, dz, n, hw, cz, draw, flags, p)
    z1, dm1 = fused(env, mom, add, dz, n, hw, cz, draw, flags, p)
    assert same_bits(z0, z1) and same_bits(dm0, dm1), "the same words must give the same bits, forward and backward"
    for other in (ln.make_draw(1234, 0, 7, True, 6), ln.make_draw(1234, 0, 8, True, 5), ln.make_draw(1234, 0, 7, False, 5), ln.make_draw(1234, 1, 7, True, 5)):
        z2, dm2 = fused(env, mom, add, dz, n, hw, cz, other, flags, p)
        assert (bits(z2) != bits(z0)).float().mean().item() > 0.9 and not same_bits(dm2, dm0), other
    L, lib = env[0], env[1]
    assert L.odvae_latent_stage_f32(mom.data_ptr(), None, z0.data_ptr(), n, hw, cz, 1, 0, 1 << 29, flags, p, lib.stream_ptr()) == 1, "stream bits in the tag"


def test_op_layer_backward_reads_no_saved_draw(env):
    """ops.latent_stage through autograd: the backward keeps the moments alone, gives `add` the incoming gradient itself, and equals the
    chain of ops (gaussian_sample, latent_combine) with the fill's tensors"""
    from odvae_amd import ops
    ln = env[2]
    draw = ln.make_draw(1234, 0, 3, True, 0)
    g = torch.Generator().manual_seed(11)
    mom = torch.randn(2, 8, 5, 3, generator=g).to(DEV).requires_grad_()
    add = torch.randn(2, 4, 5, 3, generator=g).to(DEV).requires_grad_()
    w = torch.randn(2, 4, 5, 3, generator=g).to(DEV)
    z = ops.latent_stage(mom, draw, add=add, dropout_p=0.3, noise=True)
    assert [tuple(t.shape) for t in z.grad_fn.saved_tensors] == [(2, 8, 5, 3)]
    (z * w).sum().backward()
    got = (z.detach().clone(), mom.grad.clone(), add.grad.clone())
    mom.grad = add.grad = None
    shape = (2, 4, 5, 3)
    eps, m, nz = (ops.noise_fill(shape, ln.with_stream(draw, s), DEV, kind=k, p=0.3, nhwc=True) for s, k in ((0, 0), (1, 1), (2, 0)))
    z_ref = ops.latent_combine(ops.latent_combine(ops.latent_combine(ops.gaussian_sample(mom, eps), m, None), None, nz), None, add)
    (z_ref * w).sum().backward()
    assert same_bits(got[0], z_ref) and same_bits(got[1], mom.grad) and same_bits(got[2], add.grad)


# ---- the models --------------------------------------------------------------------------------------------------------------------------
def pose_model(device_noise=None, state=None, disc_factor=1.0):
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    torch.manual_seed(23)
    mcfg, cfg = synthetic.model_config(POSE_YAML, latent_hw=4, ch=32, disc_factor=disc_factor)
    if device_noise is not None:
        mcfg.params["device_noise"] = device_noise
    model = instantiate_from_config(mcfg)
    if state is not None:
        model.load_state_dict(state, strict=True)
    model.learning_rate = 2 * cfg.model.base_learning_rate
    return model.to(DEV)


def plain_model(device_noise=None, state=None):
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    dots = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
            "model.params.ddconfig.resolution=32", "model.params.lossconfig.params.disc_start=0"]
    if device_noise is not None:
        dots.append("model.params.device_noise=%d" % device_noise)      # the launcher's dotlist override
    config = Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(dots))
    model = instantiate_from_config(config.model)
    if state is None:
        synthetic.fill_state_procedural(model, seed=23)
    else:
        model.load_state_dict(state, strict=True)
    model.learning_rate = 2 * config.model.base_learning_rate
    return model.to(DEV)


def clone_batch(batch):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}


def step_record(model, batch, optimizer_idx):
    """loss, logged scalars and parameter gradients of one training_step + backward"""
    model.zero_grad(set_to_none=True)
    model._logged = {}
    loss = model.training_step(clone_batch(batch), 0, optimizer_idx)
    loss.backward()
    logged = {k: (v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))) for k, v in model.logged_metrics.items()}
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), logged, grads


def assert_same_step(got, want, where):
    assert same_bits(got[0], want[0]), "%s: loss %r vs %r" % (where, got[0].item(), want[0].item())
    assert sorted(got[1]) == sorted(want[1]) and len(got[1]) > 3
    for k in want[1]:
        assert same_bits(got[1][k].float().cpu(), want[1][k].float().cpu()), "%s: logged %s %r vs %r" % (where, k, got[1][k], want[1][k])
    assert sorted(got[2]) == sorted(want[2]) and len(got[2]) > 10
    for k in want[2]:
        assert same_bits(got[2][k], want[2][k]), "%s: gradient of %s" % (where, k)


def test_pose_training_batch_equals_the_chain_with_the_fills_tensors(env):
    """Both optimizers of one batch.  On: device_noise=1234.  Off: the same weights, injected_noise = the fill's tensors for the words the
    first model uses (seed 1234, rank 0, the optimizer's global_step, training, call 0)."""
    from odvae_amd import ops, synthetic
    ln = env[2]
    on = pose_model(device_noise=1234)
    off = pose_model(state=on.state_dict())
    on.train(); off.train()
    batch = synthetic.make_batch(2, 64, seed=5)
    for idx in (0, 1):
        on._global_step = off._global_step = 1 + idx      # the trainer advances global_step after each optimizer's step
        draw = ln.make_draw(1234, 0, 1 + idx, True, 0)
        p = off._get_dropout_prob()
        assert 0.0 < p < 1.0
        shape = (2, 16, 4, 4)
        off.injected_noise = {"posterior_eps": ops.noise_fill(shape, ln.with_stream(draw, 0), DEV, nhwc=True),
                              "dropout_mask": ops.noise_fill(shape, ln.with_stream(draw, 1), DEV, kind=1, p=p, nhwc=True),
                              "z_noise": ops.noise_fill(shape, ln.with_stream(draw, 2), DEV, nhwc=True),
                              "bbox_eps": ops.noise_fill((2, 8), ln.with_stream(draw, 3), DEV)}
        want = step_record(off, batch, idx)
        got = step_record(on, batch, idx)
        assert on._last_draw == draw
        assert_same_step(got, want, "optimizer %d" % idx)
        if idx == 0:
            assert any(k.startswith("encoder.") for k in got[2]) and any(k.startswith("pose_") for k in got[2])
        else:
            assert any(k.startswith("loss.discriminator.") for k in got[2])


def test_plain_training_batch_equals_the_chain_with_the_fills_tensor(env):
    from odvae_amd import ops, synthetic
    ln = env[2]
    on = plain_model(device_noise=1234)
    assert on.device_noise == 1234
    off = plain_model(state=on.state_dict())
    on.train(); off.train()
    batch = synthetic.make_image_batch(2, 32, seed=5)
    for idx in (0, 1):
        on._global_step = off._global_step = 1 + idx
        draw = ln.make_draw(1234, 0, 1 + idx, True, 0)
        zc = on.embed_dim
        off.injected_noise = {"posterior_eps": ops.noise_fill((2, zc, 16, 16), draw, DEV, nhwc=True)}
        want = step_record(off, batch, idx)
        got = step_record(on, batch, idx)
        assert_same_step(got, want, "optimizer %d" % idx)


def watch_uploads(monkeypatch, lib):
    seen = []
    real = lib.upload
    monkeypatch.setattr(lib, "upload", lambda t, device: (seen.append(tuple(t.shape)) if not t.is_cuda else None, real(t, device))[1])
    return seen


def test_forward_touches_no_host_rng_and_uploads_no_noise(env, monkeypatch):
    from odvae_amd import synthetic
    lib = env[1]
    model = pose_model(device_noise=1234, disc_factor=0.0)
    model._global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    for training in (True, False):
        model.train(training)
        rgb = model._rgb_input(clone_batch(batch))
        seen = watch_uploads(monkeypatch, lib)
        before = torch.get_rng_state()
        with torch.enable_grad() if training else torch.no_grad():
            dec_obj, dec_pose, _, _ = model.forward(rgb)
        torch.cuda.synchronize()
        assert torch.equal(torch.get_rng_state(), before), "the forward drew from the host generator"
        assert seen == [], "uploads during the forward: %s" % seen
        assert torch.isfinite(dec_obj).all() and torch.isfinite(dec_pose).all()
    plain = plain_model(device_noise=1234)
    x = plain.get_input(synthetic.make_image_batch(2, 32, seed=5), "image")
    seen = watch_uploads(monkeypatch, lib)
    before = torch.get_rng_state()
    xrec, _ = plain(x)
    assert torch.equal(torch.get_rng_state(), before) and seen == [] and torch.isfinite(xrec).all()


def test_validation_and_log_images_run(env, monkeypatch):
    from odvae_amd import synthetic
    lib = env[1]
    model = pose_model(device_noise=1234, disc_factor=0.0)
    plain = plain_model(device_noise=1234)
    model._global_step = 1
    model.eval()
    batch = synthetic.make_batch(2, 64, seed=5)
    before = torch.get_rng_state()
    with torch.no_grad():
        model.validation_step(clone_batch(batch), 0)
    assert torch.isfinite(model.logged_metrics["val/rec_loss"]).all()
    calls = model._noise_calls.call
    log = model.log_images(clone_batch(batch))
    assert model._noise_calls.call == calls + 2, "log_images: the forward and the perturbed-pose sample are a call each"
    assert not same_bits(log["reconstructions_rgb"], log["perturbed_pose_reconstruction_rgb"])
    assert all(torch.isfinite(v).all() for v in log.values())
    plain.eval()
    ib = synthetic.make_image_batch(2, 32, seed=5)
    with torch.no_grad():
        plain.validation_step(ib, 0)
    log = plain.log_images(ib)
    assert {"samples", "reconstructions", "inputs"} <= set(log) and all(torch.isfinite(v).all() for v in log.values())
    assert torch.equal(torch.get_rng_state(), before), "validation / log_images drew from the host generator"
    # injected noise still wins: the injected samples_eps decodes to something else than the drawn one
    plain.injected_noise = {"samples_eps": torch.zeros(2, plain.embed_dim, 16, 16)}
    assert not same_bits(plain.log_images(ib)["samples"], log["samples"])


def test_resumed_run_draws_what_the_uninterrupted_run_drew(env, tmp_path):
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer

    def watched(model):
        drawn = []
        real = model._next_draw
        model._next_draw = lambda: (drawn.append(real()), drawn[-1])[1]
        return drawn

    model = pose_model(device_noise=1234, disc_factor=0.0)
    model.train()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
    batches = [synthetic.make_batch(2, 64, seed=300 + i) for i in range(3)]
    for i in range(2):
        trainer.training_batch(clone_batch(batches[i]), i)
    path = trainer.save_checkpoint(os.path.join(tmp_path, "last.ckpt"))
    drawn = watched(model)
    loss = trainer.training_batch(clone_batch(batches[2]), 2)[0]
    fresh = pose_model(device_noise=1234, disc_factor=0.0)
    fresh.train()
    trainer2 = Trainer(fresh, gradient_clip_val=1.0, optimizer_indices=(0,))
    trainer2.load_checkpoint(path)
    assert fresh.global_step == 2 and not any("noise" in k for k in fresh.state_dict())
    drawn2 = watched(fresh)
    loss2 = trainer2.training_batch(clone_batch(batches[2]), 2)[0]
    assert drawn2 == drawn == [env[2].make_draw(1234, 0, 2, True, 0)]
    assert same_bits(loss2, loss), "the resumed step: %r vs %r" % (loss2.item(), loss.item())


def test_option_off_consumes_the_host_generator_as_before(hip_lib):
    """device_noise absent: a fresh model's step under torch.manual_seed(s) equals, bit for bit, the step with injected_noise = the four
    host draws made in the order the forward has always made them (randn, rand, randn, randn) from the same seed.  Passes with and
    without the option in the code."""
    from odvae_amd import synthetic
    model = pose_model(disc_factor=0.0)
    model.train()
    model._global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    p = model._get_dropout_prob()
    shape = (2, 16, 4, 4)
    torch.manual_seed(77)
    model.injected_noise = {"posterior_eps": torch.randn(shape), "dropout_mask": (torch.rand(shape) >= p).float() / (1.0 - p),
                            "z_noise": torch.randn(shape), "bbox_eps": torch.randn(2, 8)}
    after = torch.get_rng_state()
    want = step_record(model, batch, 0)
    model.injected_noise = None
    torch.manual_seed(77)
    got = step_record(model, batch, 0)
    assert torch.equal(torch.get_rng_state(), after), "the forward drew more or less than four tensors"
    assert_same_step(got, want, "host draws")


def test_launcher_takes_the_key_as_a_dotlist_override(env, capsys):
    """python -m odvae_amd.run ... model.params.device_noise=1234: two batches of the plain yaml train with finite losses, and the host
    generator is where the model's construction left it"""
    from odvae_amd import run
    model = run.main(["-b", PLAIN_YAML, "--height", "32", "--steps", "2", "data.params.batch_size=2", "model.params.device_noise=1234",
                      "model.params.lossconfig.params.disc_start=0", "model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]",
                      "model.params.ddconfig.num_res_blocks=1", "model.params.ddconfig.resolution=32"])
    assert model.device_noise == 1234 and model.global_step == 4
    assert model._last_draw == env[2].make_draw(1234, 0, 3, True, 0)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("batch ")]
    assert len(lines) == 2
    for line in lines:
        words = line.split()
        ae, disc = float(words[words.index("aeloss") + 1]), float(words[words.index("discloss") + 1])
        assert abs(ae) < float("inf") and abs(disc) < float("inf"), line


def test_injected_noise_still_wins_and_the_pretraining_phase_runs(env):
    """With the option on, a tensor in injected_noise replaces its stream (the forward then takes the chain of launches, the other
    streams from the fill): an injected z_noise of zeros gives the values of a forward without the noise add at the same call.  And before
    encoder_pretrain_steps, where z_obj feeds nothing, the forward still draws bbox_eps on the device and returns the zero reconstruction."""
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    model = pose_model(device_noise=1234, disc_factor=0.0)
    model.eval()
    model._global_step = 1
    rgb = model._rgb_input(synthetic.make_batch(2, 64, seed=5))
    with torch.no_grad():
        fused_out = model.forward(rgb)[0]
        model._noise_calls.at = None      # the same call again
        model.injected_noise = {"z_noise": torch.zeros(2, 16, 4, 4)}
        injected = model.forward(rgb)[0]
        model._noise_calls.at = None
        model.injected_noise = None
        model.add_noise_to_z_obj = False
        without = model.forward(rgb)[0]
    assert torch.equal(injected, without) and not torch.equal(injected, fused_out)
    torch.manual_seed(23)
    mcfg, _ = synthetic.model_config(POSE_YAML, latent_hw=4, ch=32, phase="asis")
    mcfg.params["device_noise"] = 1234
    early = instantiate_from_config(mcfg).to(DEV).train()
    assert early.global_step < early.encoder_pretrain_steps
    before = torch.get_rng_state()
    dec_obj, dec_pose, _, bbox_posterior = early.forward(rgb)
    assert torch.equal(torch.get_rng_state(), before)
    assert not dec_obj.any() and torch.isfinite(dec_pose).all() and early.dropout_prob == early.dropout_prob_init
    other = early.forward(rgb)[1]      # the next call of the same step: another bbox_eps
    assert not torch.equal(other[:, :8], dec_pose[:, :8]) and torch.equal(other[:, 8:], dec_pose[:, 8:])
