"""The device-side latent noise on the host: the numpy mirror (odvae_amd/latent_noise.py) against the repository's Philox, its statistics,
planted faults, the key / call bookkeeping, and the host RNG calls of a model with the option off.  No GPU, no library load."""
import os

import numpy as np
import pytest
import torch

from odvae_amd import dropout_mask
from odvae_amd import latent_noise as ln

import latent_noise_checks as chk

YAML = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")


# ---- the counter layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1, 2, 3, 2 ** 34 - 6])
def test_words_are_the_repository_philox_for_the_counter_layout(first):
    """Element by element with python integers: counter (lo32(g), hi32(g), lo32(step), tag), key (lo32(s), hi32(s)).  first = 2^34 - 6 starts
    at lane 2 of quad 2^32 - 2 and carries into hi32(g) two quads later."""
    step, tag, n = 7, 0x50000005, 13
    draw = chk.draw_of(step, tag, rank=3)
    key = (1234 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert draw.key == key
    w, q, lane = ln.words(draw, first, n)
    seen_hi = set()
    for e in range(n):
        g = (first + e) >> 2
        seen_hi.add(g >> 32)
        want = dropout_mask.philox4x32_10((g & 0xFFFFFFFF, g >> 32, step, tag), (key & 0xFFFFFFFF, key >> 32))
        assert lane[e] == (first + e) & 3
        assert [int(w[j][q[e]]) for j in range(4)] == [int(v) for v in want], (first, e)
    if first > 2 ** 32:
        assert seen_hi == {0, 1}


def test_uniforms_are_exact_in_float32_and_never_zero_or_one():
    u = ln.uniforms(np.array([0, 511, 512, 0xFFFFFFFF], dtype=np.uint32))
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.sqrt(-2.0 * np.log(u.min())) < 5.77      # where the tail ends


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def samples():
    return {(s, t): ln.normals(chk.draw_of(s, t), 0, chk.N_STATS) for s, t in chk.WORDS}


@pytest.mark.parametrize("step,tag", chk.WORDS)
def test_normal_statistics(samples, step, tag):
    chk.assert_normal_statistics(samples[(step, tag)], "mirror step %d tag %#x" % (step, tag))


def test_streams_and_steps_are_uncorrelated(samples):
    base = samples[(7, 0)]
    other_stream = ln.normals(ln.with_stream(chk.draw_of(7, 0), "z_noise"), 0, chk.N_STATS)
    for what, other in (("stream 0 / stream 2 at one call", other_stream), ("step 0 / step 7", samples[(0, 0)]),
                        ("call 0 / stream 2 call 5 (training)", samples[(7, 0x50000005)])):
        c = chk.correlation_se(base, other)
        print(what, "%.3f s.e." % c)
        assert abs(c) <= chk.CAP_SE, what


@pytest.mark.parametrize("p", [0.3, 0.7, 0.999])
def test_dropout_keep_rate(p):
    n = chk.N_STATS
    m = ln.dropout_multipliers(ln.with_stream(chk.draw_of(7, 0), "dropout"), 0, n, p)
    assert set(np.unique(m).tolist()) <= {0.0, float(np.float32(1.0 / (1.0 - p)))}
    dev = ((m > 0).mean() - (1.0 - p)) / np.sqrt(p * (1.0 - p) / n)
    print("p = %g: keep rate %.3f s.e. off" % (p, dev))
    assert abs(dev) <= chk.CAP_SE


def test_dropout_at_zero_keeps_all_and_at_one_keeps_none():
    d = ln.with_stream(chk.draw_of(7, 0), "dropout")
    assert np.array_equal(ln.dropout_multipliers(d, 0, 1 << 16, 0.0), np.ones(1 << 16, dtype=np.float32))
    assert not ln.dropout_multipliers(d, 0, 1 << 16, 1.0).any()
    assert ln.dropout_threshold(1.0) == 2 ** 32 and ln.dropout_scale(1.0) == 0.0


# ---- planted faults: each is a wrong fill that the checks of the device tests must turn down -------------------------------------------
def _faulty_normals(draw, first, n, swap_lanes=False, drop_half=False):
    w, q, lane = ln.words(draw, first, n)
    pair = lane >> 1
    wa = np.where(pair == 0, w[0][q], w[2][q])
    wb = np.where(pair == 0, w[1][q], w[3][q])
    half = 0.0 if drop_half else 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(-2.0 * np.log(((wa >> np.uint32(9)).astype(np.float64) + half) * 2.0 ** -23))
        ang = 2.0 * np.pi * ((wb >> np.uint32(9)).astype(np.float64) + half) * 2.0 ** -23
        even = (lane & 1) == (1 if swap_lanes else 0)
        return np.where(even, r * np.cos(ang), r * np.sin(ang))


def test_the_checks_accept_the_mirror_rounded_to_float32():
    draw = chk.draw_of(7, 0)
    chk.assert_normals_match_mirror(ln.normals(draw, 5, 4096).astype(np.float32), draw, 5)
    d = ln.with_stream(draw, "dropout")
    chk.assert_dropout_matches_mirror(ln.dropout_multipliers(d, 5, 4096, 0.3), d, 5, 0.3)


def test_planted_faults_are_rejected():
    draw = chk.draw_of(7, 0)
    n = 1 << 16
    with pytest.raises(AssertionError, match="differ from the float64 mirror"):      # sine on the even lane
        chk.assert_normals_match_mirror(_faulty_normals(draw, 0, n, swap_lanes=True), draw, 0)
    with pytest.raises(AssertionError, match="differ from the float64 mirror"):      # z_noise's stream where posterior_eps's belongs
        chk.assert_normals_match_mirror(ln.normals(ln.with_stream(draw, "z_noise"), 0, n), draw, 0)
    # the + 0.5 dropped: every value moves, and a zero uniform becomes reachable (a word below 512, 1 in 2^23): Box-Muller's radius is
    # then infinite, which the check turns down as non-finite
    with pytest.raises(AssertionError, match="differ from the float64 mirror"):
        chk.assert_normals_match_mirror(_faulty_normals(draw, 0, n, drop_half=True), draw, 0)
    with np.errstate(divide="ignore"):
        planted = ln.normals(draw, 0, 4)
        planted[0] = np.sqrt(-2.0 * np.log((np.uint32(511) >> np.uint32(9)) * 2.0 ** -23))
    with pytest.raises(AssertionError, match="non-finite"):
        chk.assert_normals_match_mirror(planted, draw, 0)
    assert np.isfinite(np.sqrt(-2.0 * np.log(ln.uniforms(np.uint32(511)))))
    # the 1 / (1 - p) scale omitted
    d = ln.with_stream(draw, "dropout")
    unscaled = (ln.dropout_multipliers(d, 0, n, 0.3) > 0).astype(np.float32)
    with pytest.raises(AssertionError, match="mirror's bits"):
        chk.assert_dropout_matches_mirror(unscaled, d, 0, 0.3)
    # rank ignored in the key
    with pytest.raises(AssertionError, match="differ from the float64 mirror"):
        chk.assert_normals_match_mirror(ln.normals(chk.draw_of(7, 0, rank=0), 0, n), chk.draw_of(7, 0, rank=1), 0)


# ---- key and call ---------------------------------------------------------------------------------------------------------------------
def test_key_differs_per_rank_and_wraps():
    keys = [ln.device_key(1234, r) for r in range(8)]
    assert len(set(keys)) == 8 and keys[0] == 1234
    assert ln.device_key(2 ** 64 - 1, 1) == (2 ** 64 - 1 + 0x9E3779B97F4A7C15) % 2 ** 64 < 2 ** 64
    a, b = (ln.normals(ln.make_draw(1234, r, 7, True, 0), 0, 1 << 16) for r in (0, 1))
    assert abs(chk.correlation_se(a, b)) <= chk.CAP_SE


def test_tag_layout():
    assert ln.make_tag("z_noise", True, 5) == 0x50000005
    assert ln.make_tag(0, False, 0x1FFFFFFF) == 0x0FFFFFFF
    assert [ln.STREAMS[k] for k in ("posterior_eps", "dropout", "z_noise", "bbox_eps", "samples_eps")] == [0, 1, 2, 3, 4]
    d = ln.make_draw(1234, 0, 2 ** 32 + 7, True, 3)
    assert d == ln.Draw(1234, 7, 0x10000003) and ln.with_stream(d, "samples_eps").tag == 0x90000003


def test_call_resets_when_global_step_or_training_changes():
    c = ln.CallCounter()
    assert [c.next(5, True) for _ in range(3)] == [0, 1, 2]      # the micro-batches of an accumulation window
    assert c.next(6, True) == 0
    assert [c.next(6, False), c.next(6, False)] == [0, 1]        # validation batches
    assert c.next(6, True) == 0


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def _pose_model(**params):
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    torch.manual_seed(23)
    mcfg, _ = synthetic.model_config(YAML, latent_hw=4, ch=32)
    for k, v in params.items():
        mcfg.params[k] = v
    return instantiate_from_config(mcfg)


def test_model_call_counter_follows_global_step_and_training():
    model = _pose_model(device_noise=1234)
    assert model.device_noise == 1234 and model.noise_rank == 0
    model.train()
    model._global_step = 4
    draws = [model._next_draw(), model._next_draw()]
    assert draws == [ln.make_draw(1234, 0, 4, True, 0), ln.make_draw(1234, 0, 4, True, 1)]
    model._global_step = 5
    assert model._next_draw() == ln.make_draw(1234, 0, 5, True, 0)
    model.eval()
    assert model._next_draw() == ln.make_draw(1234, 0, 5, False, 0)
    model.noise_rank = 2
    assert model._next_draw().key == ln.device_key(1234, 2)
    assert not any("noise" in k for k in model.state_dict()), "the call counter must not be state"
    assert _pose_model().device_noise is None and _pose_model()._next_draw() is None


@pytest.mark.parametrize("p,expected", [(0.7, ["randn", "rand", "randn", "randn"]), (1.0, ["randn", "randn", "randn"]), (0.0, ["randn", "randn", "randn"])])
def test_option_off_makes_the_parents_host_rng_calls_in_the_parents_order(monkeypatch, p, expected):
    """device_noise=None: posterior_eps, the dropout mask (only for 0 < p < 1), z_noise, bbox_eps -- torch.randn / torch.rand with these
    shapes in this order, as before the option existed.  The network and the kernels are stood in for: only forward's own code runs."""
    from odvae_amd import autoencoder as ae
    from odvae_amd.distributions import DiagonalGaussianDistribution
    model = _pose_model()
    assert getattr(model, "device_noise", None) is None
    model._global_step = 1
    monkeypatch.setattr(model, "_get_dropout_prob", lambda: p)
    g = torch.Generator().manual_seed(1)
    moments, pose_feat = torch.randn(2, 32, 4, 4, generator=g), torch.randn(2, 16, 4, 4, generator=g)
    monkeypatch.setattr(model, "encode", lambda x: (DiagonalGaussianDistribution(moments), pose_feat))
    class PoseDecoderStandIn(torch.nn.Module):
        def forward(self, flat):
            return torch.zeros(flat.shape[0], 2 * ae.BBOX_DIM + model.num_classes)

    monkeypatch.setattr(model, "pose_decoder", PoseDecoderStandIn())
    monkeypatch.setattr(model, "_encode_pose", lambda dec_pose: torch.zeros(2, 16, 4, 4))
    monkeypatch.setattr(model, "decode", lambda z: z)
    monkeypatch.setattr(ae.ops, "latent_combine", lambda z, mask=None, add=None: (z if mask is None else z * mask) + (0 if add is None else add))
    calls = []
    real_randn, real_rand = torch.randn, torch.rand
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (calls.append(("randn", tuple(a[0]))), real_randn(*a, **k))[1])
    monkeypatch.setattr(torch, "rand", lambda *a, **k: (calls.append(("rand", tuple(a[0]))), real_rand(*a, **k))[1])
    model.forward(torch.zeros(2, 3, 64, 64))
    assert [c[0] for c in calls] == expected
    assert [c[1] for c in calls] == [(2, 16, 4, 4)] * (len(expected) - 1) + [(2, 8)]


def test_option_off_plain_model_draws_posterior_eps_then_samples_eps(monkeypatch):
    """The plain Autoencoder with device_noise=None: one torch.randn per forward (posterior_eps), and log_images adds one for `samples`,
    after its forward's -- the parent's calls in the parent's order (network and kernels stood in for)."""
    from odvae_amd.config import Config, instantiate_from_config
    from odvae_amd.distributions import DiagonalGaussianDistribution
    dots = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
            "model.params.ddconfig.resolution=32"]
    config = Config.merge(Config.load(os.path.join(os.path.dirname(YAML), "autoencoder_kl_plain.yaml")), Config.from_dotlist(dots))
    model = instantiate_from_config(config.model)
    assert getattr(model, "device_noise", None) is None
    zc = model.embed_dim
    moments = torch.randn(2, 2 * zc, 16, 16, generator=torch.Generator().manual_seed(1))
    monkeypatch.setattr(model, "encode", lambda x: DiagonalGaussianDistribution(moments))
    monkeypatch.setattr(model, "decode", lambda z: z)
    monkeypatch.setattr(model, "get_input", lambda batch, k: batch[k])
    calls = []
    real_randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (calls.append(tuple(a[0])), real_randn(*a, **k))[1])
    monkeypatch.setattr(torch, "rand", lambda *a, **k: pytest.fail("the plain model never called torch.rand"))
    model.forward(torch.zeros(2, 3, 32, 32))
    assert calls == [(2, zc, 16, 16)]
    model.log_images({"image": torch.zeros(2, 3, 32, 32)})
    assert calls == [(2, zc, 16, 16)] * 3
