"""The acceptance rule on synchronised BatchNorm: it admits the host model of the kernels and rejects the usual mistakes; plumbing.

Host only.  `syncbn_inputs.model` is the synchronised route of csrc/gan_norm.hip in float64 (record -> Chan merge in index order -> dx
with the total count); the reference is float64 BatchNorm on the concatenated shards, and the rule (`gn_offset_inputs.figure`) takes
eight times torch f32's own error against it or the project's floors.  On the ladder r in {0, 64, 1000}, with consecutive shards on
opposite sides of zero, every figure of the model lies inside the rule, and each of `syncbn_inputs.FAULTS` puts the figure it spoils
outside it -- so the inputs the GPU tests use (tests/test_syncbn_gpu.py draws them from the same generator) tell a right merge from a
wrong one.  The plumbing cases need no device either: the yaml key, the list of layers, the state_dict, the argument check.
"""
import pytest
import torch

import gn_offset_inputs as G
import syncbn_inputs as S

LADDER = (0, 64, 1000)
SPLITS = [((1, 1), 8), ((1, 62), 36), ((20, 21, 22), 36), ((20, 21, 22), 512), ((1, 5, 1, 9, 2, 1, 30, 14), 8)]
SPLIT = pytest.mark.parametrize("counts,c", SPLITS, ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else "C%d" % v)

# which figure each fault has to push outside the rule, and the splits on which it can show at all: unequal counts for the weights; for
# the unbiased correction a total small enough that n / (n - 1) of the smallest shard's count and of the total differ by more than
# the floor after the momentum of 0.1 (1 + 1: the one-row rank makes no correction, the total's is 2 -- visible as well)
SPOILS = {"no_delta_term": ("rstd / rstd64", SPLITS),
          "local_unbiased_count": ("running_var / var64", SPLITS),
          "dx_over_local_rows": ("dx", SPLITS),
          "equal_weights": ("mean * rstd64", [SPLITS[1], SPLITS[4]])}


def _names_outside(figs):
    return {f["name"] for f in figs if not G.inside(f)}


@pytest.mark.parametrize("r", LADDER)
@SPLIT
def test_rule_admits_the_model(counts, c, r):
    shards = S.make_shards(counts, c, r)
    ref = S.Reference(shards)
    out = S.model(shards, ref.gamma, ref.beta, ref.rm0, ref.rv0, ref.dys)
    assert out["rows"] == sum(counts)
    # the shards do lie on opposite sides: the union's spread is that of the centres, not of one shard
    if r:       # (the least of these splits, 1 + 62: var = 4 (r + SEP)^2 62 / 63^2 + the spread inside the shards)
        assert (ref.var64 > 0.05 * r * r).all(), "the delta^2 term does not carry the variance on these inputs"
    G.check(ref.model_figures(out), "model %s C %d r %d" % (counts, c, r))


@pytest.mark.parametrize("r", LADDER)
@pytest.mark.parametrize("fault", S.FAULTS)
def test_rule_rejects_planted_faults(fault, r):
    name, splits = SPOILS[fault]
    for counts, c in splits:
        shards = S.make_shards(counts, c, r)
        ref = S.Reference(shards)
        rank = min(range(len(counts)), key=lambda w: counts[w])      # the rank whose own count is furthest from the total
        good = ref.model_figures(S.model(shards, ref.gamma, ref.beta, ref.rm0, ref.rv0, ref.dys))
        assert not _names_outside(good)
        bad = ref.model_figures(S.model(shards, ref.gamma, ref.beta, ref.rm0, ref.rv0, ref.dys, fault=fault, rank=rank))
        assert name in _names_outside(bad), "%s at %s C %d r %d stays inside the rule: %s" % (
            fault, counts, c, r, [(f["name"], f["err"], f["bound"]) for f in bad])


def test_merge_order_is_the_index_order():
    """Chan's update is not associative in floating point: the model (and the kernel) fix the order, and a different order may give other bits"""
    shards = S.make_shards((20, 21, 22), 36, 1000)
    recs = [S.record64(x) for x in shards]
    n, mu, m2 = S.merge64(recs)
    n2, mu2, m22 = S.merge64(recs)
    assert n == n2 == 63 and torch.equal(mu, mu2) and torch.equal(m2, m22)
    x = S.concat(shards).double()
    v = x.permute(0, 2, 3, 1).reshape(-1, 36)
    assert (mu - v.mean(0)).abs().max().item() <= 1e-12 * 1002 and ((m2 - ((v - v.mean(0)) ** 2).sum(0)).abs() / m2).max().item() <= 1e-12


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def test_trainer_kwargs_passes_the_key_only_when_the_yaml_sets_it():
    from odvae_amd import run
    from odvae_amd.config import Config
    base = {"gradient_clip_val": 1.0, "precision": 32}
    assert "sync_batchnorm" not in run.trainer_kwargs(Config.create(base))
    for value in (True, False):
        kw = run.trainer_kwargs(Config.create(dict(base, sync_batchnorm=value)))
        assert kw["sync_batchnorm"] is value
        assert {k: v for k, v in kw.items() if k != "sync_batchnorm"} == run.trainer_kwargs(Config.create(base))


def test_batchnorm_layers_are_main_3_6_9_and_none_under_actnorm():
    from odvae_amd.gan import NLayerDiscriminator, BatchNormLReLU
    net = NLayerDiscriminator()
    layers = net.batchnorm_layers()
    assert [id(m) for m in layers] == [id(net.main[i]) for i in (3, 6, 9)] and all(isinstance(m, BatchNormLReLU) for m in layers)
    assert all(m.dist_group is None for m in layers)
    assert NLayerDiscriminator(use_actnorm=True).batchnorm_layers() == []
    assert len(NLayerDiscriminator(use_actnorm=True).actnorm_layers()) == 3 and net.actnorm_layers() == []


def test_state_dict_is_unchanged_by_the_switch():
    from odvae_amd.gan import NLayerDiscriminator
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(3)
    net = NLayerDiscriminator()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for m in net.batchnorm_layers():
        m.dist_group = object()         # what the Trainer hands over is no parameter and no buffer
    after = net.state_dict()
    assert list(after) == list(before) == list(RefD().state_dict()) and all(torch.equal(after[k], before[k]) for k in before)
    res = RefD().load_state_dict(after, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


@pytest.mark.parametrize("value", ["True", 1, None, "yes"])
def test_trainer_refuses_a_value_that_is_no_bool(value):
    from odvae_amd.trainer import Trainer
    with pytest.raises(ValueError, match="sync_batchnorm"):
        Trainer(torch.nn.Linear(1, 1), sync_batchnorm=value)
