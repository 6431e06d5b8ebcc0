"""The GroupNorm offset rule must be satisfiable and must be able to fail (CPU only).

Host stand-ins take the place of the kernels: torch f32 itself and a two-pass f32 evaluation (both centred) must lie inside the
acceptance rule of `gn_offset_inputs` at every rung; the one-pass model -- sequential f32 sums of x and x^2 per chunk, f64 combine,
var = E[x^2] - E[x]^2: the design of the library's statistics kernels -- must be REJECTED from r = 64 on.  The generated tensors are
checked too: the realised |mean| / std of every (sample, group) lies within a factor 2 of the nominal r.
"""
import pytest
import torch

import gn_offset_inputs as G

# ragged chunks of 128 pixels with 2 channels per group; 8 channels per group; one channel per group, 64 values each
SHAPES = [(2, 64, 16, 32), (1, 256, 20, 36), (2, 32, 8, 8)]
CHUNKS = (64, 128, 256)


def _figures(x, mean, rstd):
    """the three forward quantities of the rule for statistics (mean, rstd) applied exactly (gamma = 1, beta = 0, no swish)"""
    mean64, rstd64 = G.stats64(x)
    y32, mean32, rstd32 = G.ref32(x)
    return [G.figure("y", G.normalise(x, mean, rstd), G.ref64(x), y32, G.FLOOR_FWD)] + G.stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32)


@pytest.mark.parametrize("rung", G.RUNGS, ids=G.rung_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generated_ratio_is_the_nominal_one(shape, rung):
    r, s = rung
    x = G.make_input(shape, r, s)
    assert x.dtype == torch.float32 and tuple(x.shape) == shape
    assert torch.equal(x, G.make_input(shape, r, s))                       # seeded per case
    got = G.realised_ratio(x)
    if r == 0:
        # the mean of m >= 64 standard normal values has std <= 1/8: 4 sigma
        assert got.max().item() <= 0.5
    else:
        assert r / 2 <= got.min().item() and got.max().item() <= 2 * r
    mean64, _ = G.stats64(x)
    if r:
        assert (torch.sign(mean64[:, 0::2]) > 0).all() and (torch.sign(mean64[:, 1::2]) < 0).all()      # the sign alternates by group
    std = x.double().reshape(shape[0], G.GROUPS, -1).std(2)
    assert s / 2 <= std.min().item() and std.max().item() <= 2 * s


@pytest.mark.parametrize("rung", G.RUNGS, ids=G.rung_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_and_two_pass_f32_are_inside_the_rule(shape, rung):
    x = G.make_input(shape, *rung)
    y32, mean32, rstd32 = G.ref32(x)
    G.check(_figures(x, mean32, rstd32), "torch statistics, exact apply")
    G.check([G.figure("y", y32, G.ref64(x), y32, G.FLOOR_FWD)], "torch f32")
    G.check(_figures(x, *G.two_pass_f32(x)), "two-pass f32")
    gm = torch.Generator().manual_seed(5)
    gamma, beta = torch.randn(shape[1], generator=gm), torch.randn(shape[1], generator=gm)
    y32s, _, _ = G.ref32(x, gamma, beta, True)
    G.check([G.figure("swish(y gamma + beta)", y32s, G.ref64(x, gamma, beta, True), y32s, G.FLOOR_FWD)], "torch f32, affine + swish")


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("rung", [rg for rg in G.RUNGS if rg[0] >= 64], ids=G.rung_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_one_pass_model_is_rejected_from_r_64_on(shape, rung, chunk):
    x = G.make_input(shape, *rung)
    figs = _figures(x, *G.one_pass_model(x, chunk))
    assert not G.inside(figs[0]), "normalised output: err %.3e inside bound %.3e" % (figs[0]["err"], figs[0]["bound"])
    assert not G.inside(figs[2]), "rstd: err %.3e inside bound %.3e" % (figs[2]["err"], figs[2]["bound"])
    with pytest.raises(AssertionError, match="OUTSIDE|bound"):
        G.check(figs, "one-pass model")


@pytest.mark.parametrize("rung", [rg for rg in G.RUNGS if rg[0] <= 4], ids=G.rung_id)
def test_the_one_pass_model_is_fine_where_training_is_known_to_be(rung):
    x = G.make_input(SHAPES[0], *rung)
    G.check(_figures(x, *G.one_pass_model(x, 128)), "one-pass model")


def test_the_rule():
    assert G.bound(1e-6, 0.5, G.FLOOR_FWD) == G.FLOOR_FWD                 # the floor, relative to max(1, |q|)
    assert G.bound(1e-6, 4.0, G.FLOOR_FWD) == 4 * G.FLOOR_FWD
    assert G.bound(1e-4, 4.0, G.FLOOR_FWD) == 8e-4                        # eight times torch's own error
    q64 = torch.zeros(4, dtype=torch.float64)
    nan = G.figure("q", torch.tensor([0.0, float("nan"), 0.0, 0.0]), q64, q64.float(), G.FLOOR_FWD)
    assert not G.inside(nan)                                              # a NaN hides behind no comparison
    with pytest.raises(AssertionError):
        G.check([nan])
    with pytest.raises(AssertionError):
        G.figure("q", torch.zeros(3), q64, q64.float(), G.FLOOR_FWD)      # shapes must agree
