"""The offset rule applied to BatchNorm must be satisfiable and must be able to fail (CPU only).

Host stand-ins take the place of the kernels: torch f32 itself and a two-pass f32 evaluation (both centred) must lie inside the
acceptance rule of `gn_offset_inputs` at every rung and every shape of tests/test_batchnorm_offset_gpu.py; the one-pass model --
sequential f32 sums of x and x^2 per thread of `bn_colstats_kernel`, f64 combine, var = E[x^2] - E[x]^2: what the BatchNorm statistics
kernel was -- must be REJECTED from r = 64 on.  The generated tensors are checked too.
"""
import pytest
import torch

import bn_offset_inputs as B
import gn_offset_inputs as G


def _figures(x, mean, rstd):
    """the three forward quantities of the rule for statistics (mean, rstd) applied exactly (gamma = 1, beta = 0, no activation)"""
    mean64, _, rstd64 = B.stats64(x)
    _, _, _, mean32, rstd32 = B.ref32(x)
    return [G.figure("xhat", B.normalise(x, mean, rstd), B.normalise(x, mean64, rstd64), B.normalise(x, mean32, rstd32), G.FLOOR_FWD)] \
        + G.stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32)


@pytest.mark.parametrize("rung", B.RUNGS, ids=G.rung_id)
@pytest.mark.parametrize("shape", B.MODEL_SHAPES, ids=B.shape_id)
def test_generated_ratio_is_the_nominal_one(shape, rung):
    r, s = rung
    x = B.make_input(shape, r, s)
    assert x.dtype == torch.float32 and tuple(x.shape) == shape
    assert torch.equal(x, B.make_input(shape, r, s))                       # seeded per case
    got = B.realised_ratio(x)
    if r == 0:
        # the mean of m >= 36 standard normal values has std <= 1/6: 4 sigma
        assert got.max().item() <= 0.75
    else:
        assert r / 2 <= got.min().item() and got.max().item() <= 2 * r
        mean64 = B.stats64(x)[0]
        assert (mean64[0::2] > 0).all() and (mean64[1::2] < 0).all()       # the sign alternates by channel


def test_launch_geometry():
    assert B.launch_geometry(90, 128) == (90, 2)
    assert B.launch_geometry(512, 64) == (128, 4)
    assert B.launch_geometry(36, 512) == (36, 1)
    assert B.launch_geometry(126, 96) == (126, 2)
    assert B.launch_geometry(401, 32) == (134, 8)


@pytest.mark.parametrize("rung", B.RUNGS, ids=G.rung_id)
@pytest.mark.parametrize("shape", B.SHAPES, ids=B.shape_id)
def test_torch_and_two_pass_f32_are_inside_the_rule(shape, rung):
    x = B.make_input(shape, *rung)
    gamma, beta = B.affine(shape[1])
    rm, rv = B.running_start(shape[1])
    y32, rm32, rv32, mean32, rstd32 = B.ref32(x, gamma, beta, rm, rv)
    y64, rm64, rv64 = B.ref64(x, gamma, beta, rm, rv)
    G.check(_figures(x, mean32, rstd32), "torch statistics, exact apply")
    G.check([G.figure("lrelu(y)", y32, y64, y32, G.FLOOR_FWD)], "torch f32")
    G.check(_figures(x, *B.two_pass_f32(x)), "two-pass f32")
    assert torch.isfinite(rm32).all() and torch.isfinite(rv32).all() and rm64.dtype == torch.float64 and rv64.dtype == torch.float64


@pytest.mark.parametrize("rung", [rg for rg in B.RUNGS if rg[0] >= 64], ids=G.rung_id)
@pytest.mark.parametrize("shape", B.MODEL_SHAPES, ids=B.shape_id)
def test_the_one_pass_model_is_rejected_from_r_64_on(shape, rung):
    x = B.make_input(shape, *rung)
    figs = _figures(x, *B.one_pass_model(x))
    assert not G.inside(figs[0]), "normalised output: err %.3e inside bound %.3e" % (figs[0]["err"], figs[0]["bound"])
    assert not G.inside(figs[2]), "rstd: err %.3e inside bound %.3e" % (figs[2]["err"], figs[2]["bound"])
    with pytest.raises(AssertionError, match="OUTSIDE|bound"):
        G.check(figs, "one-pass model")


@pytest.mark.parametrize("rung", [rg for rg in B.RUNGS if rg[0] <= 4], ids=G.rung_id)
@pytest.mark.parametrize("shape", B.MODEL_SHAPES, ids=B.shape_id)
def test_the_one_pass_model_is_fine_near_zero_mean(shape, rung):
    x = B.make_input(shape, *rung)
    G.check(_figures(x, *B.one_pass_model(x)), "one-pass model")
