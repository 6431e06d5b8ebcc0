"""BatchNorm2d + LeakyReLU(0.2) held to float64 when a channel's mean is far from zero.

`bn_colstats_kernel<T, 0, V>` (csrc/gan_norm.hip) used to sum x and x^2 in f32 and `bn_finalize_kernel` formed var = E[x^2] - E[x]^2, which
loses ~ u r^2 of the variance, r = |mean| / std of a channel.  The sums are now taken about a per-channel pivot (the channel's value in
row 0), so what is squared is of the size of the spread, not of the mean.

The ladder of tests/gn_offset_inputs.py -- r in {0, 4, 16, 64, 256, 1000} at scales 1 and 0.01 -- runs through `ops.batchnorm_lrelu`
in training mode over shapes that reach every branch of the statistics kernel, under that module's acceptance rule against float64
(eight times torch f32's own error, or a quarter of the project's tolerances): the output, the saved statistics in units of the
channel, the updated running estimates in units of the float64 std and variance, and dx, dgamma, dbeta (whose own sums,
`bn_colstats_kernel<1>`, read mean and rstd from the forward).  profiles/bn_offset.md has the figures with the uncentred sums and now.
"""
import pytest
import torch

import bn_offset_inputs as B
import gn_offset_inputs as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RUNG = pytest.mark.parametrize("rung", B.RUNGS, ids=G.rung_id)
SHAPE = pytest.mark.parametrize("shape", B.SHAPES, ids=B.shape_id)


def holder(c, gamma, beta, running_mean, running_var, train):
    bn = torch.nn.BatchNorm2d(c, eps=B.EPS, momentum=B.MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        bn.running_mean.copy_(running_mean); bn.running_var.copy_(running_var)
    return bn.to(DEV).train(train)


def backward_figures(got, refs, prefix=""):
    return [G.figure(prefix + name, v, q64, q32, floor)
            for name, v, q64, q32, floor in zip(("dx", "dgamma", "dbeta"), got, refs[64], refs[32], (G.FLOOR_DX, G.FLOOR_PARAM, G.FLOOR_PARAM))]


def training_figures(x):
    """Every checked quantity of one training-mode forward and backward of the host tensor x; a measuring script can call this too."""
    from odvae_amd import ops
    c = x.shape[1]
    gamma, beta = B.affine(c)
    rm0, rv0 = B.running_start(c)
    mean64, var64, rstd64 = B.stats64(x)
    y64, rm64, rv64 = B.ref64(x, gamma, beta, rm0, rv0)
    y32, rm32, rv32, mean32, rstd32 = B.ref32(x, gamma, beta, rm0, rv0)
    bn = holder(c, gamma, beta, rm0, rv0, True)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.batchnorm_lrelu(xd, bn, B.SLOPE)
    mean, rstd = y.grad_fn.saved_tensors[3:5]              # ops._BatchNormLReLU saves (x, gamma, beta, mean, rstd)
    assert len(y.grad_fn.saved_tensors) == 5 and tuple(mean.shape) == (c,) and tuple(rstd.shape) == (c,) and (rstd > 0).all().item(), \
        "ops._BatchNormLReLU no longer saves (x, gamma, beta, mean, rstd) in that order"
    assert int(bn.num_batches_tracked) == 1
    figs = [G.figure("y", y, y64, y32, G.FLOOR_FWD)] + G.stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32)
    std64 = var64.sqrt()
    figs.append(G.figure("running_mean / std64", bn.running_mean.cpu().double() / std64, rm64 / std64, rm32.double() / std64, G.FLOOR_FWD))
    figs.append(G.figure("running_var / var64", bn.running_var.cpu().double() / var64, rv64 / var64, rv32.double() / var64, G.FLOOR_FWD))
    dy = B.kink_free_dy(B.preact64(x, gamma, beta), G.seed_of(x.shape, 0, 1.0, 19))
    y.backward(dy.to(DEV))
    return figs + backward_figures((xd.grad, bn.weight.grad, bn.bias.grad), B.backward_refs(x, gamma, beta, dy))


def eval_figures(x):
    """Eval mode with the running estimates set to the float64 batch statistics (rounded to f32)"""
    from odvae_amd import ops
    c = x.shape[1]
    gamma, beta = B.affine(c)
    mean64, var64, _ = B.stats64(x)
    running = (mean64.float(), var64.float())
    ys = B.eval_refs(x, gamma, beta, *running)
    bn = holder(c, gamma, beta, running[0], running[1], False)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.batchnorm_lrelu(xd, bn, B.SLOPE)
    assert int(bn.num_batches_tracked) == 0
    assert torch.equal(bn.running_mean.cpu(), running[0]) and torch.equal(bn.running_var.cpu(), running[1])
    figs = [G.figure("eval: y", y, ys[64], ys[32], G.FLOOR_FWD)]
    dy = B.kink_free_dy(B.preact64(x, gamma, beta, running), G.seed_of(x.shape, 0, 1.0, 23))
    y.backward(dy.to(DEV))
    return figs + backward_figures((xd.grad, bn.weight.grad, bn.bias.grad), B.backward_refs(x, gamma, beta, dy, running), "eval: ")


@RUNG
@SHAPE
def test_training_mode_on_the_ladder(hip_lib, shape, rung):
    G.check(training_figures(B.make_input(shape, *rung)), "batchnorm %s %s" % (B.shape_id(shape), G.rung_id(rung)))


@pytest.mark.parametrize("rung", [(0, 1.0), (64, 1.0), (64, 0.01)], ids=G.rung_id)
@SHAPE
def test_eval_mode(hip_lib, shape, rung):
    G.check(eval_figures(B.make_input(shape, *rung)), "batchnorm eval %s %s" % (B.shape_id(shape), G.rung_id(rung)))


# ---- degenerate channels -------------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPE = (3, 128, 6, 5)
DEGENERATE_CHANNELS = (5, 77)


def degenerate_input(kind):
    x = torch.randn(DEGENERATE_SHAPE, generator=torch.Generator().manual_seed(43))
    for ch in DEGENERATE_CHANNELS:
        if kind == "0.75":
            x[:, ch].fill_(0.75)
        else:
            x[:, ch].mul_(1e-3).add_(1.0)
    return x


def test_a_constant_channel_comes_out_as_lrelu_of_beta(hip_lib):
    """0.75 everywhere: the sums are exact, var is exactly 0 and x - mu is exactly 0, so y = lrelu(0 * rstd * gamma + beta), bit for bit"""
    from odvae_amd import ops
    x = degenerate_input("0.75")
    n, c, h, w = DEGENERATE_SHAPE
    gamma, beta = B.affine(c)
    bn = holder(c, gamma, beta, *B.running_start(c), True)
    y = ops.batchnorm_lrelu(x.to(DEV), bn, B.SLOPE).detach().cpu()
    want = torch.where(beta > 0, beta, torch.tensor(B.SLOPE, dtype=torch.float32) * beta)
    for ch in DEGENERATE_CHANNELS:
        assert torch.equal(y[:, ch], want[ch].expand(n, h, w))
    assert torch.isfinite(y).all()


def test_a_channel_of_std_1e_3_around_1_stays_inside_the_rule(hip_lib):
    G.check(training_figures(degenerate_input("std 1e-3 around 1")), "degenerate channel: std 1e-3 around 1")
