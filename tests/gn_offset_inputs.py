"""GroupNorm inputs whose group means lie far from zero: generators, references, host models, the acceptance rule.

The GroupNorm statistics kernels of the library form var = E[x^2] - E[x]^2 from f32 partial sums (the BatchNorm one sums about a
per-channel pivot instead: tests/bn_offset_inputs.py).  The subtraction cancels: the relative error
of the variance grows like u (1 + r^2) with r = |mean| / std of a (sample, group) and u = 2^-24, where a centred (two-pass, Welford)
evaluation grows like u r; `gn_finalize_kernel` therefore recentres the groups whose mean is far from zero.  `torch.nn.GroupNorm`, which the reference model runs, is of the second kind.  This module makes inputs
with a chosen r (`make_input`: x = s (randn + r sign_g), sign_g alternating from one group to the next), the two references every GPU
test of tests/test_groupnorm_offset_gpu.py compares against (`ref64`: float64; `ref32`: torch f32 on the host, what the reference
project computes), two host stand-ins for kernels (`two_pass_f32`: centred; `one_pass_model`: the uncentred design with sequential f32
sums per chunk and an f64 combine), and the acceptance rule (`bound`, `check`):

    |q_hip - q_64|max  <=  max( 8 |q_torch_f32 - q_64|max ,  floor * max(1, |q_64|max) )

The factor 8 separates the two growth laws (tests/test_gn_offset_inputs.py shows the rule accepts torch and a two-pass f32 evaluation
at every rung and rejects the one-pass model from r = 64 on).  The floors are a quarter of the project's per-op tolerances for forward
outputs, statistics and dx -- the rest is left to the other ops of a block -- and test_groupnorm's own tolerance for dgamma / dbeta.
Plain module: no fixtures, no device.  All tensors are NCHW on the host.
"""
import numpy as np
import torch
import torch.nn.functional as F

GROUPS = 32
EPS = 1e-6
RATIOS = (0, 4, 16, 64, 256, 1000)
SCALES = (1.0, 0.01)      # at s = 0.01 the variance is 1e-4 and eps = 1e-6 is 1 % of it: a misplaced eps shows
RUNGS = [(r, s) for r in RATIOS for s in SCALES]
FWD_TOL, BWD_TOL = 2e-4, 5e-4          # tests/test_ops_gpu.py
FLOOR_FWD = FWD_TOL / 4                # forward outputs and the statistics
FLOOR_DX = BWD_TOL / 4
FLOOR_PARAM = BWD_TOL * 4              # dgamma, dbeta: what test_groupnorm uses
FACTOR = 8.0


def rung_id(rung):
    return "r%g-s%g" % rung


def seed_of(shape, r, s, salt=0):
    return (1000003 * salt + 7919 * int(r) + (31 if s != 1.0 else 0) + sum((i + 1) * int(v) for i, v in enumerate(shape))) % (2 ** 31 - 1)


def group_signs(c, groups=GROUPS):
    """[c]: +1 for the channels of even groups, -1 for those of odd groups"""
    return (1.0 - 2.0 * ((torch.arange(c) // (c // groups)) % 2)).float()


def make_input(shape, r, s, seed=None, groups=GROUPS):
    """x = s (randn + r sign_g), f32 [n, c, h, w]; seeded per case"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed_of(shape, r, s) if seed is None else seed)
    return (s * (torch.randn(n, c, h, w, generator=g) + r * group_signs(c, groups).view(1, c, 1, 1))).float()


def stats64(x, groups=GROUPS, eps=EPS):
    """(mean, rstd) [n, groups] in float64 of the values x holds"""
    xg = x.double().reshape(x.shape[0], groups, -1)
    return xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + eps)


def realised_ratio(x, groups=GROUPS):
    """[n, groups]: |mean| / std of the values x holds (float64)"""
    xg = x.double().reshape(x.shape[0], groups, -1)
    return xg.mean(2).abs() / xg.std(2, unbiased=False)


def ref64(x, gamma=None, beta=None, swish=False, groups=GROUPS, eps=EPS):
    y = F.group_norm(x.double(), groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps=eps)
    return F.silu(y) if swish else y


def ref32(x, gamma=None, beta=None, swish=False, groups=GROUPS, eps=EPS):
    """torch f32 on the host: (y, mean, rstd), the statistics as torch.native_group_norm returns them"""
    n, c = x.shape[:2]
    y, mean, rstd = torch.native_group_norm(x.float().contiguous(), gamma, beta, n, c, x[0, 0].numel(), groups, eps)
    return (F.silu(y) if swish else y), mean.reshape(n, groups), rstd.reshape(n, groups)


def backward_refs(x, gamma, beta, dy, swish, dskip=None, groups=GROUPS, eps=EPS):
    """{64: (dx, dgamma, dbeta), 32: (...)} by autograd in float64 and in f32 on the host"""
    out = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        xr, gr, br = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        y = F.group_norm(xr, groups, gr, br, eps=eps)
        (F.silu(y) if swish else y).backward(dy.to(dt))
        out[bits] = (xr.grad + (dskip.to(dt) if dskip is not None else 0.0), gr.grad, br.grad)
    return out


def normalise(x, mean, rstd, groups=GROUPS):
    """(x - mean) rstd in float64 with the given statistics [n, groups]: what an exact apply pass makes of them"""
    n = x.shape[0]
    xg = x.double().reshape(n, groups, -1)
    return ((xg - mean.double().reshape(n, groups, 1)) * rstd.double().reshape(n, groups, 1)).reshape(x.shape)


def two_pass_f32(x, groups=GROUPS, eps=EPS):
    """(mean, rstd) by a centred evaluation in f32 throughout"""
    xg = x.float().reshape(x.shape[0], groups, -1)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2)
    return mean.squeeze(2), 1.0 / torch.sqrt(var + np.float32(eps))


def one_pass_model(x, chunk_pixels=128, groups=GROUPS, eps=EPS):
    """(mean, rstd) the way the kernels' design forms them: per chunk of pixels SEQUENTIAL f32 sums of x and of fl(x * x) over the
    chunk's pixels x channels of the group (numpy's cumulative sum adds in order, in the array's own type), the chunk partials combined
    in float64, var = b / m - mu mu clamped at 0."""
    n, c, h, w = x.shape
    cpg, hw = c // groups, h * w
    chunks = -(-hw // chunk_pixels)
    v = x.float().reshape(n, groups, cpg, hw).permute(0, 1, 3, 2)                       # pixel-major, as NHWC memory is walked
    v = F.pad(v, (0, 0, 0, chunks * chunk_pixels - hw)).reshape(n, groups, chunks, chunk_pixels * cpg).numpy()
    a = np.cumsum(v, axis=-1, dtype=np.float32)[..., -1].astype(np.float64).sum(-1)
    b = np.cumsum(v * v, axis=-1, dtype=np.float32)[..., -1].astype(np.float64).sum(-1)
    m = float(hw * cpg)
    mu = a / m
    var = np.maximum(b / m - mu * mu, 0.0)
    return torch.from_numpy(mu.astype(np.float32)), torch.from_numpy((1.0 / np.sqrt(var + eps)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------
# the acceptance rule
# ------------------------------------------------------------------------------------------------------------------------------
def maxabs(t):
    return t.detach().double().abs().max().item()


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def bound(err_torch, q64_max, floor):
    return max(FACTOR * err_torch, floor * max(1.0, q64_max))


def figure(name, got, q64, q32, floor):
    """One checked quantity: dict(name, err = |got - q64|max, err_torch = |q32 - q64|max, bound, finite)."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(q64.shape), "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(q64.shape))
    err_t = maxerr(q32, q64)
    return {"name": name, "err": maxerr(got, q64), "err_torch": err_t, "bound": bound(err_t, maxabs(q64), floor),
            "finite": bool(torch.isfinite(got).all())}


def stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32, prefix=""):
    """The statistics in units of the group: q = mean rstd_64 (q_64 = mean_64 rstd_64) and q = rstd / rstd_64 (q_64 = 1)."""
    return [figure(prefix + "mean * rstd64", mean.cpu().double() * rstd64, mean64 * rstd64, mean32.double() * rstd64, FLOOR_FWD),
            figure(prefix + "rstd / rstd64", rstd.cpu().double() / rstd64, torch.ones_like(rstd64), rstd32.double() / rstd64, FLOOR_FWD)]


def inside(fig):
    return fig["finite"] and fig["err"] <= fig["bound"]


def check(figs, what=""):
    """Prints every figure, then asserts the rule on each."""
    for f in figs:
        print("%s %-24s err %.3e  torch f32 %.3e  bound %.3e%s" % (what, f["name"], f["err"], f["err_torch"], f["bound"],
                                                                 "" if inside(f) else "   <-- OUTSIDE"))
    bad = [f for f in figs if not inside(f)]
    assert not bad, "%s: %s" % (what, "; ".join("%s: err %.3e > bound %.3e (torch f32 %.3e)%s" % (
        f["name"], f["err"], f["bound"], f["err_torch"], "" if f["finite"] else ", non-finite values") for f in bad))
