"""Checks shared by the host and the device tests of the device-side latent noise (odvae_amd/latent_noise.py, csrc/latent_noise.h):
the statistics of 2^20 normals with their caps, and the comparison of a filled array with the numpy mirror.

s.e. = standard error of the statistic under N(0, 1) i.i.d. draws, n = sample size:
  mean 1/sqrt(n); variance sqrt(2/n); kurtosis sqrt(24/n); a lag-k autocorrelation and a correlation of two samples 1/sqrt(n).
Kolmogorov-Smirnov: sqrt(n) * sup|F_n - Phi| <= 1.95 (the 0.1 % point of the Kolmogorov distribution)."""
import numpy as np
import torch

from odvae_amd import latent_noise as ln

SEED = 1234
N_STATS = 1 << 20
WORDS = [(0, 0), (7, 0), (7, 0x50000005)]       # (step word, tag)
CAP_SE = 4.0
CAP_KS = 1.95
# |device - float64 mirror| over the draws of the fill tests (n in {1, 3, 4, 5, 1023} x first in {0, 1, 2, 3, 2^34 - 6} x the three
# (step, tag) above, and the 8 388 613 normals past the grid cap): measured 7.448e-07 on an MI355X (profiles/device_noise.md); the gate is
# 4 x that.  For scale: one f32 rounding of a value of 4 to 5.77 is 2.4e-7 on its own, and logf, sincospif and the product each add theirs.
NORMAL_ABS_BOUND = 4 * 7.448e-07


def draw_of(step, tag, rank=0):
    return ln.Draw(ln.device_key(SEED, rank), step, tag)


def phi(x):
    return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def normal_statistics(x):
    """{name: value in units of its s.e.} and the KS figure of a sample that claims to be N(0, 1) i.i.d."""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    m, v = x.mean(), x.var()
    c = x - m
    out = {"mean": m * np.sqrt(n), "var": (v - 1.0) / np.sqrt(2.0 / n), "kurtosis": ((c ** 4).mean() / v ** 2 - 3.0) / np.sqrt(24.0 / n)}
    for lag in (1, 2, 3, 4):
        out["autocorr%d" % lag] = (c[:-lag] * c[lag:]).mean() / v * np.sqrt(n)
    s = np.sort(x)
    cdf = phi(s)
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max((i / n - cdf).max(), (cdf - (i - 1) / n).max()) * np.sqrt(n)
    return out, ks


def correlation_se(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return np.corrcoef(a, b)[0, 1] * np.sqrt(a.size)


def assert_normal_statistics(x, what):
    stats, ks = normal_statistics(x)
    print(what, {k: round(float(v), 3) for k, v in stats.items()}, "KS*sqrt(n) %.3f" % ks)
    for name, v in stats.items():
        assert abs(v) <= CAP_SE, "%s: %s is %.2f s.e. from its expectation" % (what, name, v)
    assert ks <= CAP_KS, "%s: KS distance * sqrt(n) = %.3f" % (what, ks)


def assert_normals_match_mirror(values, draw, first, bound=NORMAL_ABS_BOUND):
    """values: what a fill (or a stand-in for one) produced for elements first .. first + len - 1 of the normal stream in draw.tag"""
    values = np.asarray(values, dtype=np.float64).ravel()
    want = ln.normals(draw, first, values.size)
    assert np.isfinite(values).all(), "non-finite normals (a zero uniform?)"
    worst = np.abs(values - want).max()
    assert worst <= bound, "normals differ from the float64 mirror by %.3e (bound %.3e)" % (worst, bound)
    return worst


def assert_dropout_matches_mirror(values, draw, first, p):
    values = np.asarray(values, dtype=np.float32).ravel()
    want = ln.dropout_multipliers(draw, first, values.size, p)
    assert np.array_equal(values.view(np.uint32), want.view(np.uint32)), "dropout multipliers differ from the mirror's bits"
