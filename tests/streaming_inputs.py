"""Inputs and host references for the HBM-bound streaming kernels (csrc/elementwise.hip) at their edges.

Two kinds of check are served (tests/test_streaming_edges_gpu.py):

* exact: operands are small integers or multiples of a power of two, chosen so that every partial sum a kernel could form, in any
  order, is a multiple of one unit and smaller than 2^24 units.  No f32 addition then rounds and the device result must EQUAL the
  float64 result cast to f32.  `assert_exact_sums` asserts that condition on the tensors a test uses.
* the acceptance rule of `gn_offset_inputs` against a float64 evaluation of the f32 inputs, with torch f32 on the host as the
  yardstick; quantities far below 1 are first put in their own units (`row_units`).

Plain module: no fixtures, no device.
"""
import numpy as np
import torch

LIMIT = float(2 ** 24)      # an f32 holds every integer multiple of its unit below 2^24 units


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1))


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def assert_exact_sums(terms_bound, count, unit=1.0):
    """`count` terms of at most `terms_bound` each, all multiples of `unit`: every partial sum stays below 2^24 units"""
    assert count * terms_bound / unit < LIMIT, "%d terms of up to %g (unit %g) are not exactly summable in f32" % (count, terms_bound, unit)


def row_units(q64, *others):
    """rows divided by their float64 max |.| (1 where a row is all zero): (q64 / m, other / m, ...) in float64"""
    m = q64.abs().amax(1, keepdim=True)
    m = torch.where(m > 0, m, torch.ones_like(m))
    return tuple(t.double() / m for t in (q64,) + others)


# ---- row softmax ---------------------------------------------------------------------------------------------------------------------
def softmax_input(rows, cols, a, seed=0):
    """randn a; row 1 (if there is one) holds a single dominant entry in its last column, row 2 is all equal; so are the last two rows"""
    x = torch.randn(rows, cols, generator=gen(rows, cols, a, seed)) * a
    for peaked, flat in ((1, 2), (rows - 2, rows - 1)):
        if 0 <= peaked < rows and rows >= 3:
            x[peaked, cols - 1] = x.max() + 100.0 * a
            x[flat] = 0.37 * a
    return x


def softmax_refs(x, scale):
    """{64, 32}: softmax(scale x) along rows in float64 and in torch f32"""
    return {64: torch.softmax(x.double() * scale, 1), 32: torch.softmax(x * np.float32(scale), 1)}


def softmax_bwd_case(rows, cols, seed=0):
    """(p, dp): p a float64 softmax of a randn rounded to f32, dp randn.  a = 3 for a few rows; a = 1 where there are many: among 2^18
    rows of four some are nearly one-hot at a = 3, and there dP - sum dP P cancels, the whole row of dS is of the size of the f32
    rounding of that sum and torch f32's own error in the row's units (8e-2) leaves the rule nothing to hold"""
    g = gen(rows, cols, seed, 5)
    a = 3.0 if rows <= 16 else 1.0
    p = torch.softmax(a * torch.randn(rows, cols, generator=g).double(), 1).float()
    return p, torch.randn(rows, cols, generator=g)


def softmax_bwd_refs(p, dp, scale):
    out = {}
    for bits, dt, sc in ((64, torch.float64, scale), (32, torch.float32, np.float32(scale))):
        pp, dd = p.to(dt), dp.to(dt)
        out[bits] = sc * pp * (dd - (dd * pp).sum(1, keepdim=True))
    return out


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------
def adam_case(n, seed=0):
    """(p, g, m, v) f32 [n] with non-zero moments carried in; element n // 2 has g = m = v = 0 (not at n = 1: the one element is live)"""
    gg = gen(n, seed, 3)
    p, g = torch.randn(n, generator=gg), torch.randn(n, generator=gg)
    m, v = 0.1 * torch.randn(n, generator=gg), 0.01 * torch.rand(n, generator=gg) + 1e-4
    if n > 1:
        g[n // 2] = 0.0; m[n // 2] = 0.0; v[n // 2] = 0.0
    return p, g, m, v


def adam_refs(p, g, m, v, lr, b1, b2, eps, step, coef):
    """{64, 32}: (update / lr, m, v) of torch.optim.Adam written out, the gradient scaled by `coef` first; bias corrections from pow in
    double.  The update p_new - p is what the step adds to p: the rule holds it in units of lr."""
    out = {}
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        pp, gr, mm, vv = p.to(dt), g.to(dt) * coef, m.to(dt), v.to(dt)
        mm = b1 * mm + (1.0 - b1) * gr
        vv = b2 * vv + (1.0 - b2) * gr * gr
        pn = pp - (lr / bc1) * mm / (vv.sqrt() / np.sqrt(bc2) + eps)
        out[bits] = ((pn.double() - p.double()) / lr, mm, vv)
    return out


# ---- Gaussian posterior --------------------------------------------------------------------------------------------------------------
LOGVAR_MIN, LOGVAR_MAX = np.float32(-30.0), np.float32(20.0)
LOGVAR_SPECIAL = [float(LOGVAR_MIN), float(LOGVAR_MAX),
                  float(np.nextafter(LOGVAR_MIN, np.float32(-np.inf))), float(np.nextafter(LOGVAR_MAX, np.float32(np.inf))), -40.0, 40.0]


def gaussian_case(n, hw, cz, edges=True, seed=0):
    """(moments [n, hw, 2 cz], eps, dz [n, hw, cz], dkl [n]).  edges: every third logvar entry is one of the clamp edges -30 and 20,
    the next f32 outside each, and -40, 40, in turn; otherwise every logvar is randn, so that no term of a sum dwarfs the others"""
    g = gen(n, hw, cz, seed, 7)
    mom = torch.randn(n, hw, 2 * cz, generator=g)
    if edges:
        lv = mom[:, :, cz:].reshape(-1).clone()
        idx = torch.arange(0, lv.numel(), 3)
        lv[idx] = torch.tensor(LOGVAR_SPECIAL, dtype=torch.float32)[(idx // 3) % 6]
        mom[:, :, cz:] = lv.view(n, hw, cz)
    return mom, torch.randn(n, hw, cz, generator=g), torch.randn(n, hw, cz, generator=g), torch.randn(n, generator=g)


def gaussian_units(mom):
    """(max(1, sigma), max(1, sigma^2)) [n, hw, cz] in float64, sigma^2 = exp(clamped logvar): the size of an entry of z and of the
    sample term of dlogvar, and the size of the KL term of dlogvar.  Errors are divided by these ELEMENTWISE, so that an entry with an
    ordinary logvar is held to the floor itself and not to the floor times the e^10 or e^20 of some other entry."""
    lv = mom[:, :, mom.shape[2] // 2:].double().clamp(-30.0, 20.0)
    return torch.exp(0.5 * lv).clamp(min=1.0), torch.exp(lv).clamp(min=1.0)


def gaussian_refs(mom, eps, dz, dkl):
    """{64, 32}: dict(z, kl, dmom) from the written-out formulas; dz / dkl None leaves that term out of dmom"""
    out = {}
    cz = mom.shape[2] // 2
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        mu, lraw = mom[:, :, :cz].to(dt), mom[:, :, cz:].to(dt)
        lv = lraw.clamp(-30.0, 20.0)
        passes = ((lraw >= -30.0) & (lraw <= 20.0)).to(dt)
        r = {"z": mu + torch.exp(0.5 * lv) * eps.to(dt), "kl": 0.5 * (mu * mu + torch.exp(lv) - 1.0 - lv).sum((1, 2))}
        dmu, dlv = torch.zeros_like(mu), torch.zeros_like(mu)
        if dz is not None:
            dmu = dmu + dz.to(dt)
            dlv = dlv + dz.to(dt) * eps.to(dt) * 0.5 * torch.exp(0.5 * lv)
        if dkl is not None:
            gk = dkl.to(dt).view(-1, 1, 1)
            dmu = dmu + gk * mu
            dlv = dlv + gk * 0.5 * (torch.exp(lv) - 1.0)
        r["dmom"] = torch.cat([dmu, dlv * passes], 2)
        out[bits] = r
    return out


# ---- masked L1 -----------------------------------------------------------------------------------------------------------------------
def l1_case(n, hw, c, mask_kind, seed=0):
    """(x, xr [n, hw, c] multiples of 1/8 in [-4, 4], mask [n, hw] | None, g [n]); 5 % of the positions of xr equal x"""
    gg = gen(n, hw, c, seed, 11)
    x, xr = ints(gg, (n, hw, c), -32, 32) / 8, ints(gg, (n, hw, c), -32, 32) / 8
    tie = torch.rand(n, hw, c, generator=gg) < 0.05
    xr = torch.where(tie, x, xr)
    if n * hw * c >= 2:
        xr.view(-1)[-1] = x.view(-1)[-1]          # at least one tie, and one in the last element
    mask = {"none": None, "zero": torch.zeros(n, hw), "random": (torch.rand(n, hw, generator=gg) < 0.5).float()}[mask_kind]
    assert_exact_sums(8.0, hw * c, 0.125)
    return x, xr, mask, torch.randn(n, generator=gg)


def l1_refs(x, xr, mask, g):
    """(sums [n] from float64 cast to f32, dxr in f32: g sign(xr m - x m) m has no rounding)"""
    w = torch.ones(x.shape[:2]) if mask is None else mask
    w3 = w.unsqueeze(2)
    d = (xr * w3 - x * w3).double()
    return d.abs().sum((1, 2)).float(), g.view(-1, 1, 1) * torch.sign(d).float() * w3
