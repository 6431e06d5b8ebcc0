"""The HBM-bound streaming kernels of csrc/elementwise.hip at their edges, through the C ABI.

Every instantiation of the row softmax and its backward at its upper edge and the next one at its raggedest; grid-stride loops at
the first size at which they wrap; the three branches of the column sum; null-pointer forms, ties and clamp edges.  Where the inputs
make every sum exact the device result must equal the float64 one bit for bit; everything else is held under the acceptance rule of
tests/gn_offset_inputs.py (eight times torch f32's own error, or a quarter of the project's tolerances), small quantities first put in
their own units.  Outputs are allocated with canary elements behind them and pre-filled with NaN, so an element a kernel skips, or
one it writes past the end, shows.  profiles/streaming_edges.md has the measured figures and the mutations each family was shown
to catch.
"""
import itertools

import numpy as np
import pytest
import torch

from canary_buffers import DEV, assert_canary, assert_workspace_canary, call, out_buf, padded, workspace
import gn_offset_inputs as G
import streaming_inputs as S

pytestmark = pytest.mark.gpu
ERR_WORKSPACE = 2       # ODVAE_ERR_WORKSPACE


# ---- row softmax, forward ------------------------------------------------------------------------------------------------------------
SOFTMAX_COLS = [4, 8, 252, 1020, 1024, 1028, 2048, 2052, 4096, 4100, 16384, 16388, 20484]
SCALES = [64 ** -0.5, 1.0]


def softmax_figures(got, x, scale):
    refs = S.softmax_refs(x, scale)
    q64, q32, g = S.row_units(refs[64], refs[32], got.cpu())
    ones = torch.ones(x.shape[0], dtype=torch.float64)
    return [G.figure("p / row max", g, q64, q32, G.FLOOR_FWD),
            G.figure("row sums", got.cpu().double().sum(1), ones, refs[32].double().sum(1), G.FLOOR_FWD)]


def run_softmax(L, x, scale, pred=None, in_place=False):
    """(y, ones | None, buffers to check)"""
    rows, cols = x.shape
    xb, xd = padded(x)
    yb, y = (xb, xd) if in_place else out_buf(rows * cols)
    y = y.view(rows, cols)
    if pred is None:
        call(L.odvae_softmax_rows_f32, xd.data_ptr(), y.data_ptr(), rows, cols, float(scale))
        return y, None, (xb, yb)
    ob, ones = out_buf(rows, fill=-3.0)
    flag = torch.tensor([pred], dtype=torch.int32, device=DEV)
    call(L.odvae_softmax_rows_pred_f32, xd.data_ptr(), y.data_ptr(), rows, cols, float(scale), flag.data_ptr(), ones.data_ptr())
    return y, ones, (xb, yb, ob)


def fallbacks(L):
    torch.cuda.synchronize()
    return L.odvae_attn_softmax_fallbacks(0)


def check_softmax(L, rows, cols, a, scale, plain=True, predicated=True):
    x = S.softmax_input(rows, cols, a)
    tag = "softmax %dx%d a=%g scale=%g" % (rows, cols, a, scale)
    y = None
    if plain:
        before = fallbacks(L)
        y, _, bufs = run_softmax(L, x, scale)
        G.check(softmax_figures(y, x, scale), tag)
        assert_canary(*bufs)
        assert fallbacks(L) == before                       # only a predicated launch counts itself
    if predicated:
        before = fallbacks(L)
        yp, ones, bufs = run_softmax(L, x, scale, pred=1)
        assert fallbacks(L) == before + 1
        assert (ones == 1.0).all().item()
        G.check(softmax_figures(yp, x, scale), tag + " pred=1")
        assert_canary(*bufs)
        if y is not None:
            assert torch.equal(y, yp)
        y0, ones0, bufs = run_softmax(L, x, scale, pred=0)
        assert fallbacks(L) == before + 1                   # the counter does not move
        assert torch.isnan(y0).all().item() and (ones0 == -3.0).all().item()
        assert_canary(*bufs)


@pytest.mark.parametrize("scale", SCALES, ids=["C64", "one"])
@pytest.mark.parametrize("a", [1.0, 30.0])
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_forward_every_instantiation(hip_lib, cols, a, scale):
    check_softmax(hip_lib, 3, cols, a, scale)


@pytest.mark.parametrize("rows,cols,pred", [(2048 + 5, 8, True), (262144 + 3, 4, False)], ids=["predicated-grid", "plain-grid"])
def test_softmax_forward_row_loop_wraps(hip_lib, rows, cols, pred):
    for a, scale in itertools.product([1.0, 30.0], SCALES):
        check_softmax(hip_lib, rows, cols, a, scale, plain=not pred, predicated=pred)


@pytest.mark.parametrize("cols", [8, 1028, 4100, 16388, 20484])
def test_softmax_forward_in_place(hip_lib, cols):
    x = S.softmax_input(3, cols, 30.0)
    y, _, bufs = run_softmax(hip_lib, x, 1.0, in_place=True)
    G.check(softmax_figures(y, x, 1.0), "softmax in place, %d columns" % cols)
    assert_canary(*bufs)


# ---- row softmax, backward -----------------------------------------------------------------------------------------------------------
SOFTMAX_BWD_COLS = [4, 252, 1024, 1028, 2052, 4100, 8192, 8196, 12292]


def check_softmax_bwd(L, rows, cols, scale, in_place=False):
    p, dp = S.softmax_bwd_case(rows, cols)
    refs = S.softmax_bwd_refs(p, dp, scale)
    pb, pd = padded(p)
    db, dd = padded(dp)
    sb, ds = (db, dd) if in_place else out_buf(rows * cols)
    call(L.odvae_softmax_rows_bwd_f32, pd.data_ptr(), dd.data_ptr(), ds.data_ptr(), rows, cols, float(scale))
    q64, q32, got = S.row_units(refs[64], refs[32], ds.view(rows, cols).cpu())
    G.check([G.figure("dS / row max", got, q64, q32, G.FLOOR_DX)], "softmax backward %dx%d scale=%g%s" % (rows, cols, scale, " in place" if in_place else ""))
    assert_canary(pb, db, sb)
    assert torch.equal(pd.cpu(), p)


@pytest.mark.parametrize("scale", SCALES, ids=["C64", "one"])
@pytest.mark.parametrize("cols", SOFTMAX_BWD_COLS)
def test_softmax_backward_every_instantiation(hip_lib, cols, scale):
    check_softmax_bwd(hip_lib, 3, cols, scale)


def test_softmax_backward_row_loop_wraps(hip_lib):
    check_softmax_bwd(hip_lib, 262144 + 3, 4, 0.125)


@pytest.mark.parametrize("cols", [4, 1028, 8196, 12292])
def test_softmax_backward_in_place(hip_lib, cols):
    check_softmax_bwd(hip_lib, 3, cols, 0.125, in_place=True)


# ---- column sums ---------------------------------------------------------------------------------------------------------------------
COLSUM_C = [4, 12, 96, 256, 1024] + [1, 3, 6, 255] + [260, 1028, 2048, 257]      # quad, scalar and strided branch
COLSUM_CASES = [(r, c) for c in COLSUM_C for r in (1, 63, 65, 4099)] + [(65536 + 129, 8), (70001, 3)]


def check_colsum(L, rows, c, misalign=False):
    x = S.ints(S.gen(rows, c, 13), (rows, c), -8, 8)
    S.assert_exact_sums(8.0, rows)
    want = x.double().sum(0).float()
    xd = x.to(DEV)
    if misalign:                                            # a slice starting at element 1: 4 bytes off a 16-byte boundary
        base = torch.empty(rows * c + 1, device=DEV)
        xd = base[1:].view(rows, c)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4
    need = L.odvae_colsum_workspace_bytes(rows, c)
    ws = workspace(need)
    ob, out = out_buf(c)
    call(L.odvae_colsum_f32, xd.data_ptr(), rows, c, out.data_ptr(), ws.data_ptr(), need)
    assert torch.equal(out.cpu(), want), "colsum %dx%d: max |diff| %g" % (rows, c, (out.cpu() - want).abs().max().item())
    assert_canary(ob)
    assert_workspace_canary(ws)
    from odvae_amd import lib
    assert L.odvae_colsum_f32(xd.data_ptr(), rows, c, out.data_ptr(), ws.data_ptr(), need - 1, lib.stream_ptr()) == ERR_WORKSPACE


@pytest.mark.parametrize("rows,c", COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_exact(hip_lib, rows, c):
    check_colsum(hip_lib, rows, c)


@pytest.mark.parametrize("rows", [1, 63, 65, 4099])
def test_colsum_exact_from_a_pointer_off_the_16_byte_grid(hip_lib, rows):
    check_colsum(hip_lib, rows, 64, misalign=True)


# ---- row dot products and the attention row bound ------------------------------------------------------------------------------------
ROWDOT_CASES = [(r, c) for c in (4, 64, 256, 260, 516) for r in (1, 3, 5)] + [(262144 + 5, 4)]


@pytest.mark.parametrize("rows,cols", ROWDOT_CASES, ids=lambda v: str(v))
def test_rowdot_exact(hip_lib, rows, cols):
    L = hip_lib
    g = S.gen(rows, cols, 17)
    a, b = S.ints(g, (rows, cols), -8, 8), S.ints(g, (rows, cols), -8, 8)
    rs = torch.randn(rows, generator=g)
    S.assert_exact_sums(64.0, cols)
    want = (a.double() * b.double()).sum(1).float()
    ad, bd, rd = a.to(DEV), b.to(DEV), rs.to(DEV)
    ob, out = out_buf(rows)
    call(L.odvae_rowdot_f32, ad.data_ptr(), bd.data_ptr(), rows, cols, out.data_ptr())
    assert torch.equal(out.cpu(), want)
    o2b, out2 = out_buf(rows)
    sb, scaled = out_buf(rows * cols)
    call(L.odvae_rowdot_scale_f32, ad.data_ptr(), bd.data_ptr(), rd.data_ptr(), rows, cols, out2.data_ptr(), scaled.data_ptr())
    assert torch.equal(out2.cpu(), want)
    assert torch.equal(scaled.view(rows, cols).cpu(), a * rs.view(rows, 1))
    assert_canary(ob, o2b, sb)


@pytest.mark.parametrize("t,c", [(t, c) for c in (4, 64, 256, 260, 516) for t in (1, 3, 5)] + [(87383, 4)], ids=lambda v: str(v))
def test_attn_row_bound(hip_lib, t, c):
    """bound_i >= max_j |q_i . k_j| (float64) for every row, and no looser than (1 + 1e-5) |q_i| max_j |k_j| of the row's OWN image:
    the kernel's factor is 1.000001; the slack above it covers the rounding of two f32 norms over C <= 516 terms (at most three
    products and six shuffle additions per lane and norm, 2^-24 each, halved by the square root: < 2e-6 in all)."""
    L = hip_lib
    n = 3
    g = S.gen(t, c, 19)
    qkv = torch.randn(n, t, 3 * c, generator=g) * torch.tensor([1.0, 3.0, 0.25]).view(n, 1, 1)     # the images' maxima differ
    qd = qkv.to(DEV)
    bb, bound = out_buf(n * t)
    kb, nk = out_buf(n * t)
    flag = torch.tensor([7], dtype=torch.int32, device=DEV)
    call(L.odvae_attn_row_bound_f32, qd.data_ptr(), n, t, c, bound.data_ptr(), nk.data_ptr(), flag.data_ptr())
    assert flag.item() == 0
    assert_canary(bb, kb)
    got = bound.view(n, t).cpu().double()
    q, k = qkv[:, :, :c].double(), qkv[:, :, c:2 * c].double()
    qd64, kd64 = q.to(DEV), k.to(DEV)                      # every row against every key, float64, 2048 query rows at a time
    scores = torch.cat([torch.einsum("nic,njc->nij", qd64[:, i:i + 2048], kd64).abs().amax(2) for i in range(0, t, 2048)], 1).cpu()
    assert (got >= scores).all().item(), "a bound lies below a score"
    upper = q.norm(dim=2) * k.norm(dim=2).amax(1, keepdim=True)
    excess = (got / upper - 1.0).max().item()
    print("attn_row_bound T=%d C=%d: bound / (|q| max|k|) - 1 in [%.3e, %.3e]" % (t, c, (got / upper - 1.0).min().item(), excess))
    assert (got >= upper * (1.0 - 1e-5)).all().item() and excess <= 1e-5


# ---- gradient norm and Adam ----------------------------------------------------------------------------------------------------------
NORM_SIZES = [1, 3, 4, 5, 1023, 262144 * 4 + 3, 8388608 + 7]


def run_grad_norm(L, gd, n, max_norm):
    ws = workspace(1024 * 4)
    ob, out = out_buf(2)
    call(L.odvae_grad_norm_f32, gd.data_ptr(), n, float(max_norm), out.data_ptr(), ws.data_ptr(), 1024 * 4)
    assert_canary(ob)
    assert_workspace_canary(ws)
    return out.cpu()


@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_norm_exact_and_clip_coefficient(hip_lib, n):
    g = S.ints(S.gen(n, 23), (n,), -2, 2)
    g[n - 1] = 2.0                                           # the last element counts
    S.assert_exact_sums(4.0, n // 1024 + 1024 + 3)           # the f32 partial of one of the 1024 blocks; they are combined in f64
    total = (g.double() ** 2).sum().item()
    norm = np.float32(np.sqrt(total))
    gd = g.to(DEV)
    for max_norm in (0.0, -1.0, 2.0 * float(norm) + 1.0):    # no clipping asked for; a norm below max_norm
        out = run_grad_norm(hip_lib, gd, n, max_norm)
        assert out[0].item() == float(norm) and out[1].item() == 1.0, "n=%d max_norm=%g: %s" % (n, max_norm, out.tolist())
    max_norm = 0.3 * float(norm)
    out = run_grad_norm(hip_lib, gd, n, max_norm)
    assert out[0].item() == float(norm)
    q64 = torch.tensor([max_norm / (np.sqrt(total) + 1e-6)], dtype=torch.float64)
    q32 = torch.tensor([float(np.float32(max_norm) / (norm + np.float32(1e-6)))], dtype=torch.float32)
    G.check([G.figure("clip coefficient", out[1:2], q64, q32, G.FLOOR_FWD)], "grad_norm n=%d" % n)


ADAM_STEPS, ADAM_BETAS, ADAM_EPS = [1, 2, 1000, 100000], [(0.5, 0.9), (0.9, 0.999)], [1e-8, 1e-3]
ADAM_ALL = list(itertools.product(ADAM_STEPS, ADAM_BETAS, ADAM_EPS, [False, True]))
# at the two sizes that wrap a grid: four settings that between them hold every step, both beta pairs, both eps, clip set and null
ADAM_FEW = [(1, (0.5, 0.9), 1e-8, False), (2, (0.9, 0.999), 1e-3, True), (1000, (0.9, 0.999), 1e-8, True), (100000, (0.5, 0.9), 1e-3, False)]
LR = 1e-2


def check_adam(L, n, step, betas, eps, clip):
    p, g, m, v = S.adam_case(n)
    coef = 0.37 if clip else 1.0
    refs = S.adam_refs(p, g, m, v, LR, betas[0], betas[1], eps, step, float(np.float32(coef)))
    (pb, pd), (gb, gd), (mb, md), (vb, vd) = (padded(t) for t in (p, g, m, v))
    cd = torch.tensor([5.0, coef], device=DEV) if clip else None
    call(L.odvae_adam_step_f32, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, LR, betas[0], betas[1], eps, step,
         None if cd is None else cd.data_ptr())
    assert_canary(pb, gb, mb, vb)
    assert torch.equal(gd.cpu(), g)
    pn, mn, vn = pd.cpu(), md.cpu(), vd.cpu()
    z = n // 2
    if n > 1:
        assert pn[z].item() == p[z].item() and mn[z].item() == 0.0 and vn[z].item() == 0.0      # g = m = v = 0: nothing moves
    upd = (pn.double() - p.double()) / LR
    names = ("(p_new - p) / lr", "m / max |m|", "v / max v")
    units = (1.0, G.maxabs(refs[64][1]) or 1.0, G.maxabs(refs[64][2]) or 1.0)          # the moments in units of their largest float64 entry
    G.check([G.figure(nm, got.double() / u, r64 / u, r32.double() / u, G.FLOOR_FWD)
             for nm, got, r64, r32, u in zip(names, (upd, mn, vn), refs[64], refs[32], units)],
            "adam n=%d step=%d betas=%s eps=%g clip=%s" % (n, step, betas, eps, clip))


@pytest.mark.parametrize("n", NORM_SIZES[:5])
def test_adam_step_small(hip_lib, n):
    for step, betas, eps, clip in ADAM_ALL:
        check_adam(hip_lib, n, step, betas, eps, clip)


@pytest.mark.parametrize("setting", ADAM_FEW, ids=lambda s: "step%d-b%g-eps%g-%s" % (s[0], s[1][0], s[2], "clip" if s[3] else "noclip"))
@pytest.mark.parametrize("n", NORM_SIZES[5:])
def test_adam_step_where_the_grid_wraps(hip_lib, n, setting):
    check_adam(hip_lib, n, *setting)


# ---- Gaussian posterior --------------------------------------------------------------------------------------------------------------
# Twice each: with the clamp edges, their f32 neighbours and +-40 planted in every third logvar, and with ordinary (randn) logvars
# throughout.  z and dlogvar are compared in units of each ENTRY's own size (streaming_inputs.gaussian_units); the KL sums of the
# second kind have no e^20 term, so their bound is a few 1e-5 of a sum of terms of size 1.
GAUSSIAN_SHAPES = [(1, 1, 1), (2, 5, 3), (3, 16, 4), (2, 257, 16), (1, 131073, 16)]
GAUSSIAN = pytest.mark.parametrize("n,hw,cz", GAUSSIAN_SHAPES, ids=lambda v: str(v))
KIND = pytest.mark.parametrize("edges", [True, False], ids=["clamp-edges", "ordinary"])


def gaussian_tag(n, hw, cz, edges):
    return "gaussian %dx%dx%d %s" % (n, hw, cz, "edges" if edges else "ordinary")


@KIND
@GAUSSIAN
def test_gaussian_sample(hip_lib, n, hw, cz, edges):
    mom, eps, _, _ = S.gaussian_case(n, hw, cz, edges)
    refs = S.gaussian_refs(mom, eps, None, None)
    md, ed = mom.to(DEV), eps.to(DEV)
    zb, z = out_buf(n * hw * cz)
    call(hip_lib.odvae_gaussian_sample_f32, md.data_ptr(), ed.data_ptr(), z.data_ptr(), n, hw, cz)
    u = S.gaussian_units(mom)[0]
    G.check([G.figure("z / max(1, sigma)", z.view(n, hw, cz).cpu().double() / u, refs[64]["z"] / u, refs[32]["z"].double() / u, G.FLOOR_FWD)],
            gaussian_tag(n, hw, cz, edges))
    assert_canary(zb)


@KIND
@GAUSSIAN
def test_gaussian_kl(hip_lib, n, hw, cz, edges):
    mom, eps, _, _ = S.gaussian_case(n, hw, cz, edges)
    refs = S.gaussian_refs(mom, eps, None, None)
    md = mom.to(DEV)
    klb, kl = out_buf(n)
    call(hip_lib.odvae_gaussian_kl_f32, md.data_ptr(), kl.data_ptr(), n, hw, cz)
    unit = refs[64]["kl"].abs().clamp(min=1.0)               # per sample: a sample is not held to another sample's size
    G.check([G.figure("kl / kl64", kl.cpu().double() / unit, refs[64]["kl"] / unit, refs[32]["kl"].double() / unit, G.FLOOR_FWD)],
            gaussian_tag(n, hw, cz, edges))
    assert_canary(klb)


@KIND
@GAUSSIAN
def test_gaussian_backward(hip_lib, n, hw, cz, edges):
    """dz only, dkl only and both.  A logvar exactly at -30 or 20 passes the gradient, one outside gets exactly 0."""
    L = hip_lib
    mom, eps, dz, dkl = S.gaussian_case(n, hw, cz, edges)
    md, ed, zd, kd = mom.to(DEV), eps.to(DEV), dz.to(DEV), dkl.to(DEV)
    sigma, sigma2 = S.gaussian_units(mom)
    lraw = mom[:, :, cz:]
    outside = (lraw < -30.0) | (lraw > 20.0)
    edge = (lraw == -30.0) | (lraw == 20.0)
    assert edge.any().item() == edges and outside.any().item() == (edges and lraw.numel() > 6)
    for mode, use_dz, use_dkl in (("dz", True, False), ("dkl", False, True), ("both", True, True)):
        r = S.gaussian_refs(mom, eps, dz if use_dz else None, dkl if use_dkl else None)
        db, dmom = out_buf(n * hw * 2 * cz)
        call(L.odvae_gaussian_bwd_f32, md.data_ptr(), ed.data_ptr() if use_dz else None, zd.data_ptr() if use_dz else None,
             kd.data_ptr() if use_dkl else None, dmom.data_ptr(), n, hw, cz)
        got = dmom.view(n, hw, 2 * cz).cpu().double()
        u = sigma2 if use_dkl else sigma                     # the KL term of dlogvar is of size sigma^2, the sample term of size sigma
        r64, r32 = r[64]["dmom"], r[32]["dmom"].double()
        G.check([G.figure("dmean (%s)" % mode, got[:, :, :cz], r64[:, :, :cz], r32[:, :, :cz], G.FLOOR_DX),
                 G.figure("dlogvar / max(1, %s) (%s)" % ("sigma^2" if use_dkl else "sigma", mode), got[:, :, cz:] / u, r64[:, :, cz:] / u,
                          r32[:, :, cz:] / u, G.FLOOR_DX)], gaussian_tag(n, hw, cz, edges))
        assert_canary(db)
        dlv = got[:, :, cz:]
        assert (dlv[outside] == 0.0).all().item(), "a logvar outside the clamp received a gradient"
        assert torch.equal(dlv[edge] != 0.0, r64[:, :, cz:][edge] != 0.0), "a logvar exactly at a clamp edge lost its gradient"


# ---- masked L1 -----------------------------------------------------------------------------------------------------------------------
L1_SHAPES = [(1, 1, 1), (5, 7, 3), (2, 21846, 3), (1, 65536 + 3, 1)]


@pytest.mark.parametrize("mask_kind", ["none", "zero", "random"])
@pytest.mark.parametrize("n,hw,c", L1_SHAPES, ids=lambda v: str(v))
def test_l1_masked_exact(hip_lib, n, hw, c, mask_kind):
    L = hip_lib
    x, xr, mask, g = S.l1_case(n, hw, c, mask_kind)
    want_sum, want_dxr = S.l1_refs(x, xr, mask, g)
    xd, xrd, gd = x.to(DEV), xr.to(DEV), g.to(DEV)
    mk = None if mask is None else mask.to(DEV)
    ws = workspace(n * 256 * 4)
    ob, out = out_buf(n)
    call(L.odvae_l1_masked_sum_f32, xd.data_ptr(), xrd.data_ptr(), None if mk is None else mk.data_ptr(), out.data_ptr(), n, hw, c,
         ws.data_ptr(), n * 256 * 4)
    assert torch.equal(out.cpu(), want_sum), "%s vs %s" % (out.cpu().tolist(), want_sum.tolist())
    assert_workspace_canary(ws)
    db, dxr = out_buf(n * hw * c)
    call(L.odvae_l1_masked_bwd_f32, xd.data_ptr(), xrd.data_ptr(), None if mk is None else mk.data_ptr(), gd.data_ptr(), dxr.data_ptr(), n, hw, c)
    got = dxr.view(n, hw, c).cpu()
    assert torch.equal(got, want_dxr)
    assert (got[xr == x] == 0.0).all().item()                # sign(0) = 0, as in torch
    if mask_kind == "zero":
        assert (out.cpu() == 0.0).all().item() and (got == 0.0).all().item()
    assert_canary(ob, db)
    from odvae_amd import lib
    assert L.odvae_l1_masked_sum_f32(xd.data_ptr(), xrd.data_ptr(), None, out.data_ptr(), n, hw, c, ws.data_ptr(), n * 256 * 4 - 1,
                                     lib.stream_ptr()) == ERR_WORKSPACE


# ---- min/max rescale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["min last, max first", "max last, min first", "all negative"])
@pytest.mark.parametrize("n,c,hw", [(1, 3, 4), (3, 3, 240), (2, 3, 44100)], ids=lambda v: str(v))
def test_rescale_minmax(hip_lib, n, c, hw, kind):
    from odvae_amd import ops
    L = hip_lib
    h, w = (2, hw // 2) if hw == 4 else ((12, 20) if hw == 240 else (210, 210))
    x = torch.randn(n, c, h, w, generator=S.gen(n, c, hw, 29))
    if kind == "all negative":
        x = -x.abs() - 0.5
    else:
        lo, hi = x.min().item() - 1.5, x.max().item() + 2.25
        x.view(-1)[-1], x.view(-1)[0] = (lo, hi) if kind.startswith("min last") else (hi, lo)
    xd = x.to(DEV)
    yb, y = out_buf(x.numel())
    mb, mm = out_buf(2)
    ws = workspace(2 * 1024 * 4)
    call(L.odvae_rescale_minmax_f32, xd.data_ptr(), y.data_ptr(), n, c, hw, mm.data_ptr(), ws.data_ptr(), 2 * 1024 * 4)
    assert mm.cpu().tolist() == [x.min().item(), x.max().item()]
    assert_canary(yb, mb)
    assert_workspace_canary(ws)
    refs = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        xx = x.to(dt)
        refs[bits] = (2.0 * (xx - xx.min()) / (xx.max() - xx.min()) - 1.0).permute(0, 2, 3, 1).contiguous()
    got = y.view(n, h, w, c)
    G.check([G.figure("y", got, refs[64], refs[32], G.FLOOR_FWD)], "rescale %dx%dx%d, %s" % (n, c, hw, kind))
    via_ops = ops.rescale_minmax(xd)
    assert torch.equal(via_ops.permute(0, 2, 3, 1).contiguous(), got)
    assert L.odvae_rescale_minmax_f32(xd.data_ptr(), y.data_ptr(), n, c, hw, mm.data_ptr(), ws.data_ptr(), 2 * 1024 * 4 - 1, 0) == ERR_WORKSPACE


# ---- exact copies and sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,c", [(1, 1), (255, 1), (85, 3), (257, 1), (2097152 + 3, 1), (699052, 3)], ids=lambda v: str(v))
def test_mul_mask_exact(hip_lib, npix, c):
    g = S.gen(npix, c, 31)
    x, m = torch.randn(npix, c, generator=g), torch.randn(npix, generator=g)
    xd, md = x.to(DEV), m.to(DEV)
    yb, y = out_buf(npix * c)
    call(hip_lib.odvae_mul_mask_f32, xd.data_ptr(), md.data_ptr(), y.data_ptr(), npix, c)
    assert torch.equal(y.view(npix, c).cpu(), x * m.view(npix, 1))       # one multiplication, one rounding
    assert_canary(yb)


@pytest.mark.parametrize("with_mask,with_add", list(itertools.product([False, True], [False, True])), ids=lambda v: str(v))
@pytest.mark.parametrize("n", [1, 255, 257, 2097152 + 3])
def test_latent_combine_exact(hip_lib, n, with_mask, with_add):
    g = S.gen(n, 37)
    z, m, a = (S.ints(g, (n,), -8, 8) for _ in range(3))                 # integers: z m + a is exact, fused or not
    want = z * (m if with_mask else 1.0) + (a if with_add else 0.0)
    zd, md, ad = z.to(DEV), m.to(DEV), a.to(DEV)
    ob, out = out_buf(n)
    call(hip_lib.odvae_latent_combine_f32, zd.data_ptr(), md.data_ptr() if with_mask else None, ad.data_ptr() if with_add else None,
         out.data_ptr(), n)
    assert torch.equal(out.cpu(), want)
    assert_canary(ob)


@pytest.mark.parametrize("n,c,hw", [(1, 1, 1), (1, 5, 51), (3, 257, 1), (2, 3, 349526)], ids=lambda v: str(v))
def test_nhwc_to_nchw_exact(hip_lib, n, c, hw):
    x = torch.randn(n, hw, c, generator=S.gen(n, c, hw, 41))
    xd = x.to(DEV)
    yb, y = out_buf(n * c * hw)
    call(hip_lib.odvae_nhwc_to_nchw_f32, xd.data_ptr(), y.data_ptr(), n, c, hw)
    assert torch.equal(y.view(n, c, hw).cpu(), x.permute(0, 2, 1).contiguous())
    assert_canary(yb)


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 4), (2, 3, 5, 12), (1, 7, 9, 260)], ids=lambda v: str(v))
def test_upsample2x_bwd_exact(hip_lib, n, h, w, c):
    du = S.ints(S.gen(n, h, w, c, 43), (n, 2 * h, 2 * w, c), -8, 8)
    want = du.view(n, h, 2, w, 2, c).double().sum((2, 4)).float()
    dd = du.to(DEV)
    ob, dx = out_buf(n * h * w * c)
    call(hip_lib.odvae_upsample2x_bwd_f32, dd.data_ptr(), dx.data_ptr(), n, h, w, c)
    assert torch.equal(dx.view(n, h, w, c).cpu(), want)
    assert_canary(ob)
