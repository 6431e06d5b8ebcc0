"""odvae_rgba_terms_f32 / odvae_rgba_terms_bwd_f32 through the C ABI and through ops.rgba_terms.

Exact part: inputs are multiples of 1/8 (1/2 at the largest size) with {0,1} masks, chosen so that every partial sum of the kernel is
exact in f32 (tests/image_mask_ref.sums_are_exact, asserted here on the host for each size); the two sums and every per-element output
are then bit for bit the float64 answers, whatever the order of the kernel's additions.

Random part: f32 inputs against float64 under a bound counted in roundings of the kernel's arithmetic (u = 2^-24):
  a masked product is one rounding, so xm - rm carries at most u(|xm| + |rm|) from its operands and u|xm - rm| of its own; with
  A = sum over a sample of (|xm| + |rm|) and S = the sample's exact sum, the terms are off by at most u(A + S).  They are added in f32: two
  additions per pixel, a thread's K = ceil(HW / (256 * blocks)) pixels one after another, six butterfly levels and three additions across
  the block's waves -- at most (K + 10) additions on any path, each off by at most u times the partial sum <= S -- then one rounding of the
  f64 total.  |l1_sum - exact| <= u (A + (K + 12) S) (1 + 2^-10) (the last factor covers the second-order terms).
  The squared mask term: d = am - ra is off by u(|am| + |ra|) + u|d|, so d^2 by 2|d| times that plus its own u d^2:
  |mask_sum - exact| <= u (2 D + (K + 14) S) (1 + 2^-10) with D = sum |d| (|am| + |ra|).
  The gradient is ((g * e) * w + g_rgb * w) + g_rgba * w: one rounding per product and per addition, |error| <= 4 u T per element, T the
  sum of the magnitudes of its terms (the squared mask loss's e = 2 d carries d's two roundings: 2 more u of its term).
The per-element outputs are single products: bit for bit the f32 product."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import image_mask_ref as R  # noqa: E402

U = 2.0 ** -24
GRID_CAP_BLOCKS = 256        # kRgbaBlocks of csrc/elementwise.hip: a sample's pixels go over at most this many 256-thread blocks


def dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def call_fwd(L, rec, rgb, alpha, box, l2, skip=(), ws_short=0, fill=None):
    """The forward through the C ABI on device arrays [N][HW][C]; `skip` names outputs passed as NULL.  Returns (status, dict)."""
    from odvae_amd import lib
    n, hw = alpha.shape
    new = lambda *s: torch.full(s, float("nan") if fill is None else fill, dtype=torch.float32, device=DEV)
    out = {"l1_sum": new(n), "mask_sum": new(n), "rec_rgb_m": new(n, hw, 3), "gt_rgb_m": new(n, hw, 3), "rec_rgba_m": new(n, hw, 4),
           "gt_rgba_m": new(n, hw, 4)}
    for k in skip:
        out[k] = None
    nbytes = L.odvae_rgba_terms_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = L.odvae_rgba_terms_f32(rec.data_ptr(), rgb.data_ptr(), alpha.data_ptr(), ptr(box), int(l2), ptr(out["l1_sum"]),
                                ptr(out["mask_sum"]), ptr(out["rec_rgb_m"]), ptr(out["gt_rgb_m"]), ptr(out["rec_rgba_m"]),
                                ptr(out["gt_rgba_m"]), n, hw, ws.data_ptr(), nbytes - ws_short, lib.stream_ptr())
    torch.cuda.synchronize()
    return st, out


def call_bwd(L, rec, rgb, alpha, box, l2, g_l1, g_mask, g_rgb, g_rgba):
    from odvae_amd import lib
    n, hw = alpha.shape
    d_rec = torch.full((n, hw, 4), float("nan"), dtype=torch.float32, device=DEV)
    st = L.odvae_rgba_terms_bwd_f32(rec.data_ptr(), rgb.data_ptr(), alpha.data_ptr(), ptr(box), int(l2), ptr(g_l1), ptr(g_mask), ptr(g_rgb),
                                    ptr(g_rgba), d_rec.data_ptr(), n, hw, lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    return d_rec


def exact_grads(n, hw, seed):
    """Incoming gradients that keep the backward exact: multiples of 1/4 of magnitude <= 2 (times a multiple of 1/8 <= 8: exact)."""
    g = torch.Generator().manual_seed(seed)
    q = lambda *s: torch.randint(-8, 9, s, generator=g).double() / 4.0
    return q(n), q(n), q(n, hw, 3), q(n, hw, 4)


def same(got, want):
    return got is not None and torch.equal(got.double().cpu(), want)


def check_exact(L, n, hw, q, a):
    assert R.sums_are_exact(hw, q, a)
    for with_box in (False, True):
        rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=7 * hw + n, with_box=with_box, q=q, a=a)
        d = [dev(t) for t in (rec, rgb, alpha, box)]
        grads = exact_grads(n, hw, seed=hw + 1)
        for l2 in (False, True):
            want = R.rgba_terms_f64(rec, rgb, alpha, box, l2)
            st, out = call_fwd(L, *d, l2)
            assert st == 0
            for k, w in zip(("l1_sum", "mask_sum", "rec_rgb_m", "gt_rgb_m", "rec_rgba_m", "gt_rgba_m"), want):
                assert same(out[k], w), (k, n, hw, l2, with_box)
            got = call_bwd(L, *d, l2, *[dev(g) for g in grads])
            assert same(got, R.rgba_terms_bwd_f64(rec, rgb, alpha, box, l2, *grads)), (n, hw, l2, with_box)


@pytest.mark.parametrize("hw", [1, 7, 64, 255, 256, 257, 4100])
@pytest.mark.parametrize("n", [1, 3])
def test_exact_inputs_bit_for_bit(hip_lib, n, hw):
    check_exact(hip_lib, n, hw, 8, 2)


def test_exact_past_the_grid_cap(hip_lib):
    """More pixels than blocks * threads: every thread walks several pixels, the last stride is ragged."""
    hw = GRID_CAP_BLOCKS * 256 + 259
    check_exact(hip_lib, 1, hw, 2, 1)


def test_each_optional_output_and_gradient_may_be_null(hip_lib):
    n, hw = 3, 257
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=11)
    d = [dev(t) for t in (rec, rgb, alpha, box)]
    names = ("l1_sum", "mask_sum", "rec_rgb_m", "gt_rgb_m", "rec_rgba_m", "gt_rgba_m")
    want = dict(zip(names, R.rgba_terms_f64(rec, rgb, alpha, box, True)))
    for skip in names[2:] + (names[2:],):
        skip = skip if isinstance(skip, tuple) else (skip,)
        st, out = call_fwd(hip_lib, *d, True, skip=skip)
        assert st == 0
        for k in names:
            assert (out[k] is None) if k in skip else same(out[k], want[k]), (skip, k)
    grads = exact_grads(n, hw, seed=12)
    for drop in range(4):
        g = [None if i == drop else x for i, x in enumerate(grads)]
        got = call_bwd(hip_lib, *d, False, *[dev(x) for x in g])
        assert same(got, R.rgba_terms_bwd_f64(rec, rgb, alpha, box, False, *g)), drop
    got = call_bwd(hip_lib, *d, False, None, None, None, None)
    assert same(got, torch.zeros(n, hw, 4, dtype=torch.float64))


def test_without_the_sums_only_the_copies_are_made(hip_lib):
    """l1_sum = mask_sum = NULL (the discriminator phase): the copies as before, no workspace needed; one of the two alone, or nothing at
    all to compute, is refused."""
    from odvae_amd import lib, ops
    n, hw = 3, 300
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=17)
    d = [dev(t) for t in (rec, rgb, alpha, box)]
    want = R.rgba_terms_f64(rec, rgb, alpha, box, False)
    outs = [torch.full((n, hw, c), float("nan"), device=DEV) for c in (4, 4)]
    st = hip_lib.odvae_rgba_terms_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, None, None, None, None,
                                      outs[0].data_ptr(), outs[1].data_ptr(), n, hw, None, 0, lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and same(outs[0], want[4]) and same(outs[1], want[5])
    one = torch.zeros(n, device=DEV)
    for l1p, msp, o in ((one.data_ptr(), None, outs[0].data_ptr()), (None, one.data_ptr(), outs[0].data_ptr()), (None, None, None)):
        assert hip_lib.odvae_rgba_terms_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, l1p, msp, None, None,
                                            o, None, n, hw, None, 0, lib.stream_ptr()) != 0
    h, w = 15, 20
    nchw = lambda t, c: t.view(n, h, w, c).permute(0, 3, 1, 2)
    out = ops.rgba_terms(nchw(d[0], 4), nchw(d[1], 3), d[2].view(n, 1, h, w), d[3].view(n, 1, h, w), rec_rgba_m=True, gt_rgba_m=True, sums=False)
    assert out[0] is None and out[1] is None and out[2] is None and out[3] is None
    assert same(out[4].permute(0, 2, 3, 1).reshape(n, hw, 4), want[4]) and same(out[5].permute(0, 2, 3, 1).reshape(n, hw, 4), want[5])


def test_rgb_gt_on_a_four_byte_aligned_base(hip_lib):
    """rgb_gt one float into a buffer, odd HW: every pixel's three loads are 4-byte aligned only."""
    n, hw = 2, 7
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=13)
    buf = torch.zeros(n * hw * 3 + 1, dtype=torch.float32, device=DEV)
    buf[1:] = rgb.reshape(-1).float().to(DEV)
    rgb_dev = buf[1:].view(n, hw, 3)
    assert rgb_dev.data_ptr() % 16 == 4
    st, out = call_fwd(hip_lib, dev(rec), rgb_dev, dev(alpha), dev(box), False)
    assert st == 0
    want = R.rgba_terms_f64(rec, rgb, alpha, box, False)
    assert same(out["l1_sum"], want[0]) and same(out["gt_rgb_m"], want[3]) and same(out["gt_rgba_m"], want[5])
    grads = exact_grads(n, hw, seed=14)
    got = call_bwd(hip_lib, dev(rec), rgb_dev, dev(alpha), dev(box), False, *[dev(x) for x in grads])
    assert same(got, R.rgba_terms_bwd_f64(rec, rgb, alpha, box, False, *grads))
    # a reconstruction that is not 16-byte aligned is refused by the library (ops.rgba_terms copies it first: below)
    rbuf = torch.zeros(n * hw * 4 + 1, dtype=torch.float32, device=DEV)
    st, _ = call_fwd(hip_lib, rbuf[1:].view(n, hw, 4), rgb_dev, dev(alpha), dev(box), False)
    assert st != 0


def test_a_workspace_one_byte_short_is_refused_before_launch(hip_lib):
    n, hw = 3, 64
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=15)
    st, out = call_fwd(hip_lib, *[dev(t) for t in (rec, rgb, alpha, box)], False, ws_short=1, fill=-77.0)
    assert st != 0
    for k, t in out.items():
        assert bool((t == -77.0).all()), k      # nothing was written


def test_a_nan_in_one_alpha_reaches_its_own_mask_sum_only(hip_lib):
    n, hw = 3, 300
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=16, with_box=False)
    rec[1, 123, 3] = float("nan")
    for l2 in (False, True):
        st, out = call_fwd(hip_lib, dev(rec), dev(rgb), dev(alpha), None, l2)
        assert st == 0
        ms, l1 = out["mask_sum"].cpu(), out["l1_sum"].cpu()
        assert torch.isnan(ms).tolist() == [False, True, False] and bool(torch.isfinite(l1).all())
        clean = R.rgba_terms_f64(torch.nan_to_num(rec), rgb, alpha, None, l2)
        assert same(out["l1_sum"], clean[0]) and torch.equal(ms[[0, 2]].double(), clean[1][[0, 2]])


@pytest.mark.parametrize("n,hw", [(3, 257), (1, 4100), (2, GRID_CAP_BLOCKS * 256 * 2 + 5)])
def test_random_inputs_within_the_rounding_bound(hip_lib, n, hw):
    g = torch.Generator().manual_seed(hw)
    rec, rgb = torch.randn(n, hw, 4, generator=g), torch.rand(n, hw, 3, generator=g) * 2 - 1
    alpha = (torch.rand(n, hw, generator=g) < 0.5).float()
    box = torch.rand(n, hw, generator=g)          # a soft box: the products round
    d = [dev(t) for t in (rec, rgb, alpha, box)]
    R64 = [t.double() for t in (rec, rgb, alpha, box)]
    blocks = min((hw + 255) // 256, GRID_CAP_BLOCKS)
    K = -(-hw // (256 * blocks))
    w = R64[3][..., None]
    A = ((R64[1] * w).abs() + (R64[0][..., :3] * w).abs()).sum(dim=(1, 2))
    am, ra = R64[2] * R64[3], R64[0][..., 3] * R64[3]
    worst = {}
    for l2 in (False, True):
        want = R.rgba_terms_f64(*R64, l2)
        st, out = call_fwd(hip_lib, *d, l2)
        assert st == 0
        e1 = (out["l1_sum"].double().cpu() - want[0]).abs()
        b1 = U * (A + (K + 12) * want[0]) * (1 + 2.0 ** -10)
        if l2:
            D = ((am - ra).abs() * (am.abs() + ra.abs())).sum(dim=1)
            b2 = U * (2 * D + (K + 14) * want[1]) * (1 + 2.0 ** -10)
        else:
            b2 = U * ((am.abs() + ra.abs()).sum(dim=1) + (K + 12) * want[1]) * (1 + 2.0 ** -10)
        e2 = (out["mask_sum"].double().cpu() - want[1]).abs()
        worst["l1"] = float((e1 / b1).max())
        worst["mask_l2" if l2 else "mask_l1"] = float((e2 / b2).max())
        print("rgba_terms n=%d hw=%d l2=%d: error / bound  l1 %.3f  mask %.3f" % (n, hw, l2, float((e1 / b1).max()), float((e2 / b2).max())))
        assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), worst
        for k, i in (("rec_rgb_m", 2), ("gt_rgb_m", 3), ("rec_rgba_m", 4), ("gt_rgba_m", 5)):
            assert torch.equal(out[k].cpu(), want[i].float()), k      # one correctly rounded product each
        g_l1, g_mask = torch.randn(n, generator=g), torch.randn(n, generator=g)
        g_rgb, g_rgba = torch.randn(n, hw, 3, generator=g), torch.randn(n, hw, 4, generator=g)
        got = call_bwd(hip_lib, *d, l2, dev(g_l1), dev(g_mask), dev(g_rgb), dev(g_rgba)).double().cpu()
        # the signs and the 2 * d of the float64 answer are taken from the f32 differences the kernel forms: a difference that rounds across
        # zero is a tie of the L1 term, not an error of the gradient
        G = [t.double() for t in (g_l1, g_mask, g_rgb, g_rgba)]
        wf = box[..., None]
        sg = torch.sign(rec[..., :3] * wf - rgb * wf).double()
        df = (rec[..., 3:] * wf - alpha[..., None] * wf).double()
        e = 2.0 * df if l2 else torch.sign(df)
        t1 = torch.cat((G[0][:, None, None] * sg * w, G[1][:, None, None] * e * w), dim=-1)
        t2 = torch.cat((G[2] * w, torch.zeros(n, hw, 1, dtype=torch.float64)), dim=-1)
        t3 = G[3] * w
        T = t1.abs() + t2.abs() + t3.abs()
        err = (got - (t1 + t2 + t3)).abs()
        print("rgba_terms_bwd n=%d hw=%d l2=%d: worst error / bound %.3f" % (n, hw, l2, float((err / (4 * U * T + 1e-300)).max())))
        assert bool((err <= 4 * U * T).all())


def test_ops_rgba_terms_autograd(hip_lib):
    """ops.rgba_terms: the outputs a caller did not ask for are not produced, the target-side outputs carry no graph, and one backward
    through all four differentiable outputs is the backward kernel's answer -- on exact inputs, bit for bit.  rgb_gt sits on a 4-byte
    aligned base and the reconstruction on a misaligned one (the op layer copies that one; the result does not change)."""
    from odvae_amd import ops
    n, h, w = 2, 7, 9
    hw = h * w
    rec, rgb, alpha, box = R.exact_rgba_inputs(n, hw, seed=21)
    nchw = lambda t, c: t.view(n, h, w, c).permute(0, 3, 1, 2)
    gbuf = torch.zeros(n * hw * 3 + 1, dtype=torch.float32, device=DEV)
    gbuf[1:] = rgb.reshape(-1).float().to(DEV)
    rgb_t = nchw(gbuf[1:], 3)
    rbuf = torch.zeros(n * hw * 4 + 1, dtype=torch.float32, device=DEV)
    rbuf[1:] = rec.reshape(-1).float().to(DEV)
    assert rgb_t.data_ptr() % 16 == 4 and rbuf[1:].data_ptr() % 16 == 4
    alpha_t, box_t = dev(alpha).view(n, 1, h, w), dev(box).view(n, 1, h, w)
    g_l1, g_mask, g_rgb, g_rgba = exact_grads(n, hw, seed=22)
    for rec_t in (nchw(dev(rec), 4), nchw(rbuf[1:], 4)):
        for l2 in (False, True):
            leaf = rec_t.detach().requires_grad_(True)
            out = ops.rgba_terms(leaf, rgb_t, alpha_t.bool() if l2 else alpha_t, box_t, l2=l2, rec_rgb_m=True, gt_rgb_m=True, rec_rgba_m=True,
                                 gt_rgba_m=True)
            want = R.rgba_terms_f64(rec, rgb, alpha, box, l2)
            assert same(out[0], want[0]) and same(out[1], want[1])
            for i in (2, 3, 4, 5):
                assert same(out[i].permute(0, 2, 3, 1).reshape(n, hw, -1), want[i]), i
            assert not out[3].requires_grad and not out[5].requires_grad and out[2].requires_grad and out[4].requires_grad
            total = ((out[0] * dev(g_l1)).sum() + (out[1] * dev(g_mask)).sum() + (out[2] * nchw(dev(g_rgb), 3)).sum()
                     + (out[4] * nchw(dev(g_rgba), 4)).sum())
            total.backward()
            got = leaf.grad.permute(0, 2, 3, 1).reshape(n, hw, 4)
            assert same(got, R.rgba_terms_bwd_f64(rec, rgb, alpha, box, l2, g_l1, g_mask, g_rgb, g_rgba)), l2
    leaf = nchw(dev(rec), 4).detach().requires_grad_(True)
    out = ops.rgba_terms(leaf, rgb_t, alpha_t, None, rec_rgba_m=True)
    assert out[2] is None and out[3] is None and out[5] is None and out[4] is not None
    out[1].sum().backward()          # the mask term alone: the other gradients arrive as None and add nothing
    want = R.rgba_terms_bwd_f64(rec, rgb, alpha, None, False, None, torch.ones(n, dtype=torch.float64), None, None)
    assert same(leaf.grad.permute(0, 2, 3, 1).reshape(n, hw, 4), want)
    with pytest.raises(ValueError):
        ops.rgba_terms(nchw(dev(rec), 4)[:, :3], rgb_t, alpha_t, None)
