"""odvae_l1_weighted_sums_f32 / odvae_l1_weighted_bwd_f32 through the C ABI and through ops.l1_weighted_sums.

Exact part: images are multiples of 1/8 in [-1, 1], weights multiples of 1/4 in [-1, 2], boxes {0,1}, chosen so that every partial sum
of the kernel is exact in f32 (tests/loss_weights_ref.sums_are_exact, asserted here on the host for each case); the three sums and every
element of the gradient are then bit for bit the float64 answers, whatever the order of the kernel's additions.

Random part: f32 inputs against float64 under a bound counted in roundings of the kernel's arithmetic (u = 2^-24):
  a masked product is one rounding, so d = xm - rm carries at most u(|xm| + |rm|) from its operands and u|d| of its own.  With
  A = sum over a sample of (|xm| + |rm|) and S = sum |d|, the terms of l1 are off by at most u(A + S).  They are added in f32: C additions
  per pixel, a thread's K = ceil(HW / (256 * blocks)) pixels one after another, six butterfly levels and three additions across the
  block's waves -- at most (K C + 9) additions on any path, each off by at most u times a partial sum <= S -- then one rounding of the f64
  total:  |l1 - exact| <= u (A + (K C + 12) S) (1 + 2^-10)  (the last factor covers the second-order terms).
  A term of wl1 is w * |d|: |w| times the error of |d| plus the product's own rounding, at most u(|w|(|xm| + |rm|) + 2 |w d|); partial
  sums are bounded by SW = sum |w d| (the weights may be negative):  |wl1 - exact| <= u (AW + (K C + 13) SW) (1 + 2^-10), AW = sum
  |w|(|xm| + |rm|).  The terms of w are the inputs themselves:  |w_sum - exact| <= u (K C + 12) sum |w| (1 + 2^-10).
  The gradient is ((g_l1 + g_wl1 * w) * sign) * b: one rounding for the product, one for the sum, none for the sign, one for the box:
  |error| <= 4 u T per element, T = (|g_l1| + |g_wl1 w|) |b|, with the sign taken from the f32 difference the kernel forms."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import canary_buffers as CB  # noqa: E402
import loss_weights_ref as R  # noqa: E402

U = 2.0 ** -24
ERR_ARG, ERR_WORKSPACE = 1, 2      # ODVAE_ERR_ARG, ODVAE_ERR_WORKSPACE of include/odvae_hip.h
CHANNELS = [(1, 1), (3, 3), (3, 4), (4, 4)]


def dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def call_sums(L, x, xr, box, wgt, per_channel, n, hw, c, cr, skip=(), ws_short=0, fill=float("nan")):
    """The forward through the C ABI on device arrays; every output and the workspace carry canaries.  Returns (status, {name: [n] view})."""
    from odvae_amd import lib
    bufs = {k: CB.out_buf(n, fill) for k in ("l1", "wl1", "w") if k not in skip}
    nbytes = L.odvae_l1_weighted_workspace_bytes(n)
    ws = CB.workspace(nbytes)
    p = lambda k: bufs[k][1].data_ptr() if k in bufs else None
    st = L.odvae_l1_weighted_sums_f32(ptr(x), ptr(xr), ptr(box), ptr(wgt), int(per_channel), p("l1"), p("wl1"), p("w"), n, hw, c, cr,
                                      ws.data_ptr(), nbytes - ws_short, lib.stream_ptr())
    torch.cuda.synchronize()
    CB.assert_canary(*[b[0] for b in bufs.values()])
    CB.assert_workspace_canary(ws)
    return st, {k: (bufs[k][1] if k in bufs else None) for k in ("l1", "wl1", "w")}


def call_bwd(L, x, xr, box, wgt, per_channel, g_l1, g_wl1, n, hw, c, cr, out=None):
    from odvae_amd import lib
    whole, view = out if out is not None else CB.out_buf(n * hw * cr)
    st = L.odvae_l1_weighted_bwd_f32(ptr(x), ptr(xr), ptr(box), ptr(wgt), int(per_channel), ptr(g_l1), ptr(g_wl1), view.data_ptr(), n, hw, c, cr,
                                     lib.stream_ptr())
    torch.cuda.synchronize()
    CB.assert_canary(whole)
    return st, (view.view(n, hw, cr) if st == 0 else view)


def check_exact(L, n, hw, c, cr, per_channel, with_box, **grid):
    x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, per_channel, seed=7 * hw + 3 * n + c + cr, with_box=with_box, **grid)
    assert R.sums_are_exact(x, xr, box, wgt, per_channel)
    d = [dev(t) for t in (x, xr, box, wgt)]
    st, out = call_sums(L, *d, per_channel, n, hw, c, cr)
    assert st == 0
    assert R.accept_sums((out["l1"], out["wl1"], out["w"]), x, xr, box, wgt, per_channel), (n, hw, c, cr, per_channel, with_box)
    g_l1, g_wl1 = R.exact_grads(n, seed=hw + 1)
    st, got = call_bwd(L, *d, per_channel, dev(g_l1), dev(g_wl1), n, hw, c, cr)
    assert st == 0 and R.accept_bwd(got, x, xr, box, wgt, per_channel, g_l1, g_wl1), (n, hw, c, cr, per_channel, with_box)


@pytest.mark.parametrize("hw", [1, 63, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [1, 3])
def test_exact_inputs_bit_for_bit(hip_lib, n, hw):
    for c, cr in CHANNELS:
        for per_channel in (False, True):
            for with_box in (False, True):
                check_exact(hip_lib, n, hw, c, cr, per_channel, with_box)


@pytest.mark.parametrize("c,cr,per_channel", [(3, 4, False), (3, 3, True), (4, 4, True), (1, 1, False)])
def test_exact_past_the_grid_cap(hip_lib, c, cr, per_channel):
    """More pixels than blocks * threads at N = 1: a thread walks more than one pixel and the last stride is ragged."""
    check_exact(hip_lib, 1, R.PAST_CAP, c, cr, per_channel, True)


def test_xr_and_dxr_on_a_four_byte_aligned_base(hip_lib):
    """Cr = 4 one float into a buffer: the 16-byte form does not apply, the scalar one gives the same bits."""
    n, hw, c, cr = 2, 257, 3, 4
    x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, False, seed=5)
    buf = torch.zeros(n * hw * cr + 1, device=DEV)
    buf[1:] = dev(xr).reshape(-1)
    xr_dev = buf[1:].view(n, hw, cr)
    assert xr_dev.data_ptr() % 16 == 4
    st, out = call_sums(hip_lib, dev(x), xr_dev, dev(box), dev(wgt), False, n, hw, c, cr)
    assert st == 0 and R.accept_sums((out["l1"], out["wl1"], out["w"]), x, xr, box, wgt, False)
    g_l1, g_wl1 = R.exact_grads(n, seed=6)
    whole = torch.full((n * hw * cr + 1 + CB.PAD,), float("nan"), device=DEV)
    whole[-CB.PAD:] = CB.CANARY
    st, got = call_bwd(hip_lib, dev(x), xr_dev, dev(box), dev(wgt), False, dev(g_l1), dev(g_wl1), n, hw, c, cr, out=(whole, whole[1:1 + n * hw * cr]))
    assert st == 0 and R.accept_bwd(got, x, xr, box, wgt, False, g_l1, g_wl1) and bool(torch.isnan(whole[0]))


def test_each_output_and_gradient_may_be_null(hip_lib):
    n, hw, c, cr = 3, 257, 3, 4
    x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, False, seed=11)
    d = [dev(t) for t in (x, xr, box, wgt)]
    for skip in (("l1",), ("wl1",), ("w",), ("l1", "w"), ("l1", "wl1")):
        st, out = call_sums(hip_lib, *d, False, n, hw, c, cr, skip=skip)
        assert st == 0 and all(out[k] is None for k in skip)
        assert R.accept_sums((out["l1"], out["wl1"], out["w"]), x, xr, box, wgt, False), skip
    # the weight sums alone: no images at all (the pixel term is off), per pixel and per element
    for per_channel in (False, True):
        wq = R.exact_inputs(n, hw, c, cr, per_channel, seed=12)[3]
        st, out = call_sums(hip_lib, None, None, None, dev(wq), per_channel, n, hw, c, cr, skip=("l1", "wl1"))
        assert st == 0 and R.same(out["w"], R.l1_weighted_sums_f64(c, None, None, wq, per_channel)[2])
    g_l1, g_wl1 = R.exact_grads(n, seed=13)
    for a, b in ((g_l1, None), (None, g_wl1)):
        st, got = call_bwd(hip_lib, *d, False, dev(a), dev(b), n, hw, c, cr)
        assert st == 0 and R.accept_bwd(got, x, xr, box, wgt, False, a, b)


def test_bad_arguments_are_refused_without_a_write(hip_lib):
    from odvae_amd import lib
    n, hw, c, cr = 2, 64, 3, 4
    x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, False, seed=15)
    d = [dev(t) for t in (x, xr, box, wgt)]
    untouched = lambda out: all(bool((t == -77.0).all()) for t in out.values() if t is not None)
    st, out = call_sums(hip_lib, *d, False, n, hw, c, cr, ws_short=1, fill=-77.0)      # a workspace one byte short
    assert st == ERR_WORKSPACE and untouched(out) and b"workspace" in hip_lib.odvae_last_error()
    nbytes = hip_lib.odvae_l1_weighted_workspace_bytes(n)      # exactly what N = n asks for: the refusals below are about the arguments
    ws = CB.workspace(nbytes)
    for kw in (dict(n=0), dict(n=-1), dict(hw=0), dict(c=0), dict(c=4, cr=3), dict(n=65536)):
        a = {"n": n, "hw": hw, "c": c, "cr": cr, **kw}      # (the buffers keep their size: only the argument changes)
        outs = [CB.out_buf(n, -77.0) for _ in range(3)]
        st = hip_lib.odvae_l1_weighted_sums_f32(*[t.data_ptr() for t in d], 0, *[o[1].data_ptr() for o in outs], a["n"], a["hw"], a["c"], a["cr"],
                                                ws.data_ptr(), nbytes, lib.stream_ptr())
        torch.cuda.synchronize()
        assert st == ERR_ARG and all(bool((o[0][:n] == -77.0).all()) for o in outs), kw
        assert len(hip_lib.odvae_last_error()) > 0
    st, out = call_sums(hip_lib, *d, False, n, hw, c, cr, skip=("l1", "wl1", "w"))
    assert st == ERR_ARG      # nothing to compute
    st, out = call_sums(hip_lib, d[0], d[1], d[2], None, False, n, hw, c, cr, fill=-77.0)
    assert st == ERR_ARG and untouched(out)      # wgt is required
    st, out = call_sums(hip_lib, None, None, None, d[3], False, n, hw, c, cr, skip=("w",), fill=-77.0)
    assert st == ERR_ARG and untouched(out)      # without the images only w_sum can be asked for
    st, out = call_sums(hip_lib, d[0], None, d[2], d[3], False, n, hw, c, cr, fill=-77.0)
    assert st == ERR_ARG and untouched(out)
    st = hip_lib.odvae_l1_weighted_sums_f32(*[t.data_ptr() for t in d], 0, out["l1"].data_ptr(), None, None, n, hw, c, cr, None, nbytes, lib.stream_ptr())
    assert st == ERR_WORKSPACE and untouched(out)      # no workspace at all
    g = dev(R.exact_grads(n, seed=1)[0])
    for args in ((None, d[1], d[3]), (d[0], None, d[3]), (d[0], d[1], None)):      # x, xr and wgt are required
        whole, view = CB.out_buf(n * hw * cr, -77.0)
        st, _ = call_bwd(hip_lib, args[0], args[1], d[2], args[2], False, g, g, n, hw, c, cr, out=(whole, view))
        assert st == ERR_ARG and bool((view == -77.0).all())
    st = hip_lib.odvae_l1_weighted_bwd_f32(*[t.data_ptr() for t in d], 0, g.data_ptr(), g.data_ptr(), None, n, hw, c, cr, lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == ERR_ARG and b"dxr" in hip_lib.odvae_last_error()      # ... and so is dxr
    whole, view = CB.out_buf(n * hw * cr, -77.0)
    st, _ = call_bwd(hip_lib, *d, False, g, g, n, hw, 4, 3, out=(whole, view))
    assert st == ERR_ARG and bool((view == -77.0).all())


def test_a_nan_in_one_sample_stays_in_that_samples_sums(hip_lib):
    n, hw, c, cr = 3, 300, 3, 4
    x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, False, seed=16, with_box=False)
    bad = xr.clone()
    bad[1, 123, 2] = float("nan")
    st, out = call_sums(hip_lib, dev(x), dev(bad), None, dev(wgt), False, n, hw, c, cr)
    assert st == 0
    assert torch.isnan(out["l1"]).tolist() == [False, True, False] and torch.isnan(out["wl1"]).tolist() == [False, True, False]
    want = R.l1_weighted_sums_f64(x, xr, None, wgt, False)
    assert R.same(out["w"], want[2])
    for k, w in (("l1", want[0]), ("wl1", want[1])):
        assert torch.equal(out[k].cpu()[[0, 2]].double(), w[[0, 2]])
    # a NaN in the channel that is not read changes nothing
    bad = xr.clone()
    bad[1, 5, 3] = float("nan")
    st, out = call_sums(hip_lib, dev(x), dev(bad), None, dev(wgt), False, n, hw, c, cr)
    assert st == 0 and R.accept_sums((out["l1"], out["wl1"], out["w"]), x, xr, None, wgt, False)


@pytest.mark.parametrize("n,hw,c,cr,per_channel", [(3, 257, 3, 4, False), (1, 4100, 3, 3, True), (2, R.GRID_CAP_BLOCKS * 256 * 2 + 5, 3, 4, False),
                                                   (2, 1000, 4, 4, True), (2, 1000, 2, 5, False)])
def test_random_inputs_within_the_rounding_bound(hip_lib, n, hw, c, cr, per_channel):
    g = torch.Generator().manual_seed(hw + c)
    x, xr = torch.rand(n, hw, c, generator=g) * 2 - 1, torch.randn(n, hw, cr, generator=g)
    wgt = torch.randn((n, hw, c) if per_channel else (n, hw), generator=g)
    box = torch.rand(n, hw, generator=g)          # a soft box: the products round
    d = [dev(t) for t in (x, xr, box, wgt)]
    st, out = call_sums(hip_lib, *d, per_channel, n, hw, c, cr)
    assert st == 0
    want = R.l1_weighted_sums_f64(x, xr, box, wgt, per_channel)
    X, XR, B, W = x.double(), xr.double()[..., :c], box.double()[..., None], R._full_weight(wgt.double(), per_channel, c)
    mag = (X * B).abs() + (XR * B).abs()
    dd = (X * B - XR * B).abs()
    A, S = mag.sum(dim=(1, 2)), dd.sum(dim=(1, 2))
    AW, SW, WS = (W.abs() * mag).sum(dim=(1, 2)), (W.abs() * dd).sum(dim=(1, 2)), W.abs().sum(dim=(1, 2))
    blocks = min((hw + 255) // 256, R.GRID_CAP_BLOCKS)
    KC = -(-hw // (256 * blocks)) * c
    f = 1 + 2.0 ** -10
    bounds = {"l1": U * (A + (KC + 12) * S) * f, "wl1": U * (AW + (KC + 13) * SW) * f, "w": U * (KC + 12) * WS * f}
    for k, wv in zip(("l1", "wl1", "w"), want):
        e = (out[k].double().cpu() - wv).abs()
        print("l1_weighted n=%d hw=%d c=%d cr=%d pc=%d: %s error / bound %.3f" % (n, hw, c, cr, per_channel, k, float((e / bounds[k]).max())))
        assert bool((e <= bounds[k]).all()), k
    g_l1, g_wl1 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    st, got = call_bwd(hip_lib, *d, per_channel, dev(g_l1), dev(g_wl1), n, hw, c, cr)
    assert st == 0
    bf = box[..., None]
    sg = torch.sign(xr[..., :c] * bf - x * bf).double()      # the f32 differences the kernel forms: one that rounds across zero is a tie
    t = (g_l1.double()[:, None, None] + g_wl1.double()[:, None, None] * W) * sg * B
    T = (g_l1.double().abs()[:, None, None] + (g_wl1.double()[:, None, None] * W).abs()) * B.abs()
    err = (got.double().cpu()[..., :c] - t).abs()
    print("l1_weighted_bwd: worst error / bound %.3f" % float((err / (4 * U * T + 1e-300)).max()))
    assert bool((err <= 4 * U * T).all()) and float(got[..., c:].abs().max() if cr > c else 0.0) == 0.0


def test_ops_l1_weighted_sums_autograd(hip_lib):
    """ops.l1_weighted_sums on NCHW tensors: a 4-channel reconstruction read in place (no copy: its data pointer is the one the kernel
    gets), per-pixel [N,1,H,W] / [1,1,H,W] and per-element weights, want_l1=False, the weight sums alone, one backward launch whose
    result is the backward kernel's answer bit for bit -- channel 3 of the gradient zero."""
    from odvae_amd import ops
    n, h, w, c, cr = 2, 7, 9, 3, 4
    hw = h * w
    nchw = lambda t, ch: t.view(n, h, w, ch).permute(0, 3, 1, 2)
    for per_channel in (False, True):
        x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, per_channel, seed=21 + per_channel)
        leaf = nchw(dev(xr), cr).detach().requires_grad_(True)
        weights = nchw(dev(wgt), c) if per_channel else dev(wgt).view(n, 1, h, w)
        l1, wl1, ws = ops.l1_weighted_sums(nchw(dev(x), c), leaf, dev(box).view(n, 1, h, w), weights)
        assert R.accept_sums((l1.detach(), wl1.detach(), ws), x, xr, box, wgt, per_channel)
        assert l1.requires_grad and wl1.requires_grad and not ws.requires_grad
        g_l1, g_wl1 = R.exact_grads(n, seed=23)
        ((l1 * dev(g_l1)).sum() + (wl1 * dev(g_wl1)).sum()).backward()
        got = leaf.grad.permute(0, 2, 3, 1).reshape(n, hw, cr).contiguous()
        assert R.accept_bwd(got, x, xr, box, wgt, per_channel, g_l1, g_wl1)
        leaf.grad = None
        none, wl1b, _ = ops.l1_weighted_sums(nchw(dev(x), c), leaf, dev(box).view(n, 1, h, w), weights.cpu(), want_l1=False)      # weights from the host
        assert none is None and torch.equal(wl1b, wl1)
        wl1b.sum().backward()
        assert R.accept_bwd(leaf.grad.permute(0, 2, 3, 1).reshape(n, hw, cr).contiguous(), x, xr, box, wgt, per_channel, None, torch.ones(n, dtype=torch.float64))
        only = ops.l1_weighted_sums(None, None, None, weights, shape=(n, c, h, w))
        assert only[0] is None and only[1] is None and torch.equal(only[2], ws)
    x, xr, box, wgt = R.exact_inputs(1, hw, c, cr, False, seed=25)
    shared = dev(wgt).view(1, 1, h, w)      # one map for the whole batch
    xn, xrn = dev(x).view(1, h, w, c).permute(0, 3, 1, 2).expand(n, -1, -1, -1), dev(xr).view(1, h, w, cr).permute(0, 3, 1, 2).expand(n, -1, -1, -1)
    l1, wl1, ws = ops.l1_weighted_sums(xn, xrn, None, shared)
    want = R.l1_weighted_sums_f64(x, xr, None, wgt, False)
    for got_, want_ in zip((l1, wl1, ws), want):
        assert torch.equal(got_.double().cpu(), want_.expand(n))
    for bad in (0.5, torch.ones(n), torch.ones(n, 1, 1, 1)):
        with pytest.raises(ValueError):
            ops.l1_weighted_sums(xn, xrn, None, bad)
    with pytest.raises(ValueError):
        ops.l1_weighted_sums(xn, xrn, None, torch.ones(n, 1, h + 1, w))
