"""odvae_cat_mask_f32 / odvae_cat_mask_bwd_f32 through the C ABI and through ops.cat_mask: y = cat(x * box, cond) along the channels and
dx = dy[..., :Cx] * box.  Every output element is a copy or ONE f32 product, so on any inputs it is the correctly rounded product -- on
the exact inputs (multiples of 1/8, {0,1} boxes) bit for bit the float64 answer, and on random f32 inputs bit for bit the f32 product."""
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

CHANNELS = [(3, 1), (3, 2), (4, 2), (3, 5), (1, 3)]
ROW_CAP = 8192 * 256      # the most elements one launch's threads cover at N = 1 (grid cap 8192 blocks of 256)


def dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def off16(t, floats=1):
    """a device copy of t whose base pointer is 4 * floats bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + floats, device=DEV)
    buf[floats:] = t.reshape(-1)
    v = buf[floats:].view(t.shape)
    assert v.data_ptr() % 16 == 4 * floats
    return v


def call_fwd(L, x, box, cond, n, hw, cx, cc, y=None):
    from odvae_amd import lib
    whole, view = y if y is not None else CB.out_buf(n * hw * (cx + cc))
    st = L.odvae_cat_mask_f32(ptr(x), ptr(box), ptr(cond), view.data_ptr(), n, hw, cx, cc, lib.stream_ptr())
    torch.cuda.synchronize()
    CB.assert_canary(whole)
    return st, view.view(n, hw, cx + cc)


def call_bwd(L, dy, box, n, hw, cx, cc, dx=None):
    from odvae_amd import lib
    whole, view = dx if dx is not None else CB.out_buf(n * hw * cx)
    st = L.odvae_cat_mask_bwd_f32(ptr(dy), ptr(box), view.data_ptr(), n, hw, cx, cc, lib.stream_ptr())
    torch.cuda.synchronize()
    CB.assert_canary(whole)
    return st, view.view(n, hw, cx)


def check_exact(L, n, hw, cx, cc, with_box, shift=False):
    x, box, cond, dy = R.exact_cat_inputs(n, hw, cx, cc, seed=5 * hw + n + cx + 7 * cc, with_box=with_box)
    place = off16 if shift else (lambda t: t)
    d = [None if t is None else place(dev(t)) for t in (x, box, cond, dy)]
    out = None
    if shift:
        whole = torch.full((n * hw * (cx + cc) + 1 + CB.PAD,), float("nan"), device=DEV)
        whole[-CB.PAD:] = CB.CANARY
        out = (whole, whole[1:1 + n * hw * (cx + cc)])
    st, y = call_fwd(L, d[0], d[1], d[2], n, hw, cx, cc, y=out)
    assert st == 0
    st, dx = call_bwd(L, d[3], d[1], n, hw, cx, cc)
    assert st == 0
    assert R.accept_cat(y, dx, None, x, box, cond, dy), (n, hw, cx, cc, with_box, shift)


@pytest.mark.parametrize("hw", [1, 63, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [1, 3])
def test_exact_inputs_bit_for_bit(hip_lib, n, hw):
    for cx, cc in CHANNELS:
        for with_box in (False, True):
            check_exact(hip_lib, n, hw, cx, cc, with_box)


@pytest.mark.parametrize("cx,cc", CHANNELS)
def test_base_pointers_four_bytes_off_sixteen(hip_lib, cx, cc):
    """every array, y included, one float past a 16-byte boundary: the scalar forms give the same bits (Cx + Cc = 4 leaves its 16-byte store)"""
    for hw in (63, 257):
        check_exact(hip_lib, 3, hw, cx, cc, True, shift=True)


@pytest.mark.parametrize("cx,cc", [(3, 2), (3, 1)])
def test_exact_past_the_grid_cap(hip_lib, cx, cc):
    """N = 1 and more output elements (3 + 2) or pixels (3 + 1: the per-pixel form) than the grid's threads: a thread takes a second one,
    and the last stride is ragged."""
    hw = (ROW_CAP // (cx + cc) if cx + cc != 4 else ROW_CAP) + 259
    check_exact(hip_lib, 1, hw, cx, cc, True)


def test_random_inputs_are_the_f32_products(hip_lib):
    n, hw, cx, cc = 2, 1000, 3, 2
    g = torch.Generator().manual_seed(1)
    x, cond, dy, box = torch.randn(n, hw, cx, generator=g), torch.randn(n, hw, cc, generator=g), torch.randn(n, hw, cx + cc, generator=g), torch.rand(n, hw, generator=g)
    st, y = call_fwd(hip_lib, dev(x), dev(box), dev(cond), n, hw, cx, cc)
    assert st == 0 and torch.equal(y.cpu(), torch.cat((x * box[..., None], cond), dim=-1))
    st, dx = call_bwd(hip_lib, dev(dy), dev(box), n, hw, cx, cc)
    assert st == 0 and torch.equal(dx.cpu(), dy[..., :cx] * box[..., None])
    bad = cond.clone()
    bad[1, 7, 1] = float("nan")      # a NaN in cond is copied to its place and nowhere else
    st, y = call_fwd(hip_lib, dev(x), dev(box), dev(bad), n, hw, cx, cc)
    assert st == 0 and int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[1, 7, cx + 1]))


def test_bad_arguments_are_refused_without_a_write(hip_lib):
    from odvae_amd import lib
    n, hw, cx, cc = 2, 64, 3, 2
    x, box, cond, dy = R.exact_cat_inputs(n, hw, cx, cc, seed=3)
    d = [dev(t) for t in (x, box, cond, dy)]
    for kw in (dict(n=0), dict(hw=0), dict(cx=0), dict(cc=0), dict(cc=-1), dict(n=65536), dict(hw=2 ** 29)):
        a = {"n": n, "hw": hw, "cx": cx, "cc": cc, **kw}
        y = CB.out_buf(n * hw * (cx + cc), -77.0)
        # (the buffers keep their size: only the arguments change)
        st = hip_lib.odvae_cat_mask_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), y[1].data_ptr(), a["n"], a["hw"], a["cx"], a["cc"], lib.stream_ptr())
        torch.cuda.synchronize()
        assert st == 1 and bool((y[1] == -77.0).all()) and len(hip_lib.odvae_last_error()) > 0, kw      # ODVAE_ERR_ARG
        dx = CB.out_buf(n * hw * cx, -77.0)
        st = hip_lib.odvae_cat_mask_bwd_f32(d[3].data_ptr(), d[1].data_ptr(), dx[1].data_ptr(), a["n"], a["hw"], a["cx"], a["cc"], lib.stream_ptr())
        torch.cuda.synchronize()
        assert st != 0 and bool((dx[1] == -77.0).all()), kw
    for args in ((None, d[1], d[2]), (d[0], d[1], None)):
        y = CB.out_buf(n * hw * (cx + cc), -77.0)
        st, _ = call_fwd(hip_lib, *args, n, hw, cx, cc, y=y)
        assert st != 0 and bool((y[1] == -77.0).all())
    dx = CB.out_buf(n * hw * cx, -77.0)
    st, _ = call_bwd(hip_lib, None, d[1], n, hw, cx, cc, dx=dx)
    assert st != 0 and bool((dx[1] == -77.0).all())
    # the outputs themselves are required
    assert hip_lib.odvae_cat_mask_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, n, hw, cx, cc, lib.stream_ptr()) == 1
    assert hip_lib.odvae_cat_mask_bwd_f32(d[3].data_ptr(), d[1].data_ptr(), None, n, hw, cx, cc, lib.stream_ptr()) == 1
    torch.cuda.synchronize()


def test_ops_cat_mask_autograd(hip_lib):
    """ops.cat_mask on NCHW tensors: the gradient reaches x alone and is the backward kernel's answer bit for bit; cond may be bool or
    uint8 and may sit on the host; a cond that requires grad, or has the wrong shape, is refused; cond None is ops.mul_mask."""
    from odvae_amd import ops
    n, h, w = 2, 7, 9
    hw = h * w
    nchw = lambda t, ch: t.view(n, h, w, ch).permute(0, 3, 1, 2)
    for cx, cc in CHANNELS:
        x, box, cond, dy = R.exact_cat_inputs(n, hw, cx, cc, seed=31 + cx + cc)
        for b in (box, None):
            leaf = nchw(dev(x), cx).detach().requires_grad_(True)
            bt = None if b is None else dev(b).view(n, 1, h, w)
            y = ops.cat_mask(leaf, bt, nchw(dev(cond), cc).cpu())
            assert tuple(y.shape) == (n, cx + cc, h, w)
            (y * nchw(dev(dy), cx + cc)).sum().backward()
            got_y = y.detach().permute(0, 2, 3, 1).reshape(n, hw, cx + cc).contiguous()
            got_dx = leaf.grad.permute(0, 2, 3, 1).reshape(n, hw, cx).contiguous()
            assert R.accept_cat(got_y, got_dx, None, x, b, cond, dy), (cx, cc, b is None)
    x, box, cond, dy = R.exact_cat_inputs(n, hw, 3, 2, seed=41)
    xt, bt = nchw(dev(x), 3), dev(box).view(n, 1, h, w)
    ones = (cond > 0).double()
    for cast in (torch.bool, torch.uint8):
        y = ops.cat_mask(xt, bt, nchw(dev(ones), 2).to(cast))
        assert R.same(y.permute(0, 2, 3, 1).reshape(n, hw, 5).contiguous(), R.cat_mask_f64(x, box, ones))
    with pytest.raises(ValueError, match="requires grad"):
        ops.cat_mask(xt, bt, nchw(dev(cond), 2).clone().requires_grad_(True))
    for bad in (nchw(dev(cond), 2)[:1], nchw(dev(cond), 2)[:, :, :5], nchw(dev(cond), 2)[0], nchw(dev(cond), 2)[:, :0]):
        with pytest.raises(ValueError, match="cond must be"):
            ops.cat_mask(xt, bt, bad)
    assert torch.equal(ops.cat_mask(xt, bt, None), ops.mul_mask(xt, bt)) and ops.cat_mask(xt, None, None) is xt
