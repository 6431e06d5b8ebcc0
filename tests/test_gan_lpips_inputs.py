"""The references, the precondition and the input makers of tests/gan_lpips_inputs.py, on the host (no device).

The index-built im2col / col2im / weight-reorder references are held to torch's own F.unfold / F.fold / permute; the exactly summable
recipe is checked on every case the GPU tests run (tests/test_gan_lpips_edges_gpu.py takes its case lists from the same module); the
max-pool makers are checked for the properties their names promise, and `check_pool` must be able to fail.
"""
import pytest
import torch
import torch.nn.functional as F

import gan_lpips_inputs as I

GEOMETRY = [(s, hw) for s in (1, 2) for hw in I.MOVE_HW if I.out4x4(hw[0], s) and I.out4x4(hw[1], s)]


def test_geometry_matches_torch():
    for s in (1, 2):
        for h in range(2, 40):
            assert I.out4x4(h, s) == F.conv2d(torch.zeros(1, 1, h, 2), torch.zeros(1, 1, 4, 4), stride=s, padding=1).shape[2]
        assert I.out4x4(1, s) is None
        with pytest.raises(RuntimeError):
            F.conv2d(torch.zeros(1, 1, 1, 8), torch.zeros(1, 1, 4, 4), stride=s, padding=1)
    assert I.out4x4(8, 3) is None
    assert len(GEOMETRY) == 12 and len(I.MOVE_CASES) == 120        # Hi, Wi >= 2 is all the geometry asks: nothing is left out


def _unfold_as_cols(x_nhwc, stride):
    n, hi, wi, c = x_nhwc.shape
    u = F.unfold(x_nhwc.permute(0, 3, 1, 2), kernel_size=4, padding=1, stride=stride)       # [N, C*16, L], row c*16 + kh*4 + kw
    return u.reshape(n, c, 16, -1).permute(0, 3, 2, 1).reshape(-1, 16 * c)


@pytest.mark.parametrize("c,n", [(1, 1), (3, 3), (4, 1), (130, 3)])
@pytest.mark.parametrize("stride,hw", GEOMETRY, ids=lambda v: str(v))
def test_im2col_is_unfold_and_col2im_is_fold(stride, hw, c, n):
    hi, wi = hw
    x = I.distinct_integers((n, hi, wi, c)).double()
    cols = I.im2col4x4(x, stride)
    ho, wo = I.out4x4(hi, stride), I.out4x4(wi, stride)
    assert tuple(cols.shape) == (n * ho * wo, 16 * c)
    assert torch.equal(cols, _unfold_as_cols(x, stride))
    d = torch.randint(-8, 9, cols.shape, generator=I.gen(stride, hi, wi, c, n)).double()
    dx = I.col2im4x4(d, n, hi, wi, c, stride)
    folded = F.fold(d.reshape(n, ho * wo, 16, c).permute(0, 3, 2, 1).reshape(n, c * 16, ho * wo), (hi, wi), kernel_size=4, padding=1, stride=stride)
    assert torch.equal(dx, folded.permute(0, 2, 3, 1))
    # the adjoint identity <im2col(x), d> == <x, col2im(d)>, exact on integers
    xs = torch.randint(-8, 9, x.shape, generator=I.gen(7, stride, hi, wi, c, n)).double()
    assert (I.im2col4x4(xs, stride) * d).sum().item() == (xs * dx).sum().item()


@pytest.mark.parametrize("cout,cin", I.REORDER_CASES, ids=lambda v: str(v))
def test_weight_reorder_round_trips(cout, cin):
    w = I.distinct_integers((cout, cin, 4, 4))
    wg = I.weight_to_gemm(w)
    assert tuple(wg.shape) == (cout, 16 * cin)
    for co, ci, kh, kw in [(0, 0, 0, 0), (cout - 1, cin - 1, 3, 3), (cout // 2, cin // 2, 1, 2), (cout - 1, 0, 2, 3)]:
        assert wg[co, (kh * 4 + kw) * cin + ci] == w[co, ci, kh, kw]
    assert torch.equal(I.weight_from_gemm(wg, cin), w)
    g = I.distinct_integers((cout, 16 * cin))
    assert torch.equal(I.weight_to_gemm(I.weight_from_gemm(g, cin)), g)


@pytest.mark.parametrize("stride,hw", GEOMETRY, ids=lambda v: str(v))
def test_conv_is_the_gemm_of_the_references(stride, hw):
    """y = im2col(x) . W'^T, dx = col2im(dy . W'), dW' = dy^T . im2col(x): the three products of csrc/gan_f32.hip, exact on the recipe"""
    c = I.make_conv_case(stride, hw, 3, 4, True, 3)
    r = I.conv_references(c)
    n, cin, hi, wi = c["x"].shape
    cols = I.im2col4x4(c["x"].permute(0, 2, 3, 1).contiguous(), stride)
    wg = I.weight_to_gemm(c["w"])
    assert torch.equal((cols @ wg.T + c["b"]).reshape(n, r["y"].shape[2], r["y"].shape[3], -1).permute(0, 3, 1, 2), r["y"])
    dyf = c["dy"].permute(0, 2, 3, 1).reshape(-1, 4)
    assert torch.equal(I.col2im4x4(dyf @ wg, n, hi, wi, cin, stride).permute(0, 3, 1, 2), r["dx"])
    assert torch.equal(I.weight_from_gemm(dyf.T @ cols, cin), r["dw"])


@pytest.mark.parametrize("stride,hw", I.CONV_GEOMETRY, ids=lambda v: str(v))
def test_every_gpu_conv_case_is_exactly_summable(stride, hw):
    worst = 0.0
    for s, g, cin, cout, bias, n in I.CONV_CASES:
        if (s, g) == (stride, hw):
            worst = max(worst, I.assert_exactly_summable4x4(I.make_conv_case(s, g, cin, cout, bias, n))["worst"])
    assert 0 < worst < I.LIMIT


def test_summability_rejects_what_does_not_fit():
    c = I.make_conv_case(2, (9, 7), 3, 4, True, 1)
    bad = dict(c, x=c["x"] * 2.0 ** 20)
    with pytest.raises(AssertionError, match="2\\^24"):
        I.assert_exactly_summable4x4(bad)
    with pytest.raises(AssertionError, match="multiples"):
        I.assert_exactly_summable4x4(dict(c, w=c["w"] + 0.125))
    with pytest.raises(AssertionError, match="f32 numbers"):
        I.assert_exactly_summable4x4(dict(c, dy=c["dy"] + 2.0 ** -40))


# ---- max-pool makers ------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(n, c, h, w) for h, w in I.POOL_HW for c in I.POOL_C for n in I.POOL_N]


@pytest.mark.parametrize("h,w", I.POOL_HW, ids=lambda v: str(v))
def test_pool_makers_keep_their_promises(h, w):
    for c in I.POOL_C:
        for n in I.POOL_N:
            shape = (n, c, h, w)
            x = I.pool_relu_ties(shape)
            win = I.windows(x)
            assert tuple(win.shape) == (n, c, h // 2, w // 2, 4) and torch.equal(I.from_windows(win, h, w, x), x)
            assert (x >= 0).all() and ((win == win.max(-1, keepdim=True).values).sum(-1) > 1).any()
            win = I.windows(I.pool_all_equal(shape))
            assert (win == win[..., :1]).all() and (win.numel() <= 16 or len(win.unique()) > 1)
            assert (I.pool_all_negative(shape) < 0).all()
            for maker, special in ((I.pool_neg_inf, torch.isneginf), (I.pool_nan, torch.isnan)):
                x = maker(shape)
                cnt = special(I.windows(x)).sum(-1)
                assert set(cnt.unique().tolist()) >= {0, 1, 4} and ((cnt == 2) | (cnt == 3)).any(), "kinds of windows: %s" % cnt.unique().tolist()
                assert torch.isfinite(x[~special(x)]).all()
            dy = I.pool_upstream_gradient(shape)
            assert tuple(dy.shape) == (n, c, h // 2, w // 2) and (dy != 0).all() and (dy > 0).any() and (dy < 0).any()


def test_windows_are_row_major():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    win = I.windows(x)
    assert win[1, 2, 1, 2].tolist() == [x[1, 2, 2, 4].item(), x[1, 2, 2, 5].item(), x[1, 2, 3, 4].item(), x[1, 2, 3, 5].item()]


def _standin(x, dy, first_nan=True):
    """ops.maxpool2x2's rule on the host: torch, with dy of a NaN window moved to the window's FIRST NaN"""
    y, dx = I.pool_reference(x, dy)
    if first_nan:
        xw, h, w = I.windows(x), x.shape[2], x.shape[3]
        isn = torch.isnan(xw)
        first = isn & (isn.cumsum(-1) == 1)
        dw = torch.where(torch.isnan(y).unsqueeze(-1), first * dy.unsqueeze(-1), I.windows(dx))
        dx = I.from_windows(dw, h, w, dx)
    return y, dx


@pytest.mark.parametrize("maker", sorted(I.POOL_MAKERS))
@pytest.mark.parametrize("shape", [(1, 4, 2, 2), (3, 4, 5, 7), (1, 64, 9, 9)], ids=lambda v: str(v))
def test_check_pool_accepts_torch_and_the_first_nan_rule(maker, shape):
    x, dy = I.POOL_MAKERS[maker](shape), I.pool_upstream_gradient(shape)
    y_ref, dx_ref = I.pool_reference(x, dy)
    I.check_pool(x, dy, y_ref, dx_ref, y_ref, dx_ref, "torch itself")
    y, dx = _standin(x, dy)
    I.check_pool(x, dy, y, dx, y_ref, dx_ref, "first NaN")


def _must_fail(x, dy, y, dx):
    y_ref, dx_ref = I.pool_reference(x, dy)
    with pytest.raises(AssertionError):
        I.check_pool(x, dy, y, dx, y_ref, dx_ref)


def test_check_pool_rejects_the_faults_it_is_there_for():
    shape = (3, 4, 5, 7)
    dy = I.pool_upstream_gradient(shape)
    # the parent's forward on an odd width: windows read with the row stride 2 * Wo instead of W
    x = I.pool_all_negative(shape)
    y, dx = _standin(x, dy)
    wrong = F.max_pool2d(x.permute(0, 2, 3, 1).reshape(3, -1)[:, :4 * 6 * 4].reshape(3, 4, 6, 4).permute(0, 3, 1, 2).contiguous(), 2, 2)
    _must_fail(x, dy, wrong, dx)
    # the dropped row / column left unwritten (NaN) or non-zero
    for v in (float("nan"), 1.0):
        bad = dx.clone(); bad[:, :, 4, :] = v
        _must_fail(x, dy, y, bad)
        bad = dx.clone(); bad[0, 1, 2, 6] = v
        _must_fail(x, dy, y, bad)
    # fmaxf drops the NaN of a mixed window
    x = I.pool_nan(shape)
    y, dx = _standin(x, dy)
    _must_fail(x, dy, torch.nan_to_num(I.windows(x), nan=-1e30).max(-1).values, dx)
    # a NaN window whose gradient vanishes, goes to two elements, or goes to a number
    nanw = torch.isnan(y)
    dw = I.windows(dx)
    lost = dw.clone(); lost[nanw] = 0.0
    _must_fail(x, dy, y, I.from_windows(lost, 5, 7, dx))
    twice = dw.clone(); twice[nanw] = dy[nanw].unsqueeze(-1).expand(-1, 4).clone()
    _must_fail(x, dy, y, I.from_windows(twice, 5, 7, dx))
    xw = I.windows(x)
    mixed = nanw & ~torch.isnan(xw).all(-1)
    assert mixed.any()
    to_number = dw.clone()
    first_num = ~torch.isnan(xw) & ((~torch.isnan(xw)).cumsum(-1) == 1)
    to_number[mixed] = (first_num * dy.unsqueeze(-1))[mixed]
    _must_fail(x, dy, y, I.from_windows(to_number, 5, 7, dx))
    # the tie rule: the gradient on the LAST maximum instead of the first
    x = I.pool_relu_ties(shape)
    y, dx = _standin(x, dy)
    xw = I.windows(x)
    ismax = xw == xw.max(-1, keepdim=True).values
    last = ismax & (ismax.flip(-1).cumsum(-1).flip(-1) == 1)
    _must_fail(x, dy, y, I.from_windows(last * dy.unsqueeze(-1), 5, 7, dx))
