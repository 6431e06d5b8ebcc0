"""The f32 implicit-GEMM PatchGAN convolutions (csrc/conv3x3_f32.hip modes 6 - 9 behind odvae_conv4x4_f32, csrc/conv4x4_wgrad_f32.hip)
through the C ABI, bit for bit.

Every case of tests/conv4x4_f32_inputs.py runs on operands made of small whole numbers (gan_lpips_inputs.make_conv_case): every product
and every partial sum is exact in f32 in any order (tests/test_conv4x4_f32_inputs.py asserts it on the tensors), so y, dx, dw and db must
EQUAL the float64 convolution -- torch.equal, no tolerance.  Outputs are allocated with NaN fill and canaries behind them, operands and
packs carry canaries too, the workspace is exactly the size the library asks for, NaN-filled, with canary bytes behind it; a second
launch must give the same bits.  On the parent commit every test here fails: the entry points do not exist."""
import ctypes

import pytest
import torch

import conv4x4_bf16_inputs as M
import conv4x4_f32_inputs as C
import gan_lpips_inputs as G
from canary_buffers import assert_canary, assert_workspace_canary, out_buf, padded, workspace

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_WORKSPACE = 1, 2       # ODVAE_ERR_ARG, ODVAE_ERR_WORKSPACE
NAN = float("nan")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float()


def nchw(flat, n, h, w, c):
    return flat.cpu().view(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def mismatch(got, want):
    bad = (got.double() != want).nonzero()
    return "%d of %d elements differ, first at %s: %r vs %r" % (len(bad), want.numel(), bad[0].tolist() if len(bad) else None,
                                                                  got[tuple(bad[0])].item() if len(bad) else None,
                                                                  want[tuple(bad[0])].item() if len(bad) else None)


def nan_workspace(nbytes):
    buf = workspace(nbytes)
    assert nbytes % 4 == 0
    buf[:nbytes].view(torch.float32).fill_(NAN)
    return buf


class Layer:
    """The device side of one case: operands and packs with canaries behind them; every launch writes into fresh NaN-filled outputs."""

    def __init__(self, L, c):
        from odvae_amd import lib
        self.L, self.lib, self.s = L, lib, lib.stream_ptr()
        self.stride = c["stride"]
        self.n, self.cin, self.hi, self.wi = c["x"].shape
        self.cout, self.ho, self.wo = c["dy"].shape[1:]
        self.held = []
        self.x, self.dy, self.w = self.put(nhwc(c["x"])), self.put(nhwc(c["dy"])), self.put(c["w"].float().contiguous())
        self.b = self.put(c["b"].float()) if c["b"] is not None else None
        fb, self.fwd = out_buf(L.odvae_conv4x4_pack_floats(self.cin, self.cout))
        db, self.dgr = out_buf(L.odvae_conv4x4_pack_floats(self.cout, self.cin))
        self.held += [fb, db]
        lib.check(L.odvae_conv4x4_pack_f32(self.w.data_ptr(), self.cout, self.cin, self.stride, self.fwd.data_ptr(), self.dgr.data_ptr(), self.s),
                  "odvae_conv4x4_pack_f32")
        torch.cuda.synchronize()
        assert not torch.isnan(self.fwd).any().item() and not torch.isnan(self.dgr).any().item(), "the pack kernel left an entry unwritten"
        self.need = L.odvae_conv4x4_wgrad_workspace_bytes(self.stride, self.n, self.ho, self.wo, self.cin, self.cout)

    def put(self, t):
        buf, view = padded(t)
        self.held.append(buf)
        return view

    def forward(self, x=None):
        yb, y = out_buf(self.n * self.ho * self.wo * self.cout)
        self.lib.check(self.L.odvae_conv4x4_f32(self.stride, 0, (self.x if x is None else x).data_ptr(), self.n, self.hi, self.wi, self.cin,
                                                self.fwd.data_ptr(), self.cout, None if self.b is None else self.b.data_ptr(), y.data_ptr(),
                                                self.ho, self.wo, self.s), "odvae_conv4x4_f32 forward")
        torch.cuda.synchronize()
        assert_canary(yb, *self.held)
        return nchw(y, self.n, self.ho, self.wo, self.cout)

    def dgrad(self, dy=None):
        xb, dx = out_buf(self.n * self.hi * self.wi * self.cin)
        self.lib.check(self.L.odvae_conv4x4_f32(self.stride, 1, (self.dy if dy is None else dy).data_ptr(), self.n, self.ho, self.wo, self.cout,
                                                self.dgr.data_ptr(), self.cin, None, dx.data_ptr(), self.hi, self.wi, self.s),
                       "odvae_conv4x4_f32 data gradient")
        torch.cuda.synchronize()
        assert_canary(xb, *self.held)
        return nchw(dx, self.n, self.hi, self.wi, self.cin)

    def wgrad_outputs(self):
        self.dwb, self.dw = out_buf(self.cout * self.cin * 16)
        self.dbb, self.db = out_buf(self.cout)
        self.ws = nan_workspace(self.need)

    def wgrad_raw(self, stride=None, x_off=0, dy_off=0, hi=None, wi=None, ho=None, cin=None, bias=True, ws_bytes=None, x_null=False, dw_null=False):
        return self.L.odvae_conv4x4_wgrad_f32(
            self.stride if stride is None else stride, None if x_null else self.x.data_ptr() + x_off, self.dy.data_ptr() + dy_off, self.n,
            self.hi if hi is None else hi, self.wi if wi is None else wi, self.cin if cin is None else cin, self.ho if ho is None else ho,
            self.wo, self.cout, None if dw_null else self.dw.data_ptr(), self.db.data_ptr() if bias else None, self.ws.data_ptr(),
            self.need if ws_bytes is None else ws_bytes, self.s)

    def wgrad(self, bias=True):
        self.wgrad_outputs()
        self.lib.check(self.wgrad_raw(bias=bias), "odvae_conv4x4_wgrad_f32")
        torch.cuda.synchronize()
        assert_canary(self.dwb, self.dbb, *self.held)
        assert_workspace_canary(self.ws)
        return self.dw.cpu().view(self.cout, self.cin, 4, 4), self.db.cpu()

    def wgrad_untouched(self):
        torch.cuda.synchronize()
        assert torch.isnan(self.dw).all().item() and torch.isnan(self.db).all().item(), "a refused call wrote an output"
        assert torch.isnan(self.ws[:self.need].view(torch.float32)).all().item(), "a refused call wrote the workspace"
        assert_canary(self.dwb, self.dbb, *self.held)
        assert_workspace_canary(self.ws)


def check_exact(L, case):
    c = G.make_conv_case(*case)
    ref = G.conv_references(c)
    r = Layer(L, c)
    for what, run, want in (("y", r.forward, ref["y"]), ("dx", r.dgrad, ref["dx"])):
        got = run()
        assert not torch.isnan(got).any().item(), "%s: an output element was never written" % what
        assert torch.equal(got.double(), want), "%s: %s" % (what, mismatch(got, want))
        assert torch.equal(run(), got), "%s: a second launch gave other bits" % what
    dw, db = r.wgrad(bias=c["b"] is not None)
    assert not torch.isnan(dw).any().item(), "dw: an output element was never written"
    assert torch.equal(dw.double(), ref["dw"]), "dw: " + mismatch(dw, ref["dw"])
    if c["b"] is not None:
        assert torch.equal(db.double(), ref["db"]), "db: " + mismatch(db, ref["db"])
    else:
        assert torch.isnan(db).all().item(), "dbias = NULL: something was written"
    dw2, db2 = r.wgrad(bias=c["b"] is not None)                 # a second launch into a fresh NaN workspace: same bits
    assert torch.equal(dw2, dw) and torch.equal(torch.nan_to_num(db2), torch.nan_to_num(db))
    return r


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_every_output_equals_float64(hip_lib, case):
    check_exact(hip_lib, case)


@pytest.mark.parametrize("stride", [1, 2])
def test_weight_gradient_past_one_tile_per_block(hip_lib, stride):
    case = C.WGRAD_SPLIT_CASES[stride]
    s, (h, w), cin, cout, bias, n = case
    out = (ctypes.c_int * 8)()
    assert hip_lib.odvae_conv4x4_wgrad_plan(s, n, h, w, cin, cout, out) == 0
    plan = dict(zip(C.PLAN_FIELDS, out))
    print(plan)
    assert plan["nsplit"] == 30 and plan["tiles_per_split"] == 3 and plan["ntiles"] == 88      # 29 splits of 3 tiles and one of 1
    assert plan["ci_tiles"] == 2 and plan["co_tiles"] == 3 and plan["stride"] == s
    assert n * G.out4x4(h, s) * G.out4x4(w, s) <= 40000
    r = check_exact(hip_lib, case)
    dw, db = r.wgrad(bias=True)
    dw3, db3 = r.wgrad(bias=False)                                  # dbias = NULL: the same dw, and nothing else written
    assert torch.equal(dw3, dw) and torch.isnan(db3).all().item()


def dgrad_footprint(hi, wi, ho, wo, stride, oy, ox):
    """[hi, wi] bool: the input pixels whose data gradient reads dy pixel (oy, ox) -- those inside that output's 4x4 window"""
    m = torch.zeros(hi, wi, dtype=torch.bool)
    for iy in range(hi):
        for ix in range(wi):
            m[iy, ix] = M.nan_footprint((ho, wo), stride, iy, ix)[oy, ox]
    return m


@pytest.mark.parametrize("stride,hw", [(1, (10, 19)), (2, (17, 33)), (2, (20, 36))])
def test_a_planted_nan_reaches_its_footprint_and_nothing_else(hip_lib, stride, hw):
    cin, cout, n = 8, 5, 2
    c = G.make_conv_case(stride, hw, cin, cout, True, n, seed=9)
    r = Layer(hip_lib, c)
    hi, wi = hw
    ho, wo = r.ho, r.wo
    clean_y, clean_dx = r.forward(), r.dgrad()
    for iy, ix in ((hi // 2, wi // 2), (0, 0), (hi - 1, wi - 1), (0, wi - 1)):
        x = c["x"].clone()
        x[1, 3, iy, ix] = NAN
        y = r.forward(r.put(nhwc(x)))
        want = torch.zeros(n, cout, ho, wo, dtype=torch.bool)
        want[1] = M.nan_footprint((ho, wo), stride, iy, ix)
        assert want.any().item()
        assert torch.equal(torch.isnan(y), want), "x NaN at (%d, %d): %d NaN in y, footprint %d" % (iy, ix, int(torch.isnan(y).sum()), int(want.sum()))
        assert torch.equal(y[~want], clean_y[~want])
    for oy, ox in ((ho // 2, wo // 2), (0, 0), (ho - 1, wo - 1), (ho - 1, 0)):
        dy = c["dy"].clone()
        dy[0, 2, oy, ox] = NAN
        dx = r.dgrad(r.put(nhwc(dy)))
        want = torch.zeros(n, cin, hi, wi, dtype=torch.bool)
        want[0] = dgrad_footprint(hi, wi, ho, wo, stride, oy, ox)
        assert want.any().item()
        assert torch.equal(torch.isnan(dx), want), "dy NaN at (%d, %d): %d NaN in dx, footprint %d" % (oy, ox, int(torch.isnan(dx).sum()), int(want.sum()))
        assert torch.equal(dx[~want], clean_dx[~want])


def refused(L, what, call, code=ERR_ARG):
    L.odvae_conv3x3_wgrad_f32(0, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, None, 0, None)      # leaves another entry point's message
    stale = L.odvae_last_error()
    assert call() == code, what
    msg = L.odvae_last_error()
    assert msg and msg != stale, what + ": no message of its own"


@pytest.mark.parametrize("stride", [1, 2])
def test_argument_contract_of_the_forward_and_data_gradient(hip_lib, stride):
    """what the launcher refuses, it refuses before it launches anything"""
    L = hip_lib
    c = G.make_conv_case(stride, (12, 20), 8, 12, True, 2)
    r = Layer(L, c)
    n, cin, cout, hi, wi, ho, wo, s = r.n, r.cin, r.cout, r.hi, r.wi, r.ho, r.wo, r.s
    yb = out_buf(n * (hi + 2) * (wi + 2) * max(cin, cout))
    X, D, P, Q, B, Y = r.x.data_ptr(), r.dy.data_ptr(), r.fwd.data_ptr(), r.dgr.data_ptr(), r.b.data_ptr(), yb[1].data_ptr()
    f = L.odvae_conv4x4_f32
    big = 23171                      # 23171^2 * 4 bytes >= 2^31 - 16: one channel makes a 2 GiB image
    big_o = (big - 2) // stride + 1
    refusals = [
        ("x null", lambda: f(stride, 0, None, n, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("pack null", lambda: f(stride, 0, X, n, hi, wi, cin, None, cout, B, Y, ho, wo, s)),
        ("y null", lambda: f(stride, 0, X, n, hi, wi, cin, P, cout, B, None, ho, wo, s)),
        ("stride 0", lambda: f(0, 0, X, n, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("stride 3", lambda: f(3, 0, X, n, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("dgrad 2", lambda: f(stride, 2, X, n, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("empty shape", lambda: f(stride, 0, X, 0, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("Ho that does not follow from Hi", lambda: f(stride, 0, X, n, hi, wi, cin, P, cout, B, Y, ho + 1, wo, s)),
        ("Wo that does not follow from Wi", lambda: f(stride, 0, X, n, hi, wi, cin, P, cout, B, Y, ho, wo - 1, s)),
        ("Hi = 1", lambda: f(stride, 0, X, n, 1, wi, cin, P, cout, B, Y, 1, wo, s)),
        ("x offset by 4 bytes", lambda: f(stride, 0, X + 4, n, hi, wi, cin, P, cout, B, Y, ho, wo, s)),
        ("pack offset by 4 bytes", lambda: f(stride, 0, X, n, hi, wi, cin, P + 4, cout, B, Y, ho, wo, s)),
        ("a 2 GiB input image", lambda: f(stride, 0, X, 1, big, big, 1, P, 1, None, Y, big_o, big_o, s)),
        ("data gradient: dy's size does not follow from dx's", lambda: f(stride, 1, D, n, ho, wo, cout, Q, cin, None, Y, hi + 2, wi, s)),
        ("data gradient: the forward's geometry the wrong way round", lambda: f(stride, 1, D, n, hi, wi, cout, Q, cin, None, Y, ho, wo, s)),
        ("data gradient with a bias", lambda: f(stride, 1, D, n, ho, wo, cout, Q, cin, B, Y, hi, wi, s)),
        ("data gradient: dy offset by 4 bytes", lambda: f(stride, 1, D + 4, n, ho, wo, cout, Q, cin, None, Y, hi, wi, s)),
        ("data gradient: a 2 GiB dx image", lambda: f(stride, 1, D, 1, big_o, big_o, 1, Q, 1, None, Y, big, big, s)),
    ]
    for what, call in refusals:
        refused(L, what, call)
        torch.cuda.synchronize()
        assert torch.isnan(yb[1]).all().item(), what + ": a refused call wrote an output"
        assert_canary(yb[0], *r.held)
    pb = out_buf(L.odvae_conv4x4_pack_floats(cin, cout))
    for what, call in (("pack: w null", lambda: L.odvae_conv4x4_pack_f32(None, cout, cin, stride, pb[1].data_ptr(), None, s)),
                       ("pack: stride 3", lambda: L.odvae_conv4x4_pack_f32(r.w.data_ptr(), cout, cin, 3, pb[1].data_ptr(), None, s)),
                       ("pack: no channels", lambda: L.odvae_conv4x4_pack_f32(r.w.data_ptr(), 0, cin, stride, pb[1].data_ptr(), None, s))):
        refused(L, what, call)
        torch.cuda.synchronize()
        assert torch.isnan(pb[1]).all().item(), what + ": a refused call wrote the pack"
        assert_canary(pb[0])


@pytest.mark.parametrize("stride", [1, 2])
def test_argument_contract_of_the_weight_gradient(hip_lib, stride):
    L = hip_lib
    c = G.make_conv_case(stride, (12, 20), 8, 12, True, 2)
    r = Layer(L, c)
    r.wgrad_outputs()
    refusals = [
        ("one workspace byte short", dict(ws_bytes=r.need - 1), ERR_WORKSPACE),
        ("no workspace bytes", dict(ws_bytes=0), ERR_WORKSPACE),
        ("x null", dict(x_null=True), ERR_ARG),
        ("dw null", dict(dw_null=True), ERR_ARG),
        ("stride 3", dict(stride=3), ERR_ARG),
        ("stride 0", dict(stride=0), ERR_ARG),
        ("Ho that does not follow from Hi", dict(ho=r.ho + 1), ERR_ARG),
        ("Hi that does not follow from Ho", dict(hi=r.hi + 2), ERR_ARG),
        ("Hi = 1", dict(hi=1, ho=1), ERR_ARG),
        ("no input channels", dict(cin=0), ERR_ARG),
        ("x offset by 4 bytes", dict(x_off=4), ERR_ARG),
        ("dy offset by 4 bytes", dict(dy_off=4), ERR_ARG),
        ("a 2 GiB input image", dict(cin=2 ** 23), ERR_ARG),        # 12 x 20 pixels of 2^23 channels
    ]
    for what, kwargs, code in refusals:
        refused(L, what, lambda: r.wgrad_raw(**kwargs), code)
        r.wgrad_untouched()
    dw, db = r.wgrad()              # and the same buffers take a sound call afterwards
    ref = G.conv_references(c)
    assert torch.equal(dw.double(), ref["dw"]) and torch.equal(db.double(), ref["db"])
