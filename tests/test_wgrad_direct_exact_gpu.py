"""The direct 3x3 weight-gradient kernels of csrc/conv3x3_wgrad_f32.hip past one pixel tile per block, through the C ABI.

Every case of tests/wgrad_direct_inputs.py (several tiles per block on both LDS-DMA buffers, splits that cross an image boundary, a
short last split, a thin-kernel wave that owns rows of two images, 140 and 816 slabs in the thin reduction; the host test
tests/test_wgrad_direct_inputs.py asserts that the library plans them so) on operands that are small whole numbers: every product and
every partial sum is then exact in f32 in any order, and dw and db must equal the float64 gradient bit for bit.  Outputs are allocated
with NaN fill and canaries behind them, the workspace is exactly the size the library asks for, NaN-filled (a slab element read but
never written would otherwise hide in a rounding) with canary bytes behind it.  One random-normal case per kernel kind keeps a silent
drop to lower precision from passing, under the acceptance rule of tests/gn_offset_inputs.py.  profiles/wgrad_direct_exact.md has the
plans, the figures and the mutations these tests were shown to catch.
"""
import pytest
import torch

import gn_offset_inputs as G
import wgrad_direct_inputs as W
from canary_buffers import DEV, assert_canary, assert_workspace_canary, out_buf, padded, workspace

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_WORKSPACE = 1, 2       # ODVAE_ERR_ARG, ODVAE_ERR_WORKSPACE


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float()


def nan_workspace(nbytes):
    """exactly nbytes of workspace, every float of it NaN, with 64 canary bytes behind it"""
    buf = workspace(nbytes)
    assert nbytes % 4 == 0
    buf[:nbytes].view(torch.float32).fill_(float("nan"))
    return buf


class Launch:
    """The device side of one case: operands with canaries behind them, NaN-filled outputs, a workspace of exactly the asked size."""

    def __init__(self, L, mode, x, dy):
        self.L, self.mode = L, mode
        self.n, self.cin, self.hi, self.wi = x.shape
        self.cout, self.ho, self.wo = dy.shape[1:]
        self.xb, self.x = padded(nhwc(x))
        self.dyb, self.dy = padded(nhwc(dy))
        self.need = L.odvae_conv3x3_wgrad_workspace_bytes(mode, self.n, self.ho, self.wo, self.cin, self.cout)

    def outputs(self):
        self.dwb, self.dw = out_buf(self.cout * self.cin * 9)
        self.dbb, self.db = out_buf(self.cout)
        self.ws = nan_workspace(self.need)

    def raw(self, mode=None, x_off=0, dy_off=0, hi=None, ho=None, bias=True, ws_bytes=None):
        from odvae_amd import lib
        return self.L.odvae_conv3x3_wgrad_f32(
            self.mode if mode is None else mode, self.x.data_ptr() + x_off, self.dy.data_ptr() + dy_off, self.n,
            self.hi if hi is None else hi, self.wi, self.cin, self.ho if ho is None else ho, self.wo, self.cout,
            self.dw.data_ptr(), self.db.data_ptr() if bias else None, self.ws.data_ptr(),
            self.need if ws_bytes is None else ws_bytes, lib.stream_ptr())

    def run(self, bias=True):
        """(dw [cout][cin][3][3], db [cout]) on the host after one launch into fresh outputs and a fresh workspace"""
        from odvae_amd import lib
        self.outputs()
        lib.check(self.raw(bias=bias), "odvae_conv3x3_wgrad_f32")
        torch.cuda.synchronize()
        assert_canary(self.xb, self.dyb, self.dwb, self.dbb)
        assert_workspace_canary(self.ws)
        return self.dw.cpu().view(self.cout, self.cin, 3, 3), self.db.cpu()

    def assert_untouched(self):
        torch.cuda.synchronize()
        assert torch.isnan(self.dw).all().item() and torch.isnan(self.db).all().item(), "a refused call wrote an output"
        assert torch.isnan(self.ws[:self.need].view(torch.float32)).all().item(), "a refused call wrote the workspace"
        assert_canary(self.xb, self.dyb, self.dwb, self.dbb)
        assert_workspace_canary(self.ws)


def mismatch(got, want):
    bad = (got.double() != want).nonzero()
    return "%d of %d elements differ, first at %s: %r vs %r" % (len(bad), want.numel(), bad[0].tolist() if len(bad) else None,
                                                                  got[tuple(bad[0])].item() if len(bad) else None,
                                                                  want[tuple(bad[0])].item() if len(bad) else None)


@pytest.mark.parametrize("name", list(W.CASES))
def test_exact_operands_give_the_float64_gradient_bit_for_bit(hip_lib, name):
    mode, n, cin, cout, hi, wi, _ = W.CASES[name]
    x, dy = W.make_exact(mode, n, cin, cout, hi, wi, W.case_seed(name))
    dw64, db64 = W.wgrad_f64(mode, x, dy)
    run = Launch(hip_lib, mode, x, dy)
    dw, db = run.run()
    assert not torch.isnan(dw).any().item() and not torch.isnan(db).any().item(), "an output element was never written"
    assert torch.equal(dw.double(), dw64), "dw: " + mismatch(dw, dw64)
    assert torch.equal(db.double(), db64), "db: " + mismatch(db, db64)
    dw2, db2 = run.run()                                   # a second launch: same bits
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dw3, db3 = run.run(bias=False)                         # dbias = NULL: the same dw, and nothing else written
    assert torch.equal(dw3, dw), "dw without dbias: " + mismatch(dw3, dw64)
    assert torch.isnan(db3).all().item()


@pytest.mark.parametrize("kind", W.KINDS)
def test_argument_contract(hip_lib, kind):
    """what the launcher refuses, it refuses before it launches anything"""
    mode, n, cin, cout, hi, wi, _ = W.CASES[W.PRECISION_CASES[kind]]
    x, dy = W.make_normal(mode, n, cin, cout, hi, wi, 1)
    run = Launch(hip_lib, mode, x, dy)
    run.outputs()
    refusals = [
        ("one workspace byte short", dict(ws_bytes=run.need - 1), ERR_WORKSPACE),
        ("mode 3", dict(mode=3), ERR_ARG),
        ("mode 1 with odd Hi", dict(mode=1, hi=2 * run.ho + 1, ho=run.ho), ERR_ARG),
        ("mode 5 with Ho != 2 Hi", dict(mode=5, hi=run.ho // 2, ho=2 * (run.ho // 2) + 1), ERR_ARG),
        ("x offset by 4 bytes", dict(x_off=4), ERR_ARG),
        ("dy offset by 4 bytes", dict(dy_off=4), ERR_ARG),
    ]
    for what, kwargs, code in refusals:
        hip_lib.odvae_conv3x3_wgrad_f32(mode, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, None, 0, None)   # leaves another message
        stale = hip_lib.odvae_last_error()
        assert run.raw(**kwargs) == code, what
        msg = hip_lib.odvae_last_error()
        assert msg and msg != stale, what + ": no message of its own"
        run.assert_untouched()


def test_slab_of_two_gib_is_refused(hip_lib):
    """One split's slab is addressed with 32-bit byte offsets: at 2^31 bytes the call is an argument error of its own, one channel tile
    below it is an ordinary call (here: one without workspace).  Neither call can launch anything."""
    from odvae_amd import lib
    cin = 4096
    x = torch.zeros(1, 1, 1, cin, device=DEV)
    dw = torch.full((64,), float("nan"), device=DEV)
    for cout, code in ((8192, ERR_ARG), (8128, ERR_WORKSPACE)):      # parity slab: 16 * CinP * CoutP * 4 = 2^31, and 2^31 - 2^24
        dy = torch.zeros(1, 2, 2, cout, device=DEV)
        assert x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
        hip_lib.odvae_conv3x3_wgrad_f32(5, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, None, 0, None)   # leaves another message
        stale = hip_lib.odvae_last_error()
        assert hip_lib.odvae_conv3x3_wgrad_f32(5, x.data_ptr(), dy.data_ptr(), 1, 1, 1, cin, 2, 2, cout, dw.data_ptr(), None, None, 0,
                                               lib.stream_ptr()) == code, cout
        msg = hip_lib.odvae_last_error()
        assert msg and msg != stale, "Cout %d: no message of its own" % cout
    torch.cuda.synchronize()
    assert torch.isnan(dw).all().item(), "a refused call wrote dw"


@pytest.mark.parametrize("kind", W.KINDS)
def test_random_normal_operands_stay_at_f32_precision(hip_lib, kind):
    from test_ops_gpu import ref_conv
    name = W.PRECISION_CASES[kind]
    mode, n, cin, cout, hi, wi, _ = W.CASES[name]
    x, dy = W.make_normal(mode, n, cin, cout, hi, wi, W.case_seed(name))
    dw64, db64 = W.wgrad_f64(mode, x, dy)
    w = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    ref_conv(2 if mode == 5 else mode, x, w, b).backward(dy)           # torch f32 on the host
    dw, db = Launch(hip_lib, mode, x, dy).run()
    G.check([G.figure("dw", dw, dw64, w.grad, G.FLOOR_DX), G.figure("db", db, db64, b.grad, G.FLOOR_DX)], name)
