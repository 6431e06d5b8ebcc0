"""The Winograd-domain weight gradient (csrc/conv3x3_wgrad_wino_f32.hip) bit for bit at the edges of its plan, through the C ABI.

The f32 loop (odvae_conv3x3_wgrad_wino_select(0), both the narrow and the wide variant) on the dense whole-number recipe of
tests/wgrad_wino_exact_inputs.py, on which every partial sum is exact in f32 in any order: dw and db must equal the float64 gradient bit
for bit at one tile per image, at ragged last chunks, chunks that span tile rows and images, one to four chunks per split with and without
a short last split, 1 to 64 slabs in the reduction, the XCD block mapping on, and the wide walk's advance off whole chunks.  The split loop
(selector 1, and the default) on the three sparse recipes of tests/wgrad_wino_math.py at plans of several chunks per split, a short last
split and 8 and 16 splits, and on the dense recipe under the accuracy rule of tests/test_wgrad_wino_split_gpu.py.  Every case first asserts
the plan its shape was chosen for: nsplit read from the workspace bytes, the rest from the mirror of plan() (which
tests/test_wgrad_wino_exact_inputs.py holds to the tables, beside showing that the float64 model of the loop rejects thirteen planted faults).

dw and db are NaN-prefilled with canaries behind them; the workspace has exactly the bytes asked for, NaN in every float, canary bytes behind
it; x and dy sit in the middle of larger NaN-filled buffers, so a read outside the tensors that reaches a product shows.
profiles/wgrad_wino_exact.md has the plans as the library reports them and the kernel mutations these tests were shown to catch.
"""
import pytest
import torch

import wgrad_wino_exact_inputs as E
import wgrad_wino_math as wm
from canary_buffers import DEV, assert_canary, assert_workspace_canary, out_buf, workspace

pytestmark = pytest.mark.gpu


def embedded(t):
    """t NCHW float64 on the host -> (whole buffer, NHWC f32 view of its middle) on the device: NaN on both sides of the tensor, at least
    a pixel row and two pixels of it, the tensor 16-byte aligned"""
    n, c, h, w = t.shape
    margin = (w + 2) * c
    buf = torch.full((2 * margin + t.numel(),), float("nan"), device=DEV)
    view = buf[margin:margin + t.numel()].view(n, h, w, c)
    view.copy_(t.permute(0, 2, 3, 1).float())
    assert view.data_ptr() % 16 == 0
    return buf, view


class Launch:
    """The device side of one case."""

    def __init__(self, L, shape, x, dy):
        self.L, self.shape = L, shape
        n, cin, cout, h, w = shape
        assert L.odvae_conv3x3_wgrad_wino_supported(n, h, w, cin, cout) == 1
        self.need = L.odvae_conv3x3_wgrad_wino_workspace_bytes(n, h, w, cin, cout)
        self.xb, self.x = embedded(x)
        self.dyb, self.dy = embedded(dy)

    def assert_plan(self, row):
        """the plan the tables claim: nsplit from the library, the other columns from the mirror, which must agree with the library"""
        n, cin, cout, h, w = self.shape
        p = E.plan(*self.shape)
        assert self.need == p.workspace_bytes, "workspace %d bytes, the mirror has %d" % (self.need, p.workspace_bytes)
        assert E.nsplit_from_workspace(self.need, cin, cout) == p.nsplit == row[5]
        assert E.table_row(self.shape) == row
        return p

    def run(self, form, bias=True):
        """(dw [cout][cin][3][3], db [cout]) on the host after one launch into fresh outputs and a fresh workspace"""
        from odvae_amd import lib
        n, cin, cout, h, w = self.shape
        dwb, dw = out_buf(cout * cin * 9)
        dbb, db = out_buf(cout)
        ws = workspace(self.need)
        ws[:self.need].view(torch.float32).fill_(float("nan"))
        prev = self.L.odvae_conv3x3_wgrad_wino_select(form)
        try:
            lib.check(self.L.odvae_conv3x3_wgrad_wino_f32(self.x.data_ptr(), self.dy.data_ptr(), n, h, w, cin, cout, dw.data_ptr(),
                                                          db.data_ptr() if bias else None, ws.data_ptr(), self.need, lib.stream_ptr()),
                      "odvae_conv3x3_wgrad_wino_f32")
        finally:
            self.L.odvae_conv3x3_wgrad_wino_select(prev)
        torch.cuda.synchronize()
        assert_canary(dwb, dbb)
        assert_workspace_canary(ws)
        return dw.cpu().view(cout, cin, 3, 3), db.cpu()


def mismatch(got, want):
    bad = (got.double() != want.double()).nonzero()
    if not len(bad):
        return "equal"
    i = tuple(bad[0].tolist())
    return "%d of %d elements differ, first at %s: %r vs %r" % (len(bad), want.numel(), list(i), got[i].item(), want[i].item())


def assert_exact_and_repeatable(run, form, dw64, db64):
    dw, db = run.run(form)
    assert torch.equal(dw, dw64.float()), "dw: " + mismatch(dw, dw64)
    assert torch.equal(db, db64.float()), "db: " + mismatch(db, db64)
    dw2, db2 = run.run(form)                                # a second launch: the same bits
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dw3, db3 = run.run(form, bias=False)                    # dbias = NULL: the same dw, db left alone
    assert torch.equal(dw3, dw), "dw without dbias: " + mismatch(dw3, dw64)
    assert torch.isnan(db3).all().item()
    return dw, db


@pytest.mark.parametrize("shape", list(E.F32_CASES), ids=E.case_id)
def test_f32_loop_gives_the_float64_gradient_bit_for_bit(hip_lib, shape):
    x, dy, dw64, db64, _ = E.dense_case(shape)
    run = Launch(hip_lib, shape, x, dy)
    run.assert_plan(E.F32_CASES[shape])
    assert_exact_and_repeatable(run, 0, dw64, db64)


@pytest.mark.parametrize("recipe", E.RECIPES)
@pytest.mark.parametrize("shape", list(E.SPLIT_CASES), ids=E.case_id)
def test_split_loop_gives_the_float64_gradient_bit_for_bit(hip_lib, shape, recipe):
    x, dy, dw64, db64 = E.sparse_case(recipe, shape)
    run = Launch(hip_lib, shape, x, dy)
    assert run.assert_plan(E.SPLIT_CASES[shape]).split_eligible
    dw, db = assert_exact_and_repeatable(run, 1, dw64, db64)
    dd, bd = run.run(-1)
    assert torch.equal(dd, dw) and torch.equal(bd, db), "the default takes the split loop here"


@pytest.mark.parametrize("shape", list(E.SPLIT_CASES), ids=E.case_id)
def test_split_loop_on_the_dense_recipe_is_within_its_dropped_products(hip_lib, shape):
    """e(split) <= e(f32) + 2^-22 sbar, the rule of tests/test_wgrad_wino_split_gpu.py, where e(f32) is 0: the f32 loop is exact here"""
    x, dy, dw64, db64, sbar = E.dense_case(shape)
    run = Launch(hip_lib, shape, x, dy)
    run.assert_plan(E.SPLIT_CASES[shape])
    d0, b0 = run.run(0)
    d1, b1 = run.run(1)
    e0 = (d0.double() - dw64).abs().max().item()
    e1 = (d1.double() - dw64).abs().max().item()
    print("%s: e(f32) %.3e e(split) %.3e sbar %.3e bound %.3e" % (E.case_id(shape), e0, e1, sbar, e0 + 2.0 ** -22 * sbar))
    assert torch.equal(d0, dw64.float()), "f32 loop, dw: " + mismatch(d0, dw64)
    assert e1 <= e0 + 2.0 ** -22 * sbar
    assert torch.equal(b0, db64.float()) and torch.equal(b1, db64.float()), "dbias is summed from the unsplit dM: whole numbers"
    dd, bd = run.run(-1)
    assert torch.equal(dd, d1) and torch.equal(bd, b1)


@pytest.mark.parametrize("side", ["x", "dy"])
@pytest.mark.parametrize("form,shape", E.NAN_CASES, ids=["form%d-%s" % (f, E.case_id(s)) for f, s in E.NAN_CASES])
def test_a_planted_nan_stays_in_its_channel(hip_lib, form, shape, side):
    n, cin, cout, h, w = shape
    x, dy, _, _, _ = E.dense_case(shape)
    p = E.plan(*shape)
    assert E.nsplit_from_workspace(hip_lib.odvae_conv3x3_wgrad_wino_workspace_bytes(n, h, w, cin, cout), cin, cout) == p.nsplit >= 2
    assert not form or p.split_eligible
    base_dw, base_db = Launch(hip_lib, shape, x, dy).run(form)
    assert torch.isfinite(base_dw).all().item() and torch.isfinite(base_db).all().item()
    ch = (cin if side == "x" else cout) - 91
    inside = torch.zeros(cout, cin, 3, 3, dtype=torch.bool)
    if side == "x":
        inside[:, ch] = True
    else:
        inside[ch] = True
    for img, row, col in E.nan_pixels(shape):
        xs, dys = x.clone(), dy.clone()
        (xs if side == "x" else dys)[img, ch, row, col] = float("nan")
        dw64, db64 = wm.wgrad_f64(xs, dys)
        marked = torch.isnan(dw64)
        assert marked.any().item() and not marked[~inside].any().item()
        dw, db = Launch(hip_lib, shape, xs, dys).run(form)
        where = "NaN in %s at image %d, pixel (%d, %d)" % (side, img, row, col)
        assert torch.equal(dw[~inside], base_dw[~inside]), where + ": it left its slice of dw"
        assert not torch.isfinite(dw[marked]).any().item(), where + ": %d marked taps stayed finite" % torch.isfinite(dw[marked]).sum().item()
        others = torch.arange(cout) != ch if side == "dy" else torch.ones(cout, dtype=torch.bool)
        assert torch.equal(db[others], base_db[others]), where + ": db"
        if side == "dy":
            assert not torch.isfinite(db[ch]).item(), where + ": db[ch] stayed finite"


def test_limits_without_a_launch(hip_lib):
    """the first pixel count at which N H W C 4 reaches 0xFFFFFFF0 is refused, the one below it is planned as the mirror plans it"""
    L = hip_lib
    cases = [((2, 128, 128, 2048, 2048), (1, 128, 128, 2, 4194302)),         # 2^23 pixels x 512 bytes = 2^32; four pixels fewer
             ((1, 384, 128, 2, 1398102), (1, 384, 128, 2, 1398100)),         # 2 796 204 pixels x 1 536 bytes >= 0xFFFFFFF0 > 2 796 200 x 1 536
             ((1, 128, 384, 2, 1398102), (1, 128, 384, 2, 1398100))]
    for over, under in cases:
        for shape, want in ((over, 0), (under, 1)):
            n, cin, cout, h, w = shape
            px, c = n * h * w, max(cin, cout)
            assert (px * c * 4 >= 0xFFFFFFF0) == (want == 0) and ((px - 4) * c * 4 < 0xFFFFFFF0)
            assert L.odvae_conv3x3_wgrad_wino_supported(n, h, w, cin, cout) == want == E.supported(n, h, w, cin, cout), shape
            assert L.odvae_conv3x3_wgrad_wino_workspace_bytes(n, h, w, cin, cout) == E.workspace_bytes(*shape), shape
        assert E.workspace_bytes(*over) == 0 and E.workspace_bytes(*under) > 0
