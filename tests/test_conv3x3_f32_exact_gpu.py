"""The f32 3x3 conv forward and data-gradient kernels (csrc/conv3x3_f32.hip, conv3x3_wino_f32.hip, conv3x3_wino4_f32.hip) through the
C ABI, bit for bit.

Every case of tests/conv_f32_exact_inputs.py runs on operands made of small whole numbers (and, for F(4x4), weights 576 m 2^-10): every
product and every partial sum is exact in f32 in any order (`assert_exactly_summable`, on the very tensors), so each output must EQUAL
the float64 convolution -- torch.equal, no tolerance.  Outputs are allocated with NaN fill and canaries behind them, operands and packs
carry canaries too; a second launch must give the same bits.  The packs come from the library's own pack entry points (sums and halves:
exact on these weights), except F(4x4)'s, whose pack kernel multiplies by rounded 1/6, 1/12, 1/24: those kernels run on the host-made
pack, and the device pack has a test of its own against a forward-error bound.  One random-normal case per kernel kind keeps a silent
drop in precision from passing.  profiles/conv3x3_f32_exact.md has the cases, the figures and the mutations these tests were shown to
catch.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_f32_exact_inputs as C
import exact_inputs as E
import gn_offset_inputs as G
from canary_buffers import DEV, assert_canary, out_buf, padded

pytestmark = pytest.mark.gpu
ERR_ARG = 1                     # ODVAE_ERR_ARG
WINO4_TOL = 5e-5                # tests/test_ops_gpu.py WINO_TOL[True]: F(4x4) against float64, of max|y|
TILE4 = C.WINO_TILE[4]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float()


def nchw(flat, n, h, w, c):
    return flat.cpu().view(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def dev(t):
    """(buffer with canary, device view) of a host tensor, or (None, None)"""
    return padded(t.float().contiguous()) if t is not None else (None, None)


def ptr(view):
    return None if view is None else view.data_ptr()


def mismatch(got, want):
    bad = (got.double() != want).nonzero()
    return "%d of %d elements differ, first at %s: %r vs %r" % (len(bad), want.numel(), bad[0].tolist() if len(bad) else None,
                                                                  got[tuple(bad[0])].item() if len(bad) else None,
                                                                  want[tuple(bad[0])].item() if len(bad) else None)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def exact_case(name):
    if C.case_n(C.CASES[name], cus()) is None:
        pytest.skip("no N makes this layer persistent on a device with %d CUs" % cus())
    c = C.make_exact(name, cus())
    C.assert_exactly_summable(c)
    if c.get("persistent"):
        m = 2 if c["route"] == "wino2" else 4
        plan = C.persistent_plan(m, cus(), c["n"], c["hi"], c["wi"], c["cin"], c["cout"])
        assert plan["persistent"] and plan["uneven"], "the launcher's rule does not make %s persistent with uneven tiles: %r" % (name, plan)
    return c


class Run:
    """Launches of one case.  `launch(call, shapes)`: NaN-filled outputs with canaries, one call, the outputs on the host."""

    def __init__(self, L):
        from odvae_amd import lib
        self.L, self.lib = L, lib
        self.held = []              # every buffer with a canary behind it

    def put(self, t):
        buf, view = dev(t)
        if buf is not None:
            self.held.append(buf)
        return view

    def pack(self, fn, floats, w, cout, cin):
        """(fwd, dgrad) from one of the library's pack entry points: NaN-filled before, so an entry the pack kernel skips shows"""
        wv = self.put(w)
        fb, fwd = out_buf(floats(cin, cout))
        db, dgr = out_buf(floats(cout, cin))
        self.lib.check(fn(wv.data_ptr(), cout, cin, fwd.data_ptr(), dgr.data_ptr(), self.lib.stream_ptr()), fn.__name__)
        torch.cuda.synchronize()
        assert not torch.isnan(fwd).any().item() and not torch.isnan(dgr).any().item(), "the pack kernel left an entry unwritten"
        self.held += [fb, db]
        return fwd, dgr

    def launch(self, call, numels):
        outs = [out_buf(k) for k in numels]
        rc = call(*[v for _, v in outs])
        self.lib.check(rc, "launch")
        torch.cuda.synchronize()
        assert_canary(*[b for b, _ in outs], *self.held)
        return [v.cpu() for _, v in outs]

    def exact(self, what, call, shapes, refs):
        """One launch into fresh outputs: no NaN left, every output equal to its float64 reference (None: not compared here), canaries
        intact; a second launch gives the same bits.  shapes: (n, h, w, c) of every output; one with a reference is an image and comes
        back NCHW, one without (the statistics) comes back flat."""
        numels = [s[0] * s[1] * s[2] * s[3] for s in shapes]
        first = self.launch(call, numels)
        outs = []
        for got, shape, ref in zip(first, shapes, refs):
            assert not torch.isnan(got).any().item(), "%s: an output element was never written" % what
            if ref is not None:
                got = nchw(got, *shape)
                assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
                assert torch.equal(got.double(), ref), "%s: %s" % (what, mismatch(got, ref))
            outs.append(got)
        second = self.launch(call, numels)
        for a, b in zip(first, second):
            assert torch.equal(a, b), "%s: a second launch gave other bits" % what
        return outs


# ------------------------------------------------------------------------------------------------------------------------------
# the direct kernels: odvae_conv3x3_f32
# ------------------------------------------------------------------------------------------------------------------------------
def direct_call(r, mode, x, n, hi, wi, cin, pack, cout, bias, res, ho, wo, act):
    return lambda y: r.L.odvae_conv3x3_f32(mode, x.data_ptr(), n, hi, wi, cin, pack.data_ptr(), cout, ptr(bias), ptr(res), y.data_ptr(), ho, wo,
                                           act, r.lib.stream_ptr())


def direct_packs(r, c):
    L = r.L
    if c["abi"] == 5:
        return r.pack(L.odvae_conv3x3_pack_up_f32, L.odvae_conv3x3_up_pack_floats, c["w"], c["cout"], c["cin"])
    return r.pack(L.odvae_conv3x3_pack_f32, L.odvae_conv3x3_pack_floats, c["w"], c["cout"], c["cin"])


def run_direct_forward(r, c, fwd, epilogues):
    n, cin, cout, hi, wi, mode = c["n"], c["cin"], c["cout"], c["hi"], c["wi"], c["mode"]
    ho, wo = C.out_hw(mode, hi, wi)
    x, b, res = r.put(nhwc(c["x"])), r.put(c["b"]), r.put(nhwc(c["res"]))
    for what, (ub, ur, act) in epilogues.items():
        ref = C.conv_ref(mode, c["x"], c["w"], c["b"] if ub else None, c["res"] if ur else None, relu=bool(act))
        assert (ref != 0).any().item()
        r.exact("%s forward (mode %d, %s)" % (c["name"], c["abi"], what),
                direct_call(r, c["abi"], x, n, hi, wi, cin, fwd, cout, b if ub else None, res if ur else None, ho, wo, act),
                [(n, ho, wo, cout)], [ref])


def run_direct_dgrad(r, c, dgr):
    """the data-gradient call: roles swapped, the data-gradient pack; abi 0 -> mode 0, 1 -> mode 3, 2 -> mode 0 at 2h x 2w, 5 -> mode 6"""
    n, cin, cout, hi, wi, mode = c["n"], c["cin"], c["cout"], c["hi"], c["wi"], c["mode"]
    ho, wo = C.out_hw(mode, hi, wi)
    dy = r.put(nhwc(c["dy"]))
    dmode = {0: 0, 1: 3, 2: 0, 5: 6}[c["abi"]]
    yh, yw = (ho, wo) if c["abi"] == 2 else (hi, wi)
    ref = C.dgrad_full_ref(mode, c["dy"], c["w"], c["x"].shape) if c["abi"] == 2 else C.dgrad_ref(mode, c["dy"], c["w"], c["x"].shape)
    r.exact("%s data gradient (mode %d)" % (c["name"], dmode),
            direct_call(r, dmode, dy, n, ho, wo, cout, dgr, cin, None, None, yh, yw, 0), [(n, yh, yw, cin)], [ref])


FULL_AND_NONE = {"bias + residual + ReLU": (True, True, 1), "no bias, no residual, no activation": (False, False, 0)}


@pytest.mark.parametrize("name", list(C.DIRECT_CASES) + list(C.THIN_IN_CASES))
def test_direct_kernels_equal_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    fwd, dgr = direct_packs(r, c)
    run_direct_forward(r, c, fwd, FULL_AND_NONE)
    run_direct_dgrad(r, c, dgr)


@pytest.mark.parametrize("name", list(C.THIN_OUT_CASES))
def test_thin_output_kernel_equals_float64(hip_lib, name):
    """conv3x3_thin_out_kernel takes neither residual nor activation (with either the launcher uses the generic kernel: the third run)"""
    c = exact_case(name)
    r = Run(hip_lib)
    fwd, dgr = direct_packs(r, c)
    run_direct_forward(r, c, fwd, {"bias": (True, False, 0), "no bias": (False, False, 0), "generic kernel: bias + residual + ReLU": (True, True, 1)})
    run_direct_dgrad(r, c, dgr)


# ------------------------------------------------------------------------------------------------------------------------------
# F(2x2): odvae_conv3x3_wino_f32
# ------------------------------------------------------------------------------------------------------------------------------
def wino_call(r, fn, x, n, h, w, cin, pack, cout, bias, res, act):
    return lambda y: fn(x.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, ptr(bias), ptr(res), y.data_ptr(), act, r.lib.stream_ptr())


def run_wino(r, c, fn, fwd, dgr, epilogues):
    n, cin, cout, h, w = c["n"], c["cin"], c["cout"], c["hi"], c["wi"]
    x, b, res, dy = r.put(nhwc(c["x"])), r.put(c["b"]), r.put(nhwc(c["res"])), r.put(nhwc(c["dy"]))
    for what, (ub, ur, act) in epilogues.items():
        ref = C.conv_ref(0, c["x"], c["w"], c["b"] if ub else None, c["res"] if ur else None, relu=bool(act))
        r.exact("%s forward (%s)" % (c["name"], what), wino_call(r, fn, x, n, h, w, cin, fwd, cout, b if ub else None, res if ur else None, act),
                [(n, h, w, cout)], [ref])
    r.exact("%s data gradient" % c["name"], wino_call(r, fn, dy, n, h, w, cout, dgr, cin, None, None, 0), [(n, h, w, cin)],
            [C.dgrad_ref(0, c["dy"], c["w"], c["x"].shape)])


@pytest.mark.parametrize("name", list(C.WINO2_CASES))
def test_f2x2_kernels_equal_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    L = hip_lib
    fwd, dgr = r.pack(L.odvae_conv3x3_pack_wino_f32, L.odvae_conv3x3_wino_pack_floats, c["w"], c["cout"], c["cin"])
    run_wino(r, c, L.odvae_conv3x3_wino_f32, fwd, dgr, FULL_AND_NONE)


# ------------------------------------------------------------------------------------------------------------------------------
# F(4x4) on the host-made pack
# ------------------------------------------------------------------------------------------------------------------------------
def host_packs(r, c):
    fwd, dgr = C.wino4_pack_f64(c["w"])
    assert torch.equal(fwd.float().double(), fwd) and torch.equal(dgr.float().double(), dgr)
    assert fwd.numel() == r.L.odvae_conv3x3_wino4_pack_floats(c["cin"], c["cout"]) and dgr.numel() == r.L.odvae_conv3x3_wino4_pack_floats(c["cout"], c["cin"])
    return r.put(fwd), r.put(dgr)


BIAS_RES_AND_NONE = {"bias + residual": (True, True, 0), "no bias, no residual": (False, False, 0)}


@pytest.mark.parametrize("name", list(C.WINO4_CASES))
def test_f4x4_kernel_equals_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    fwd, dgr = host_packs(r, c)
    run_wino(r, c, hip_lib.odvae_conv3x3_wino4_f32, fwd, dgr, BIAS_RES_AND_NONE)


def partial_sums_of(y, groups):
    """[n][tiles][groups][2] float64 (sum, sum of squares) of the y a kernel wrote, per 16 x 32 tile and channel group"""
    return C.tile_group_sums(y.double(), groups, TILE4)


@pytest.mark.parametrize("name", list(C.WINO4_STATS_CASES))
def test_f4x4_statistics_epilogue_equals_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    L = hip_lib
    fwd, _ = host_packs(r, c)
    n, cin, cout, h, w, groups = c["n"], c["cin"], c["cout"], c["hi"], c["wi"], c["groups"]
    chunks = L.odvae_conv3x3_wino4_stats_chunks(h, w)
    assert chunks == C.tiles_of(4, 1, h, w)
    x, b, res = r.put(nhwc(c["x"])), r.put(c["b"]), r.put(nhwc(c["res"]))
    for what, (ub, ur) in {"bias + residual": (True, True), "no bias, no residual": (False, False)}.items():
        ref = C.conv_ref(0, c["x"], c["w"], c["b"] if ub else None, c["res"] if ur else None)
        call = lambda y, p: L.odvae_conv3x3_wino4_stats_f32(x.data_ptr(), n, h, w, cin, fwd.data_ptr(), cout, ptr(b if ub else None),
                                                            ptr(res if ur else None), y.data_ptr(), p.data_ptr(), groups, r.lib.stream_ptr())
        y, part = r.exact("%s (%s)" % (name, what), call, [(n, h, w, cout), (n, chunks, groups, 2)], [ref, None])
        part = part.view(n, chunks, groups, 2)
        want = partial_sums_of(y, groups)
        assert torch.equal(part.double(), want), "%s (%s): partials: %s" % (name, what, mismatch(part, want))


@pytest.mark.parametrize("name", list(C.WINO4_UP_CASES))
def test_f4x4_upsample_form_equals_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    L = hip_lib
    fwd, _ = host_packs(r, c)
    n, cin, cout, hi, wi, groups = c["n"], c["cin"], c["cout"], c["hi"], c["wi"], c["groups"]
    h, w = 2 * hi, 2 * wi
    chunks = L.odvae_conv3x3_wino4_stats_chunks(h, w)
    x, b, res = r.put(nhwc(c["x"])), r.put(c["b"]), r.put(nhwc(c["res"]))
    for ub, ur in ((True, True), (False, False)):
        ref = C.conv_ref(2, c["x"], c["w"], c["b"] if ub else None, c["res"] if ur else None)
        args = (x.data_ptr(), n, h, w, cin, fwd.data_ptr(), cout, ptr(b if ub else None), ptr(res if ur else None))
        r.exact("%s without statistics" % name, lambda y: L.odvae_conv3x3_wino4_up_f32(*args, y.data_ptr(), None, 0, r.lib.stream_ptr()),
                [(n, h, w, cout)], [ref])
        y, part = r.exact("%s with statistics" % name,
                          lambda y, p: L.odvae_conv3x3_wino4_up_f32(*args, y.data_ptr(), p.data_ptr(), groups, r.lib.stream_ptr()),
                          [(n, h, w, cout), (n, chunks, groups, 2)], [ref, None])
        want = partial_sums_of(y, groups)
        part = part.view(n, chunks, groups, 2)
        assert torch.equal(part.double(), want), "%s: partials: %s" % (name, mismatch(part, want))


@pytest.mark.parametrize("name", list(C.WINO4_POOL_CASES))
def test_f4x4_pooled_data_gradient_equals_float64(hip_lib, name):
    c = exact_case(name)
    r = Run(hip_lib)
    _, dgr = host_packs(r, c)
    n, cin, cout, hi, wi = c["n"], c["cin"], c["cout"], c["hi"], c["wi"]
    dy = r.put(nhwc(c["dy"]))
    ref = C.dgrad_ref(2, c["dy"], c["w"], c["x"].shape)
    r.exact(name, lambda y: hip_lib.odvae_conv3x3_wino4_pool_f32(dy.data_ptr(), n, 2 * hi, 2 * wi, cout, dgr.data_ptr(), cin, y.data_ptr(),
                                                                 r.lib.stream_ptr()), [(n, hi, wi, cin)], [ref])


def gn_operands(c, seed):
    """a GroupNorm in front of the conv: its input (standard normal, shifted), the f32 statistics it would hand on, gamma, beta"""
    g = torch.Generator().manual_seed(seed)
    n, cin, h, w, groups = c["n"], c["cin"], c["hi"], c["wi"], c["groups"]
    gx = (torch.randn(n, cin, h, w, generator=g) * 1.5 + 0.3).float()
    mean, rstd = G.stats64(gx, groups)
    return gx, mean.float(), rstd.float(), torch.randn(cin, generator=g), torch.randn(cin, generator=g)


def gn_bwd_sums(da, gx, mean, rstd, gamma, beta, groups, dtype):
    """[n][tiles][2][c]: per 16 x 32 tile and channel (sum du xhat, sum du), du = da swish'(xhat gamma + beta), in `dtype` on the host"""
    n, c, h, w = gx.shape
    cpg = c // groups
    mu = mean.to(dtype).repeat_interleave(cpg, 1).view(n, c, 1, 1)
    rs = rstd.to(dtype).repeat_interleave(cpg, 1).view(n, c, 1, 1)
    xh = (gx.to(dtype) - mu) * rs
    u = xh * gamma.to(dtype).view(1, c, 1, 1) + beta.to(dtype).view(1, c, 1, 1)
    sg = torch.sigmoid(u)
    du = da.to(dtype) * (sg * (1 + u * (1 - sg)))
    th, tw = TILE4
    ty, tx = -(-h // th), -(-w // tw)

    def tiles(t):
        return F.pad(t, (0, tx * tw - w, 0, ty * th - h)).reshape(n, c, ty, th, tx, tw).sum((3, 5)).permute(0, 2, 3, 1).reshape(n, ty * tx, c)
    return torch.stack([tiles(du * xh), tiles(du)], 2)


@pytest.mark.parametrize("name", list(C.WINO4_GNBWD_CASES))
def test_f4x4_groupnorm_backward_epilogue(hip_lib, name):
    """da bit for bit; the sums contain swish', so they go under the acceptance rule of gn_offset_inputs against float64, with the same
    sums in torch f32 on the host as the yardstick"""
    c = exact_case(name)
    r = Run(hip_lib)
    L = hip_lib
    _, dgr = host_packs(r, c)
    n, cin, cout, h, w, groups = c["n"], c["cin"], c["cout"], c["hi"], c["wi"], c["groups"]
    chunks = L.odvae_conv3x3_wino4_stats_chunks(h, w)
    gx, mean, rstd, gamma, beta = gn_operands(c, C.case_seed(name))
    dy, gxd, md, rd, gd, bd = r.put(nhwc(c["dy"])), r.put(nhwc(gx)), r.put(mean), r.put(rstd), r.put(gamma), r.put(beta)
    ref = C.dgrad_ref(0, c["dy"], c["w"], c["x"].shape)
    call = lambda y, p: L.odvae_conv3x3_wino4_gnbwd_f32(dy.data_ptr(), n, h, w, cout, dgr.data_ptr(), cin, y.data_ptr(), gxd.data_ptr(), md.data_ptr(),
                                                        rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), groups, p.data_ptr(), r.lib.stream_ptr())
    da, part = r.exact(name, call, [(n, h, w, cin), (n, chunks, 2, cin)], [ref, None])
    q64 = gn_bwd_sums(da, gx, mean, rstd, gamma, beta, groups, torch.float64)
    q32 = gn_bwd_sums(da, gx, mean, rstd, gamma, beta, groups, torch.float32)
    part = part.view(n, chunks, 2, cin)
    G.check([G.figure("sum du * xhat", part[:, :, 0], q64[:, :, 0], q32[:, :, 0], G.FLOOR_DX),
             G.figure("sum du", part[:, :, 1], q64[:, :, 1], q32[:, :, 1], G.FLOOR_DX)], name)


# ------------------------------------------------------------------------------------------------------------------------------
# the device F(4x4) pack: not exact (rounded 1/6, 1/12, 1/24), so held to a forward-error bound
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact-case weights", "standard normal"])
def test_device_f4x4_pack_within_its_forward_error_bound(hip_lib, kind):
    """Padding entries are zero exactly; every other entry lies within k 2^-24 (|G| |g| |G|^T), k = C.W4_PACK_ROUNDINGS (counted at its
    definition) -- and the entries of a weight that is zero are zero."""
    L = hip_lib
    cout, cin = 88, 72
    if kind == "standard normal":
        w = (torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(88)) / (9 * cin) ** 0.5).float().double()
    else:
        w = C.make_exact("w4-20x36-ragged")["w"]
    r = Run(L)
    fwd, dgr = r.pack(L.odvae_conv3x3_pack_wino4_f32, L.odvae_conv3x3_wino4_pack_floats, w, cout, cin)
    worst = 0.0
    for what, got, want, scale, (red, out) in zip(("forward pack", "data-gradient pack"), (fwd, dgr), C.wino4_pack_f64(w), C.wino4_pack_abs_f64(w),
                                                  ((cin, cout), (cout, cin))):
        got = got.cpu().double()
        redP, outP = L.odvae_conv3x3_wino4_reduce_pad(red), L.odvae_conv3x3_wino4_out_pad(out)
        assert got.numel() == 36 * redP * outP == want.numel()
        ci = (4 * torch.arange(redP // 4).view(1, -1, 1, 1) + torch.arange(4).view(1, 1, 1, 4)).expand(36, -1, outP, -1)
        co = torch.arange(outP).view(1, 1, -1, 1).expand(36, redP // 4, -1, 4)
        pad = ((ci >= red) | (co >= out)).reshape(-1)
        assert pad.any().item() and (got[pad] == 0).all().item(), "%s: padding is not zero" % what
        bound = C.W4_PACK_ROUNDINGS * 2.0 ** -24 * scale
        err = (got - want).abs()
        live = scale > 0
        ratio = (err[live] / bound[live]).max().item()
        print("%s, %s: max |device - float64| / bound = %.3f (max error %.3e)" % (kind, what, ratio, err.max().item()))
        assert (err <= bound).all().item(), "%s: %d entries outside the bound, worst ratio %.3f" % (what, int((err > bound).sum()), ratio)
        worst = max(worst, ratio)
    assert worst > 0 or kind != "standard normal"      # (the comparison is live: a random pack is not exact)


# ------------------------------------------------------------------------------------------------------------------------------
# random-normal operands: no silent drop in precision
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PRECISION_CASES)
def test_random_normal_operands_stay_at_f32_precision(hip_lib, name):
    c = C.make_normal(name, cus())
    L = hip_lib
    r = Run(L)
    route, mode = c["route"], c["mode"]
    for k in ("x", "w", "b", "res", "dy"):
        c[k] = c[k].float().double()
    n, cin, cout, hi, wi = c["n"], c["cin"], c["cout"], c["hi"], c["wi"]
    ho, wo = C.out_hw(mode, hi, wi)
    thin_out = route == "thin_out"
    res64 = None if thin_out else c["res"]
    y64 = C.conv_ref(mode, c["x"], c["w"], c["b"], res64)
    dx64 = C.dgrad_ref(mode, c["dy"], c["w"], c["x"].shape)
    x32 = c["x"].float().requires_grad_(True)
    y32 = E.conv_f64(mode, x32, c["w"].float(), c["b"].float())             # torch f32 on the host (the function takes any float type)
    dx32, = torch.autograd.grad(y32, x32, c["dy"].float())
    y32 = y32.detach() + (0.0 if thin_out else c["res"].float())
    x, b, res, dy = r.put(nhwc(c["x"])), r.put(c["b"]), (None if thin_out else r.put(nhwc(c["res"]))), r.put(nhwc(c["dy"]))
    if route in ("direct", "thin_in", "thin_out"):
        fwd, dgr = direct_packs(r, c)
        dmode = {0: 0, 1: 3, 2: 0, 5: 6}[c["abi"]]
        y, = r.launch(direct_call(r, c["abi"], x, n, hi, wi, cin, fwd, cout, b, res, ho, wo, 0), [n * ho * wo * cout])
        if c["abi"] == 2:       # the dense form's data gradient is mode 0 at 2h x 2w: compared before the sum-pool
            dx64 = C.dgrad_full_ref(mode, c["dy"], c["w"], c["x"].shape)
            xu = C.upsample2x(c["x"]).float().requires_grad_(True)
            dx32, = torch.autograd.grad(F.conv2d(xu, c["w"].float(), padding=1), xu, c["dy"].float())
        dh, dw_ = dx64.shape[2:]
        dx, = r.launch(direct_call(r, dmode, dy, n, ho, wo, cout, dgr, cin, None, None, dh, dw_, 0), [n * dh * dw_ * cin])
    else:
        fn, pk, fl = ((L.odvae_conv3x3_wino_f32, L.odvae_conv3x3_pack_wino_f32, L.odvae_conv3x3_wino_pack_floats) if route == "wino2" else
                      (L.odvae_conv3x3_wino4_f32, L.odvae_conv3x3_pack_wino4_f32, L.odvae_conv3x3_wino4_pack_floats))
        fwd, dgr = r.pack(pk, fl, c["w"], cout, cin)
        y, = r.launch(wino_call(r, fn, x, n, hi, wi, cin, fwd, cout, b, res, 0), [n * ho * wo * cout])
        dh, dw_ = hi, wi
        dx, = r.launch(wino_call(r, fn, dy, n, hi, wi, cout, dgr, cin, None, None, 0), [n * hi * wi * cin])
    y, dx = nchw(y, n, ho, wo, cout), nchw(dx, n, dh, dw_, cin)
    figs = [G.figure("y", y, y64, y32, G.FLOOR_FWD), G.figure("dx", dx, dx64, dx32, G.FLOOR_DX)]
    if route == "wino4":        # F(4x4) is inherently ~20x less exact than direct f32: the project's own bound against float64
        for f, q in zip(figs, (y64, dx64)):
            rel = f["err"] / G.maxabs(q)
            print("%s %-4s err %.3e = %.3e of max|q| (bound %.1e); torch f32 %.3e" % (name, f["name"], f["err"], rel, WINO4_TOL, f["err_torch"]))
            assert f["finite"] and rel <= WINO4_TOL, "%s %s: %.3e of max|q|" % (name, f["name"], rel)
    else:
        G.check(figs, name)


# ------------------------------------------------------------------------------------------------------------------------------
# the argument contract: what a launcher refuses, it refuses before it launches anything
# ------------------------------------------------------------------------------------------------------------------------------
def refuse(L, what, call, outs, held):
    L.odvae_conv3x3_wgrad_f32(0, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, None, 0, None)      # leaves another entry point's message
    stale = L.odvae_last_error()
    assert call() == ERR_ARG, what
    msg = L.odvae_last_error()
    assert msg and msg != stale, what + ": no message of its own"
    torch.cuda.synchronize()
    for buf, view in outs:
        assert torch.isnan(view).all().item(), what + ": a refused call wrote an output"
    assert_canary(*[b for b, _ in outs], *held)


def test_argument_contract_direct(hip_lib):
    from odvae_amd import lib
    L, s = hip_lib, lib.stream_ptr()
    c = C.make_normal("m0-wide-ragged")
    r = Run(L)
    n, cin, cout, h, w = c["n"], c["cin"], c["cout"], 12, 20
    x = r.put(torch.zeros(n, 2 * h, 2 * w, cin))            # large enough for every mode below
    fwd, _ = direct_packs(r, c)
    yb = out_buf(n * 4 * h * w * cout)
    y = yb[1]
    X, P, Y = x.data_ptr(), fwd.data_ptr(), y.data_ptr()
    f = L.odvae_conv3x3_f32
    refusals = [
        ("x null", lambda: f(0, None, n, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("pack null", lambda: f(0, X, n, h, w, cin, None, cout, None, None, Y, h, w, 0, s)),
        ("y null", lambda: f(0, X, n, h, w, cin, P, cout, None, None, None, h, w, 0, s)),
        ("mode 4", lambda: f(4, X, n, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("mode 7", lambda: f(7, X, n, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("empty shape", lambda: f(0, X, 0, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("mode 0 with Ho != Hi", lambda: f(0, X, n, h, w, cin, P, cout, None, None, Y, h + 1, w, 0, s)),
        ("mode 1 with odd Hi", lambda: f(1, X, n, h + 1, w, cin, P, cout, None, None, Y, h // 2, w // 2, 0, s)),
        ("mode 1 with Wo != Wi / 2", lambda: f(1, X, n, h, w, cin, P, cout, None, None, Y, h // 2, w // 2 + 1, 0, s)),
        ("mode 2 with Ho != 2 Hi", lambda: f(2, X, n, h, w, cin, P, cout, None, None, Y, 2 * h - 1, 2 * w, 0, s)),
        ("mode 3 with Ho != 2 Hi", lambda: f(3, X, n, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("mode 5 with Wo != 2 Wi", lambda: f(5, X, n, h, w, cin, P, cout, None, None, Y, 2 * h, 2 * w + 1, 0, s)),
        ("mode 6 with Hi != 2 Ho", lambda: f(6, X, n, 2 * h, 2 * w, cin, P, cout, None, None, Y, h + 1, w, 0, s)),
        ("x offset by 4 bytes", lambda: f(0, X + 4, n, h, w, cin, P, cout, None, None, Y, h, w, 0, s)),
        ("pack offset by 4 bytes", lambda: f(0, X, n, h, w, cin, P + 4, cout, None, None, Y, h, w, 0, s)),
    ]
    for what, call in refusals:
        refuse(L, what, call, [yb], r.held)


@pytest.mark.parametrize("f4", [False, True])
def test_argument_contract_winograd(hip_lib, f4):
    from odvae_amd import lib
    L, s = hip_lib, lib.stream_ptr()
    n, cin, cout, h, w = 1, 64, 64, 16, 32
    r = Run(L)
    x = r.put(torch.zeros(n, h + 2, w, cin + 4))             # large enough for every shape named below
    wt = torch.zeros(cout, cin, 3, 3)
    pk, fl, f = ((L.odvae_conv3x3_pack_wino4_f32, L.odvae_conv3x3_wino4_pack_floats, L.odvae_conv3x3_wino4_f32) if f4 else
                 (L.odvae_conv3x3_pack_wino_f32, L.odvae_conv3x3_wino_pack_floats, L.odvae_conv3x3_wino_f32))
    fwd, _ = r.pack(pk, fl, wt, cout, cin)
    yb = out_buf(n * (h + 2) * w * cout)
    X, P, Y = x.data_ptr(), fwd.data_ptr(), yb[1].data_ptr()
    refusals = [
        ("x null", lambda: f(None, n, h, w, cin, P, cout, None, None, Y, 0, s)),
        ("pack null", lambda: f(X, n, h, w, cin, None, cout, None, None, Y, 0, s)),
        ("y null", lambda: f(X, n, h, w, cin, P, cout, None, None, None, 0, s)),
        ("empty shape", lambda: f(X, n, h, w, cin, P, 0, None, None, Y, 0, s)),
        ("H no multiple of the tile", lambda: f(X, n, h + (2 if f4 else 1), w, cin, P, cout, None, None, Y, 0, s)),
        ("W no multiple of the tile", lambda: f(X, n, h, w - (2 if f4 else 1), cin, P, cout, None, None, Y, 0, s)),
        ("Cin no whole chunk", lambda: f(X, n, h, w, cin + (4 if f4 else 2), P, cout, None, None, Y, 0, s)),
        ("x offset by 4 bytes", lambda: f(X + 4, n, h, w, cin, P, cout, None, None, Y, 0, s)),
        ("pack offset by 4 bytes", lambda: f(X, n, h, w, cin, P + 4, cout, None, None, Y, 0, s)),
    ]
    if f4:
        refusals.append(("act = 1 on F(4x4)", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, 1, s)))
    for what, call in refusals:
        refuse(L, what, call, [yb], r.held)


@pytest.mark.parametrize("entry", ["stats", "up", "pool", "gnbwd"])
def test_argument_contract_f4x4_epilogues(hip_lib, entry):
    from odvae_amd import lib
    L, s = hip_lib, lib.stream_ptr()
    n, cin, cout, h, w, groups = 1, 64, 64, 16, 32, 32
    r = Run(L)
    x = r.put(torch.zeros(n, h + 2, w, cin + 4))
    fwd, _ = r.pack(L.odvae_conv3x3_pack_wino4_f32, L.odvae_conv3x3_wino4_pack_floats, torch.zeros(cout, cin, 3, 3), cout, cin)
    gx, mean, rstd, gamma = r.put(torch.zeros(n, h, w, cout)), r.put(torch.zeros(n, groups)), r.put(torch.ones(n, groups)), r.put(torch.ones(cout))
    yb, pb = out_buf(n * (h + 2) * w * cout), out_buf(n * 2 * 2 * cout)
    X, P, Y, Q = x.data_ptr(), fwd.data_ptr(), yb[1].data_ptr(), pb[1].data_ptr()
    GX, M, R, GA = gx.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr()
    if entry == "stats":
        f = L.odvae_conv3x3_wino4_stats_f32
        refusals = [
            ("x null", lambda: f(None, n, h, w, cin, P, cout, None, None, Y, Q, groups, s)),
            ("y null", lambda: f(X, n, h, w, cin, P, cout, None, None, None, Q, groups, s)),
            ("partials null", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, None, groups, s)),
            ("no groups", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 0, s)),
            ("groups that do not divide Cout", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 48, s)),
            ("64 channels per group", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 1, s)),
            ("H no multiple of 4", lambda: f(X, n, h + 2, w, cin, P, cout, None, None, Y, Q, groups, s)),
            ("Cin no multiple of 8", lambda: f(X, n, h, w, cin + 4, P, cout, None, None, Y, Q, groups, s)),
            ("x offset by 4 bytes", lambda: f(X + 4, n, h, w, cin, P, cout, None, None, Y, Q, groups, s)),
        ]
    elif entry == "up":
        f = L.odvae_conv3x3_wino4_up_f32
        refusals = [
            ("x null", lambda: f(None, n, h, w, cin, P, cout, None, None, Y, None, 0, s)),
            ("pack null", lambda: f(X, n, h, w, cin, None, cout, None, None, Y, None, 0, s)),
            ("odd output height", lambda: f(X, n, h + 1, w, cin, P, cout, None, None, Y, None, 0, s)),
            ("output height no multiple of 4", lambda: f(X, n, h + 2, w, cin, P, cout, None, None, Y, None, 0, s)),
            ("partials without groups", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 0, s)),
            ("groups that do not divide Cout", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 48, s)),
            ("64 channels per group", lambda: f(X, n, h, w, cin, P, cout, None, None, Y, Q, 1, s)),
            ("x offset by 4 bytes", lambda: f(X + 4, n, h, w, cin, P, cout, None, None, Y, None, 0, s)),
        ]
    elif entry == "pool":
        f = L.odvae_conv3x3_wino4_pool_f32
        refusals = [
            ("x null", lambda: f(None, n, h, w, cin, P, cout, Y, s)),
            ("pack null", lambda: f(X, n, h, w, cin, None, cout, Y, s)),
            ("y null", lambda: f(X, n, h, w, cin, P, cout, None, s)),
            ("H no multiple of 4", lambda: f(X, n, h + 2, w, cin, P, cout, Y, s)),
            ("Cin no multiple of 8", lambda: f(X, n, h, w, cin + 4, P, cout, Y, s)),
            ("x offset by 4 bytes", lambda: f(X + 4, n, h, w, cin, P, cout, Y, s)),
        ]
    else:
        f = L.odvae_conv3x3_wino4_gnbwd_f32
        refusals = [
            ("x null", lambda: f(None, n, h, w, cin, P, cout, Y, GX, M, R, GA, GA, groups, Q, s)),
            ("y null", lambda: f(X, n, h, w, cin, P, cout, None, GX, M, R, GA, GA, groups, Q, s)),
            ("GroupNorm input null", lambda: f(X, n, h, w, cin, P, cout, Y, None, M, R, GA, GA, groups, Q, s)),
            ("mean null", lambda: f(X, n, h, w, cin, P, cout, Y, GX, None, R, GA, GA, groups, Q, s)),
            ("rstd null", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, None, GA, GA, groups, Q, s)),
            ("gamma null", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, R, None, GA, groups, Q, s)),
            ("beta null", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, R, GA, None, groups, Q, s)),
            ("sums null", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, R, GA, GA, groups, None, s)),
            ("no groups", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, R, GA, GA, 0, Q, s)),
            ("groups that do not divide Cout", lambda: f(X, n, h, w, cin, P, cout, Y, GX, M, R, GA, GA, 48, Q, s)),
            ("W no multiple of 4", lambda: f(X, n, h, w - 2, cin, P, cout, Y, GX, M, R, GA, GA, groups, Q, s)),
            ("x offset by 4 bytes", lambda: f(X + 4, n, h, w, cin, P, cout, Y, GX, M, R, GA, GA, groups, Q, s)),
        ]
    for what, call in refusals:
        refuse(L, what, call, [yb, pb], r.held)


# ------------------------------------------------------------------------------------------------------------------------------
# autograd wiring: ops.conv3x3(...).backward on every route that needs no host-made pack
# ------------------------------------------------------------------------------------------------------------------------------
ROUTE_CASES = {"direct": "m0-wide-ragged", "down": "m1-wide", "up_dense": "m2-wide", "up_parity": "m5-wide", "wino2": "w2-4wave"}


def test_route_cases_cover_every_route_but_the_f4x4_ones():
    from odvae_amd import ops
    assert set(ROUTE_CASES) == set(ops.CONV3X3_ROUTES) - {"wino4", "wino4_up"}


@pytest.mark.parametrize("route", list(ROUTE_CASES))
def test_autograd_routes_equal_float64(hip_lib, monkeypatch, route):
    """y, dx and dres of ops.conv3x3 on an exact case: the flipped data-gradient pack, mode 3 / mode 6 and the upsample2x_bwd step of
    up_dense, as autograd wires them"""
    from odvae_amd import ops
    c = exact_case(ROUTE_CASES[route])
    monkeypatch.setattr(ops, "UPCONV_BY_PARITY", route != "up_dense")
    monkeypatch.setattr(ops, "WINOGRAD", True)
    mode, x, w, b, res, dy = c["mode"], c["x"], c["w"], c["b"], c["res"], c["dy"]
    assert ops._conv3x3_route(mode, c["hi"], c["wi"], c["cin"], c["cout"], False) == route
    xd = x.float().to(DEV).requires_grad_(True)
    rd = res.float().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV)
    y = ops.conv3x3(xd, wd, b.float().to(DEV), rd, mode)
    y.backward(dy.float().to(DEV))
    y64 = C.conv_ref(mode, x, w, b, res)
    dx64 = C.dgrad_ref(mode, dy, w, x.shape)
    for what, got, want in (("y", y.detach(), y64), ("dx", xd.grad, dx64), ("dres", rd.grad, dy)):
        got = got.cpu().contiguous()
        assert torch.equal(got.double(), want), "%s route, %s: %s" % (route, what, mismatch(got, want))
