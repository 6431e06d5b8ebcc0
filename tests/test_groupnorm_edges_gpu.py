"""GroupNorm, f32 and bf16, through the C ABI at the shapes no model width reaches (tests/gn_edge_inputs.py has the tables).

Three kinds of test on every case:
  exact     -- inputs whose statistics and output have a bit-for-bit answer under any summation order: every forward entry point
               (own statistics pass, caller-supplied partial sums at chunk counts on both sides of a wavefront, the apply pass alone,
               the three dropout forms at p = 0, 0.5 and 1) must return exactly it, in a regime where the recentring of
               gn_finalize_kernel must not run and in one where it must run for every group;
  rule      -- random inputs, gamma with c distinct values, beta, swish on and off: forward outputs, saved statistics and every
               backward form (two-kernel, the default that takes the read-once kernel where one block holds an item, caller-supplied
               backward partials, bf16, the dropout forms; each with and without dx_add) against float64 under the unchanged acceptance
               rule of tests/gn_offset_inputs.py; a bf16 output may differ by half a bf16 ulp more, elementwise;
  contract  -- the workspace queries equal what the kernels write (canaries right behind), one byte less is ODVAE_ERR_WORKSPACE,
               refused shapes and misaligned operands are ODVAE_ERR_ARG from every entry point and leave the outputs untouched.
Outputs are pre-filled with NaN and have canaries behind them; the workspace is exactly the queried size with a canary behind it.
"""
import pytest
import torch

import canary_buffers as CB
import gn_edge_inputs as E
import gn_offset_inputs as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
BF_CANARY = 12288.0                    # canary_buffers.CANARY is not a bf16 value
OK, ERR_ARG, ERR_WORKSPACE = 0, 1, 2

ALL = [(dt, case) for dt in ("f32", "bf16") for case in E.CASES[dt]]
ALL_IDS = ["%s-%s" % (dt, E.case_id(case)) for dt, case in ALL]
DROP = [(dt, case) for dt, case in ALL if case[1] % 8 == 0]
DROP_IDS = ["%s-%s" % (dt, E.case_id(case)) for dt, case in DROP]


def out_buf(numel, dt="f32"):
    """numel NaN-filled output elements of the dtype with canary_buffers.PAD canary elements behind them: (whole buffer, view)"""
    if dt == "f32":
        return CB.out_buf(numel)
    buf = torch.full((int(numel) + CB.PAD,), float("nan"), dtype=BF, device=DEV)
    buf[int(numel):] = BF_CANARY
    return buf, buf[:int(numel)]


def assert_canary(*bufs):
    for b in bufs:
        assert (b[-CB.PAD:] == (BF_CANARY if b.dtype == BF else CB.CANARY)).all().item(), "the kernel wrote past the end of an output"


def untouched(*bufs):
    assert_canary(*bufs)
    return all(bool(torch.isnan(b[:-CB.PAD]).all()) for b in bufs)


def dev(t, dt="f32"):
    return t.to(DEV).to(BF if dt == "bf16" else torch.float32).contiguous()


class Gn:
    """The entry points of one (dtype, shape).  Every call allocates NaN-filled outputs with canaries and a workspace of exactly the
    queried size (or `ws_bytes`) with a canary behind it, checks the canaries, and returns (rc, outputs as views)."""

    def __init__(self, L, dt, n, c, g, hw):
        self.L, self.dt, self.n, self.c, self.g, self.hw = L, dt, n, c, g, hw
        self.sfx = "_bf16" if dt == "bf16" else "_f32"
        self.query = (L.odvae_groupnorm_bf16_workspace_bytes if dt == "bf16" else L.odvae_groupnorm_workspace_bytes)(n, hw, c, g)

    def fn(self, entry, drop):
        return getattr(self.L, "odvae_groupnorm_" + entry + ("_drop" if drop else "") + self.sfx)

    def _ws(self, ws_bytes):
        nbytes = self.query if ws_bytes is None else ws_bytes
        return CB.workspace(max(nbytes, 0)), nbytes

    def forward(self, entry, x, gamma, beta, swish, partial=None, stats=None, drop=None, ws_bytes=None, x_ptr=None, y_off=0):
        """entry: "fwd" | "fwd_partials" | "apply" -> (rc, y [n, hw, c], mean [n, g], rstd [n, g]); stats = (mean, rstd) for "apply";
        drop = (p, seed); x_ptr / y_off (bytes): misaligned operands for the contract tests"""
        from odvae_amd import lib
        n, c, g, hw = self.n, self.c, self.g, self.hw
        esz = 2 if self.dt == "bf16" else 4
        yb, y = out_buf(n * hw * c + y_off // esz, self.dt)
        mb, mean = out_buf(n * g)
        rb, rstd = out_buf(n * g)
        head = (x.data_ptr() if x_ptr is None else x_ptr, n, hw, c, g, gamma.data_ptr(), beta.data_ptr())
        dr = () if drop is None else (float(drop[0]), int(drop[1]))
        ws = None
        if entry == "fwd":
            ws, nbytes = self._ws(ws_bytes)
            rc = self.fn(entry, drop)(*head, E.EPS, int(swish), *dr, y.data_ptr() + y_off, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nbytes, lib.stream_ptr())
        elif entry == "fwd_partials":
            rc = self.fn(entry, drop)(*head, E.EPS, int(swish), *dr, y.data_ptr() + y_off, mean.data_ptr(), rstd.data_ptr(), partial.data_ptr(),
                                      int(partial.shape[1]), lib.stream_ptr())
        else:
            rc = self.fn(entry, drop)(*head, stats[0].data_ptr(), stats[1].data_ptr(), int(swish), *dr, y.data_ptr() + y_off, lib.stream_ptr())
        torch.cuda.synchronize()
        assert_canary(yb, mb, rb)
        if ws is not None:
            CB.assert_workspace_canary(ws)
        self.last = (yb, mb, rb)
        return rc, y[y_off // esz:].view(n, hw, c), mean.view(n, g), rstd.view(n, g)

    def backward(self, entry, x, dy, gamma, beta, stats, swish, dx_add=None, partial=None, drop=None, ws_bytes=None, ptrs=None, dx_off=0):
        """entry: "bwd" | "bwd_partials" -> (rc, dx [n, hw, c], dgamma [c], dbeta [c]); ptrs: {"x" | "dy": address} overrides"""
        from odvae_amd import lib
        n, c, g, hw = self.n, self.c, self.g, self.hw
        esz = 2 if self.dt == "bf16" else 4
        xb, dx = out_buf(n * hw * c + dx_off // esz, self.dt)
        gb, dg = out_buf(c)
        bb, db = out_buf(c)
        ptrs = ptrs or {}
        head = (ptrs.get("x", x.data_ptr()), ptrs.get("dy", dy.data_ptr()), n, hw, c, g, gamma.data_ptr(), beta.data_ptr(), stats[0].data_ptr(),
                stats[1].data_ptr(), int(swish))
        dr = () if drop is None else (float(drop[0]), int(drop[1]))
        outs = (dx.data_ptr() + dx_off, dg.data_ptr(), db.data_ptr(), lib.ptr(dx_add))
        ws, nbytes = self._ws(ws_bytes)
        if entry == "bwd":
            rc = self.fn(entry, drop)(*head, *dr, *outs, ws.data_ptr(), nbytes, lib.stream_ptr())
        else:
            rc = self.fn(entry, None)(*head, *outs, partial.data_ptr(), int(partial.shape[1]), ws.data_ptr(), nbytes, lib.stream_ptr())
        torch.cuda.synchronize()
        assert_canary(xb, gb, bb)
        CB.assert_workspace_canary(ws)
        self.last = (xb, gb, bb)
        return rc, dx[dx_off // esz:].view(n, hw, c), dg, db


def ok(res, what):
    from odvae_amd import lib
    lib.check(res[0], what)
    return res[1:]


# ---- exact ---------------------------------------------------------------------------------------------------------------------------
def _same(what, got, want):
    assert got.dtype == want.dtype and torch.equal(got, want), "%s: %d of %d elements differ from the prediction" % (
        what, int((got != want).sum()), want.numel())


@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_exact_forward(hip_lib, dt, case):
    """fwd, fwd_partials at every chunk count and apply return the predicted y, mean and rstd bit for bit; the recentring ran for no group
    (|m| <= 3 s) or for every group (|m| = 32 s)"""
    L = hip_lib
    n, c, g, hw, _ = case
    gn = Gn(L, dt, n, c, g, hw)
    for regime in E.REGIMES:
        ex = E.exact_case(case, regime)
        tag = "%s %s %s " % (dt, E.case_id(case), regime)
        xd, gd, bd = dev(ex.x, dt), dev(ex.gamma), dev(ex.beta)
        want = (dev(ex.y_bf16 if dt == "bf16" else ex.y, dt), dev(ex.mean), dev(ex.rstd))
        runs = [("fwd", None)] + [("fwd_partials", k) for k in E.FWD_CHUNK_COUNTS]
        for entry, chunks in runs:
            part = dev(E.fwd_partials(ex.x, g, chunks)) if chunks else None
            before = L.odvae_groupnorm_recentred(0)
            got = ok(gn.forward(entry, xd, gd, bd, 0, partial=part), tag + entry)
            ran = L.odvae_groupnorm_recentred(0) - before
            for name, a, b in zip(("y", "mean", "rstd"), got, want):
                _same("%s%s chunks=%s %s" % (tag, entry, chunks, name), a, b)
            assert ran == ex.recentred, "%s%s chunks=%s: %d groups recentred, expected %d" % (tag, entry, chunks, ran, ex.recentred)
        before = L.odvae_groupnorm_recentred(0)
        y = ok(gn.forward("apply", xd, gd, bd, 0, stats=want[1:]), tag + "apply")[0]
        _same(tag + "apply y", y, want[0])
        assert L.odvae_groupnorm_recentred(0) == before


@pytest.mark.parametrize("dt,case", DROP, ids=DROP_IDS)
def test_exact_forward_dropout(hip_lib, dt, case):
    """the three dropout forms at p = 0, 0.5 and 1: the same y times the host mask (scales 1, 2, 0: exact), statistics unaffected by p"""
    L = hip_lib
    n, c, g, hw, _ = case
    gn = Gn(L, dt, n, c, g, hw)
    for regime in E.REGIMES:
        ex = E.exact_case(case, regime)
        tag = "%s %s %s " % (dt, E.case_id(case), regime)
        xd, gd, bd = dev(ex.x, dt), dev(ex.gamma), dev(ex.beta)
        stats = (dev(ex.mean), dev(ex.rstd))
        part = dev(E.fwd_partials(ex.x, g, 3))
        for p in E.DROP_PS:
            want = dev(ex.dropped(p, dt), dt)
            drop = (p, E.DROP_SEED)
            for entry in ("fwd", "fwd_partials", "apply"):
                before = L.odvae_groupnorm_recentred(0)
                y, mean, rstd = ok(gn.forward(entry, xd, gd, bd, 0, partial=part, stats=stats, drop=drop), tag + entry + "_drop")
                _same("%s%s_drop p=%g y" % (tag, entry, p), y, want)
                if entry != "apply":
                    _same("%s%s_drop p=%g mean" % (tag, entry, p), mean, stats[0])
                    _same("%s%s_drop p=%g rstd" % (tag, entry, p), rstd, stats[1])
                    assert L.odvae_groupnorm_recentred(0) - before == ex.recentred


# ---- rule ----------------------------------------------------------------------------------------------------------------------------
def _out_figure(dt, name, got, q64, q32, floor):
    if dt == "bf16":
        return E.bf16_elementwise(name, got, q64, q32, floor)
    return G.figure(name, got, q64, q32, floor)


@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_forward_against_float64(hip_lib, dt, case):
    L = hip_lib
    n, c, g, hw, _ = case
    gn = Gn(L, dt, n, c, g, hw)
    figs = []
    for r in E.RULE_RATIOS:
        rc = E.rule_case(dt, case, r)
        xd, gd, bd = dev(rc.x, dt), dev(rc.gamma), dev(rc.beta)
        stats64 = (dev(rc.mean64.float()), dev(rc.rstd64.float()))
        for swish in (False, True):
            y64, y32, mean32, rstd32 = rc.forward_refs(swish)
            counts = E.FWD_CHUNK_COUNTS if (r, swish) == (4, True) else (3,)
            for entry, chunks in [("fwd", None), ("apply", None)] + [("fwd_partials", k) for k in counts]:
                tag = "r%d swish%d %s%s: " % (r, swish, entry, "" if chunks is None else " chunks=%d" % chunks)
                part = dev(E.fwd_partials(rc.x, g, chunks)) if chunks else None
                y, mean, rstd = ok(gn.forward(entry, xd, gd, bd, swish, partial=part, stats=stats64), tag)
                figs.append(_out_figure(dt, tag + "y", y, y64, y32, G.FLOOR_FWD))
                if entry != "apply":
                    figs += G.stat_figures(mean.cpu(), rstd.cpu(), rc.mean64, rc.rstd64, mean32, rstd32, tag)
    G.check(figs, "%s %s" % (dt, E.case_id(case)))


def _bwd_figures(dt, tag, got, refs, dskip):
    add = 0.0 if dskip is None else dskip.double()
    return [_out_figure(dt, tag + "dx", got[0], refs[64][0] + add, refs[32][0] + (0.0 if dskip is None else dskip), G.FLOOR_DX),
            G.figure(tag + "dgamma", got[1], refs[64][1], refs[32][1], G.FLOOR_PARAM),
            G.figure(tag + "dbeta", got[2], refs[64][2], refs[32][2], G.FLOOR_PARAM)]


@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_backward_against_float64(hip_lib, dt, case):
    """every backward form, with and without dx_add, at r = 0 and 4, swish off and on; the two forms of odvae_groupnorm_bwd_f32 agree"""
    from odvae_amd import dropout_mask as dm
    L = hip_lib
    n, c, g, hw, _ = case
    gn = Gn(L, dt, n, c, g, hw)
    need_partials = 4 * E.workspace_floats(E.shape_of(dt, n, hw, c, g), "bwd_partials")      # what include/odvae_hip.h states
    mask = torch.from_numpy(dm.resnet_dropout_keep_nhwc(E.DROP_SEED, 0.5, n, c, hw, 1)).reshape(n, hw, c) if c % 8 == 0 else None
    figs = []
    prev = L.odvae_groupnorm_select_backward(-1)
    try:
        for combo, (r, swish) in enumerate((r, s) for r in E.RULE_RATIOS for s in (False, True)):
            rc = E.rule_case(dt, case, r)
            xd, dyd, skd, gd, bd = dev(rc.x, dt), dev(rc.dy, dt), dev(rc.dskip, dt), dev(rc.gamma), dev(rc.beta)
            stats = (dev(rc.mean64.float()), dev(rc.rstd64.float()))
            refs = rc.backward_refs(swish)
            for with_add in (False, True):
                add, dskip = (skd, rc.dskip) if with_add else (None, None)
                tag = "r%d swish%d add%d " % (r, swish, with_add)
                forms = {}
                for mode in ((0, -1) if dt == "f32" else (-1,)):
                    L.odvae_groupnorm_select_backward(mode)
                    forms[mode] = ok(gn.backward("bwd", xd, dyd, gd, bd, stats, swish, add), tag + "bwd")
                    figs += _bwd_figures(dt, tag + "bwd(form %d) " % mode, forms[mode], refs, dskip)
                L.odvae_groupnorm_select_backward(-1)
                if dt == "f32":
                    scale = max(1.0, G.maxabs(refs[64][0] + (0.0 if dskip is None else dskip.double())))
                    gap = G.maxerr(forms[0][0], forms[-1][0])
                    assert gap <= G.FLOOR_DX * scale, "%sdx of the two forms differs by %.3e > %.3e" % (tag, gap, G.FLOOR_DX * scale)
                    for k, name in ((1, "dgamma"), (2, "dbeta")):
                        bnd = G.bound(G.maxerr(refs[32][k], refs[64][k]), G.maxabs(refs[64][k]), G.FLOOR_PARAM)
                        assert G.maxerr(forms[0][k], forms[-1][k]) <= bnd, "%s%s of the two forms differs by more than the rule allows" % (tag, name)
                    # caller-supplied backward partials: every chunk count meets dx_add and no dx_add over the four (r, swish)
                    for i, chunks in enumerate(E.BWD_CHUNK_COUNTS):
                        if (i + combo) % 2 != int(with_add):
                            continue
                        part = dev(E.bwd_partials(rc.x, rc.dy, rc.gamma, rc.beta, swish, g, chunks))
                        got = ok(gn.backward("bwd_partials", xd, dyd, gd, bd, stats, swish, add, partial=part, ws_bytes=need_partials), tag + "bwd_partials")
                        figs += _bwd_figures(dt, tag + "bwd_partials chunks=%d " % chunks, got, refs, dskip)
                if mask is not None:
                    got = ok(gn.backward("bwd", xd, dyd, gd, bd, stats, swish, add, drop=(0.5, E.DROP_SEED)), tag + "bwd_drop")
                    figs += _bwd_figures(dt, tag + "bwd_drop p=0.5 ", got, rc.backward_refs(swish, mask), dskip)
    finally:
        L.odvae_groupnorm_select_backward(prev)
    assert L.odvae_groupnorm_fused_timeouts() == 0
    G.check(figs, "%s %s" % (dt, E.case_id(case)))


# ---- contract ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_workspace_queries_are_what_the_kernels_write(hip_lib, dt, case):
    """the query equals the restated need (forward partials, backward partials + chan + grp, the read-once kernel's counters and partials);
    each entry point runs inside exactly its own need with the canary intact and refuses one byte less"""
    L = hip_lib
    n, c, g, hw, _ = case
    s = E.shape_of(dt, n, hw, c, g)
    gn = Gn(L, dt, n, c, g, hw)
    assert gn.query == E.workspace_bytes(dt, s)
    ex = E.exact_case(case, "near")
    xd, gd, bd = dev(ex.x, dt), dev(ex.gamma), dev(ex.beta)
    stats = (dev(ex.mean), dev(ex.rstd))
    drops = (None, (0.5, E.DROP_SEED)) if c % 8 == 0 else (None,)
    fwd_need = 4 * E.workspace_floats(s, "fwd")
    for drop in drops:
        y = ok(gn.forward("fwd", xd, gd, bd, 0, drop=drop, ws_bytes=fwd_need), "fwd in its own need")[0]
        assert not torch.isnan(y.float()).any()
        assert gn.forward("fwd", xd, gd, bd, 0, drop=drop, ws_bytes=fwd_need - 1)[0] == ERR_WORKSPACE and untouched(*gn.last)
        assert gn.backward("bwd", xd, xd, gd, bd, stats, 0, drop=drop, ws_bytes=gn.query - 1)[0] == ERR_WORKSPACE and untouched(*gn.last)
    if dt == "f32":
        need = 4 * E.workspace_floats(s, "bwd_partials")
        part = torch.zeros(n, 1, 2, c, device=DEV)
        assert gn.backward("bwd_partials", xd, xd, gd, bd, stats, 0, partial=part, ws_bytes=need - 1)[0] == ERR_WORKSPACE and untouched(*gn.last)


def _every_entry_point(gn, x, v, st, with_plain=True, with_drop=True):
    """(name, rc, outputs untouched) of every entry point of the family on one shape; x doubles as dy, v as gamma / beta, st as mean / rstd"""
    out = []
    part_f = torch.zeros(gn.n, 1, gn.g, 2, device=DEV)
    part_b = torch.zeros(gn.n, 1, 2, gn.c, device=DEV)
    drops = ([None] if with_plain else []) + ([(0.5, E.DROP_SEED)] if with_drop else [])
    for drop in drops:
        sfx = "_drop" if drop else ""
        for entry in ("fwd", "fwd_partials", "apply"):
            rc = gn.forward(entry, x, v, v, 1, partial=part_f, stats=(st, st), drop=drop, ws_bytes=1 << 20)[0]
            out.append((entry + sfx, rc, untouched(*gn.last)))
        rc = gn.backward("bwd", x, x, v, v, (st, st), 1, drop=drop, ws_bytes=1 << 20)[0]
        out.append(("bwd" + sfx, rc, untouched(*gn.last)))
    if gn.dt == "f32" and with_plain:
        rc = gn.backward("bwd_partials", x, x, v, v, (st, st), 1, partial=part_b, ws_bytes=1 << 20)[0]
        out.append(("bwd_partials", rc, untouched(*gn.last)))
    return out


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_refused_shapes_are_refused_by_every_entry_point(hip_lib, dt):
    L = hip_lib
    for n, c, g, hw, why in E.REFUSED[dt]:
        gn = Gn(L, dt, n, c, g, hw)
        assert gn.query == 0, "workspace query of a refused shape (%s)" % why
        x = dev(torch.ones(n, hw, c), dt)
        v, st = torch.ones(c, device=DEV), torch.ones(n * g, device=DEV)
        res = _every_entry_point(gn, x, v, st)
        assert len(res) == (9 if dt == "f32" else 8)
        for name, rc, clean in res:
            assert rc == ERR_ARG, "%s took n=%d c=%d g=%d hw=%d (%s): rc %d" % (name, n, c, g, hw, why, rc)
            assert clean, "%s wrote to its outputs before refusing (%s)" % (name, why)
    if dt == "f32":
        for n, c, g, hw, why in E.F32_REFUSED_DROP_ONLY:
            gn = Gn(L, dt, n, c, g, hw)
            x = dev(torch.ones(n, hw, c), dt)
            v, st = torch.ones(c, device=DEV), torch.ones(n * g, device=DEV)
            for name, rc, clean in _every_entry_point(gn, x, v, st, with_plain=False):
                assert rc == ERR_ARG and clean, "%s: %s" % (name, why)
                assert b"C % 8" in L.odvae_last_error()
            assert gn.forward("fwd", x, v, v, 1)[0] == OK          # the plain forms take C = 100
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,case", [("f32", E.F32_CASES[0]), ("bf16", E.BF16_CASES[3])], ids=["f32", "bf16"])
def test_misaligned_operands_are_refused(hip_lib, dt, case):
    """x, y, dy or dx four bytes off a 16-byte boundary: ODVAE_ERR_ARG, nothing written"""
    L = hip_lib
    n, c, g, hw, _ = case
    gn = Gn(L, dt, n, c, g, hw)
    per = 2 if dt == "f32" else 4                              # elements in 8 bytes; the operand starts 4 bytes in
    big = dev(torch.ones(n * hw * c + per), dt)
    x = big[:n * hw * c].view(n, hw, c)
    off = big.data_ptr() + 4
    v, st = torch.ones(c, device=DEV), torch.ones(n * g, device=DEV)
    part = torch.zeros(n, 1, g, 2, device=DEV)
    for drop in (None, (0.5, E.DROP_SEED)) if c % 8 == 0 else (None,):
        for entry in ("fwd", "fwd_partials", "apply"):
            for kw in (dict(x_ptr=off), dict(y_off=4)):
                rc = gn.forward(entry, x, v, v, 1, partial=part, stats=(st, st), drop=drop, **kw)[0]
                assert rc == ERR_ARG and untouched(*gn.last), "%s %s" % (entry, kw)
        for kw in (dict(ptrs={"x": off}), dict(ptrs={"dy": off}), dict(dx_off=4)):
            rc = gn.backward("bwd", x, x, v, v, (st, st), 1, drop=drop, **kw)[0]
            assert rc == ERR_ARG and untouched(*gn.last), "bwd %s" % kw
    if dt == "f32":
        part_b = torch.zeros(n, 1, 2, c, device=DEV)
        for kw in (dict(ptrs={"x": off}), dict(ptrs={"dy": off}), dict(dx_off=4)):
            assert gn.backward("bwd_partials", x, x, v, v, (st, st), 1, partial=part_b, **kw)[0] == ERR_ARG and untouched(*gn.last)
    assert gn.forward("fwd", x, v, v, 1)[0] == OK              # the same operands aligned are taken


def test_bf16_group_norm_at_96_channels_fails_loudly_through_the_op_layer(hip_lib):
    """ch: 96 under precision: bf16 reaches the bf16 kernels with C = 96, which they do not take: an error with the library's message"""
    from odvae_amd import lib, ops
    x = torch.randn(1, 96, 4, 4, device=DEV).to(BF).contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.ones(96, device=DEV, requires_grad=True), torch.zeros(96, device=DEV)
    with pytest.raises(lib.HipLibraryError, match=r"unsupported shape N=1 HW=16 C=96 G=32 .*256%\(C/8\)==0"):
        ops.group_norm(x, gamma, beta, 32, 1e-6, swish=True)
    y = ops.group_norm(x.float(), gamma, beta, 32, 1e-6, swish=True)      # the f32 kernels take it
    assert torch.isfinite(y).all()
