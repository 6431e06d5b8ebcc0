"""Synchronised BatchNorm + LeakyReLU(0.2) through the C ABI on one device: shards of one tensor stand in for the ranks.

record (per shard) -> merge -> apply, and sums (per shard) -> dx (per shard), f32 and bf16, exactly the calls `ops._SyncBatchNormLReLU`
makes with the exchange replaced by writing every shard's record / sums into its slot of the [world][...] f64 buffer.  The reference is
float64 BatchNorm on the CONCATENATED rows (tests/syncbn_inputs.py), never this library's own unsynchronised route; the rule is that of
tests/gn_offset_inputs.py, for bf16 outputs `bn_bounds` / `inside` of tests/test_disc_bf16_gpu.py.  Consecutive shards lie on opposite
sides of zero, so a merge without the delta^2 term, with equal weights, or a dx over the local count is far outside
(tests/test_syncbn_inputs.py shows it for exactly these inputs).

Splits: 2 = 1 + 1; 63 = 1 + 62 and 20 + 21 + 22 at C 36 and 512 (one pass and two passes over 256 channels, C no multiple of 4, the bf16
dword path); 131073 = 1024 * 128 + 1 rows, as 131072 + 1 and as three uneven shards, where a shard's blocks walk more than 128 rows; eight
shards with one-row shards among them.
"""
import pytest
import torch

import bn_offset_inputs as B
import gn_offset_inputs as G
import syncbn_inputs as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
WRAP_ROWS = 1024 * 128 + 1

SPLITS = [((1, 1), 8),
          ((1, 62), 36), ((20, 21, 22), 36), ((1, 62), 512), ((20, 21, 22), 512),
          ((1, 5, 1, 9, 2, 1, 30, 14), 8),
          ((WRAP_ROWS - 1, 1), 8), ((50000, 40001, 41072), 8)]
assert sum(SPLITS[-1][0]) == sum(SPLITS[-2][0]) == WRAP_ROWS
SPLIT = pytest.mark.parametrize("counts,c", SPLITS, ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else "C%d" % v)
DTYPE = pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])


def to_rows(x, bf):
    """host [1, c, n, 1] -> device [n, c], the matrix the kernels walk"""
    return B.rows_of(x).contiguous().to(BF if bf else torch.float32).to(DEV)


def from_rows(t):
    """device [n, c] -> host f32 [1, c, n, 1]"""
    return t.detach().float().cpu().t().reshape(1, t.shape[1], t.shape[0], 1)


class Split:
    """The synchronised route on one device.  Every call is checked for ODVAE_OK."""

    def __init__(self, L, shards, bf, gamma, beta, rm0, rv0):
        from odvae_amd import lib
        self.L, self.lib, self.bf, self.sfx = L, lib, bf, "bf16" if bf else "f32"
        self.xs = [to_rows(x, bf) for x in shards]
        self.world, self.c = len(shards), shards[0].shape[1]
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.rm, self.rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
        c, w = self.c, self.world
        self.records = torch.zeros(w, c, 3, dtype=torch.float64, device=DEV)
        self.sums_all = torch.zeros(w, 2, c, dtype=torch.float64, device=DEV)
        self.mean, self.rstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        self.total = torch.zeros(1, dtype=torch.float64, device=DEV)
        nbytes = max(L.odvae_batchnorm_workspace_bytes(x.shape[0], c) for x in self.xs)
        self.ws, self.ws_bytes = torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes

    def ok(self, rc, what):
        self.lib.check(rc, what)

    def forward(self):
        L, c = self.L, self.c
        for w, x in enumerate(self.xs):
            self.ok(getattr(L, "odvae_batchnorm_sync_stats_record_" + self.sfx)(x.data_ptr(), x.shape[0], c, self.records[w].data_ptr(), c * 24,
                                                                                self.ws.data_ptr(), self.ws_bytes, None), "record")
        self.ok(L.odvae_batchnorm_sync_stats_merge(self.records.data_ptr(), self.records.numel() * 8, self.world, c, B.EPS, B.MOMENTUM,
                                                   self.mean.data_ptr(), self.rstd.data_ptr(), self.rm.data_ptr(), self.rv.data_ptr(),
                                                   self.total.data_ptr(), None), "merge")
        self.ys = [torch.empty_like(x) for x in self.xs]
        for x, y in zip(self.xs, self.ys):
            self.ok(getattr(L, "odvae_batchnorm_lrelu_fwd_" + self.sfx)(x.data_ptr(), x.shape[0], c, self.gamma.data_ptr(), self.beta.data_ptr(), B.EPS,
                                                                        B.MOMENTUM, B.SLOPE, 0, self.mean.data_ptr(), self.rstd.data_ptr(), None, None,
                                                                        y.data_ptr(), None, 0, None), "apply")
        return self

    def backward(self, dys):
        L, c = self.L, self.c
        self.dys = [to_rows(d, self.bf) for d in dys]
        self.dgs, self.dbs = [torch.empty(c, device=DEV) for _ in dys], [torch.empty(c, device=DEV) for _ in dys]
        for w, (x, dy) in enumerate(zip(self.xs, self.dys)):
            self.ok(getattr(L, "odvae_batchnorm_sync_bwd_sums_" + self.sfx)(x.data_ptr(), dy.data_ptr(), x.shape[0], c, self.gamma.data_ptr(),
                                                                            self.beta.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), B.SLOPE,
                                                                            self.sums_all[w].data_ptr(), c * 16, self.dgs[w].data_ptr(),
                                                                            self.dbs[w].data_ptr(), self.ws.data_ptr(), self.ws_bytes, None), "bwd_sums")
        self.dxs = [torch.empty_like(x) for x in self.xs]
        for x, dy, dx in zip(self.xs, self.dys, self.dxs):
            self.ok(getattr(L, "odvae_batchnorm_sync_bwd_dx_" + self.sfx)(x.data_ptr(), dy.data_ptr(), x.shape[0], c, self.gamma.data_ptr(),
                                                                          self.beta.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), B.SLOPE,
                                                                          self.sums_all.data_ptr(), self.sums_all.numel() * 8, self.world,
                                                                          self.total.data_ptr(), dx.data_ptr(), self.ws.data_ptr(), self.ws_bytes, None), "bwd_dx")
        return self

    def merged_sums_f32(self):
        """(sum g, sum g xhat) as bwd_dx forms them: the shards' f64 sums added in index order, rounded to f32 once"""
        s = self.sums_all.cpu()
        a = s[0].clone()
        for w in range(1, self.world):
            a = a + s[w]
        return a[0].float(), a[1].float()


def make_case(counts, c, r, bf):
    shards = S.make_shards(counts, c, r)
    rnd = (lambda t: t.to(BF).float()) if bf else None
    if bf:      # the statistics are those of the bf16 values as stored: the reference sees the rounded values
        shards = [rnd(x) for x in shards]
    return shards, S.Reference(shards, dy_round=rnd)


@pytest.mark.parametrize("r", [0, 1000])
@DTYPE
@SPLIT
def test_split_route_matches_float64_on_the_concatenated_rows(hip_lib, counts, c, bf, r):
    from test_disc_bf16_gpu import bn_bounds, inside
    shards, ref = make_case(counts, c, r, bf)
    run = Split(hip_lib, shards, bf, ref.gamma, ref.beta, ref.rm0, ref.rv0).forward().backward(ref.dys)
    what = "syncbn %s %s C %d r %d" % ("bf16" if bf else "f32", "+".join(map(str, counts)), c, r)
    assert run.total.item() == float(sum(counts))
    rec = run.records.cpu()
    assert torch.equal(rec[:, :, 0], torch.tensor(counts, dtype=torch.float64).view(-1, 1).expand(-1, c)), "record[.][c][0] is the shard's row count"
    figs = ref.stat_figures(run.mean, run.rstd, run.rm, run.rv)
    dgamma = sum(t.cpu().double() for t in run.dgs)
    dbeta = sum(t.cpu().double() for t in run.dbs)
    ys, dxs = [from_rows(t) for t in run.ys], [from_rows(t) for t in run.dxs]
    back = ref.backward_figures(dxs, dgamma, dbeta)
    if not bf:
        figs += [ref.y_figure(ys)] + back
    else:
        figs += back[1:]
    G.check(figs, what)
    if bf:      # y, dx: the kernels' formulas in float64 with the device's own statistics and sums, M the TOTAL count (x is the whole tensor)
        sum_g, sum_gxh = run.merged_sums_f32()
        bd = bn_bounds(ref.x, ref.gamma, ref.beta, run.mean.cpu(), run.rstd.cpu(), ref.dy, sum_g, sum_gxh, True)
        inside(S.concat(ys), bd["y"], bd["y_bound"], what + " y")
        inside(S.concat(dxs), bd["dx"], bd["dx_bound"], what + " dx")


@DTYPE
def test_buffers_one_byte_short_are_refused_with_the_needed_size(hip_lib, bf):
    L = hip_lib
    c, rows, world = 36, 21, 3
    sfx = "bf16" if bf else "f32"
    x = torch.zeros(rows, c, dtype=BF if bf else torch.float32, device=DEV)
    f = lambda *shape: torch.zeros(*shape, device=DEV)
    d = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=DEV)
    ws_bytes = L.odvae_batchnorm_workspace_bytes(rows, c)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rec_bytes, sums_bytes = L.odvae_batchnorm_sync_record_bytes(c), L.odvae_batchnorm_sync_sums_bytes(c)
    assert (rec_bytes, sums_bytes) == (c * 3 * 8, c * 2 * 8)
    g, b, mean, rstd = f(c) + 1, f(c), f(c), f(c) + 1
    record, records, sums, sums_all, total = d(c, 3), d(world, c, 3), d(2, c), d(world, 2, c), d(1) + world * rows
    P = lambda t: t.data_ptr()
    calls = {
        "record: record": (lambda n, w: getattr(L, "odvae_batchnorm_sync_stats_record_" + sfx)(P(x), rows, c, P(record), n, P(ws), w, None), rec_bytes, False),
        "record: workspace": (lambda n, w: getattr(L, "odvae_batchnorm_sync_stats_record_" + sfx)(P(x), rows, c, P(record), n, P(ws), w, None), rec_bytes, True),
        "merge: records": (lambda n, w: L.odvae_batchnorm_sync_stats_merge(P(records), n, world, c, B.EPS, B.MOMENTUM, P(mean), P(rstd), None, None, None, None),
                           world * rec_bytes, False),
        "bwd_sums: sums": (lambda n, w: getattr(L, "odvae_batchnorm_sync_bwd_sums_" + sfx)(P(x), P(x), rows, c, P(g), P(b), P(mean), P(rstd), B.SLOPE, P(sums), n,
                                                                                           P(f(c)), P(f(c)), P(ws), w, None), sums_bytes, False),
        "bwd_sums: workspace": (lambda n, w: getattr(L, "odvae_batchnorm_sync_bwd_sums_" + sfx)(P(x), P(x), rows, c, P(g), P(b), P(mean), P(rstd), B.SLOPE, P(sums), n,
                                                                                                P(f(c)), P(f(c)), P(ws), w, None), sums_bytes, True),
        "bwd_dx: sums": (lambda n, w: getattr(L, "odvae_batchnorm_sync_bwd_dx_" + sfx)(P(x), P(x), rows, c, P(g), P(b), P(mean), P(rstd), B.SLOPE, P(sums_all), n, world,
                                                                                       P(total), P(torch.empty_like(x)), P(ws), w, None), world * sums_bytes, False),
        "bwd_dx: workspace": (lambda n, w: getattr(L, "odvae_batchnorm_sync_bwd_dx_" + sfx)(P(x), P(x), rows, c, P(g), P(b), P(mean), P(rstd), B.SLOPE, P(sums_all), n, world,
                                                                                            P(total), P(torch.empty_like(x)), P(ws), w, None), world * sums_bytes, True),
    }
    for name, (call, need, short_ws) in calls.items():
        rc = call(need, ws_bytes - 1) if short_ws else call(need - 1, ws_bytes)
        msg = L.odvae_last_error().decode()
        assert rc == 2, "%s: a buffer one byte short returned %d" % (name, rc)           # ODVAE_ERR_WORKSPACE
        assert str(ws_bytes if short_ws else need) in msg, "%s: %r does not name the needed size" % (name, msg)
        assert call(need, ws_bytes) == 0, "%s: the exact size is refused: %s" % (name, L.odvae_last_error().decode())
    torch.cuda.synchronize()


@pytest.mark.parametrize("r", [0, 1000])
@DTYPE
@pytest.mark.parametrize("rows,c", [(63, 36), (63, 512), (401, 32), (63, 263), (63, 520)], ids=lambda v: str(v))      # the last two: a partial second 256-column pass
def test_one_shard_agrees_with_the_monolithic_entry_point(hip_lib, rows, c, bf, r):
    """world = 1: the same statistics, outputs and gradients as odvae_batchnorm_lrelu_fwd / _bwd, both inside the rule against float64
    and no further from each other than the rule's bound; dx, dgamma, dbeta given the SAME mean and rstd bit for bit."""
    L = hip_lib
    from odvae_amd import lib
    shards, ref = make_case((rows,), c, r, bf)
    run = Split(L, shards, bf, ref.gamma, ref.beta, ref.rm0, ref.rv0).forward().backward(ref.dys)
    sfx = "bf16" if bf else "f32"
    x, dy = run.xs[0], run.dys[0]
    mean, rstd, rm, rv = torch.empty(c, device=DEV), torch.empty(c, device=DEV), ref.rm0.clone().to(DEV), ref.rv0.clone().to(DEV)
    y, dx, dg, db = torch.empty_like(x), torch.empty_like(x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    lib.check(getattr(L, "odvae_batchnorm_lrelu_fwd_" + sfx)(x.data_ptr(), rows, c, run.gamma.data_ptr(), run.beta.data_ptr(), B.EPS, B.MOMENTUM, B.SLOPE, 1,
                                                             mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), y.data_ptr(),
                                                             run.ws.data_ptr(), run.ws_bytes, None), "monolithic fwd")
    # the backward with the split route's statistics: what is left to differ is the sums' path (f64 kept against f32 stored), nothing
    lib.check(getattr(L, "odvae_batchnorm_lrelu_bwd_" + sfx)(x.data_ptr(), dy.data_ptr(), rows, c, run.gamma.data_ptr(), run.beta.data_ptr(),
                                                             run.mean.data_ptr(), run.rstd.data_ptr(), B.SLOPE, 1, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                                             run.ws.data_ptr(), run.ws_bytes, None), "monolithic bwd")
    assert torch.equal(dx, run.dxs[0]) and torch.equal(dg, run.dgs[0]) and torch.equal(db, run.dbs[0])
    what = "syncbn world 1 %s rows %d C %d r %d" % (sfx, rows, c, r)
    split_figs = ref.stat_figures(run.mean, run.rstd, run.rm, run.rv, "split ")
    mono_figs = ref.stat_figures(mean, rstd, rm, rv, "monolithic ")
    G.check(split_figs + mono_figs, what)
    pairs = [(run.mean.cpu().double() * ref.rstd64, mean.cpu().double() * ref.rstd64), (run.rstd.cpu().double() / ref.rstd64, rstd.cpu().double() / ref.rstd64),
             (run.rm.cpu().double() / (ref.var64 + B.EPS).sqrt(), rm.cpu().double() / (ref.var64 + B.EPS).sqrt()),
             (run.rv.cpu().double() / (ref.var64 + B.EPS), rv.cpu().double() / (ref.var64 + B.EPS))]
    for f, (a, b) in zip(split_figs, pairs):
        gap = G.maxerr(a, b)
        print("%s %-28s split - monolithic %.3e  bound %.3e" % (what, f["name"], gap, f["bound"]))
        assert gap <= f["bound"], "%s: %s differs from the monolithic route by %.3e > %.3e" % (what, f["name"], gap, f["bound"])
    if not bf:
        yf = ref.y_figure([from_rows(run.ys[0])], "split ")
        G.check([yf, ref.y_figure([from_rows(y)], "monolithic ")], what)
        assert G.maxerr(run.ys[0], y) <= yf["bound"]


@DTYPE
def test_without_a_group_the_calls_are_todays(hip_lib, monkeypatch, bf):
    """ops.batchnorm_lrelu with dist_group = None: workspace size, forward, workspace size, backward -- and none of the new entry points"""
    from test_disc_bf16_gpu import _Recorder
    from test_batchnorm_offset_gpu import holder
    from odvae_amd import lib, ops
    from odvae_amd.gan import BatchNormLReLU
    c = 36
    gamma, beta = B.affine(c)
    bn = BatchNormLReLU(c).to(DEV).train()
    assert bn.dist_group is None
    plain = holder(c, gamma, beta, *B.running_start(c), True)          # a torch.nn.BatchNorm2d: no such attribute at all
    x = torch.randn(2, c, 5, 3, generator=torch.Generator().manual_seed(3)).to(BF if bf else torch.float32).to(DEV)
    sfx = "bf16" if bf else "f32"
    for mod in (bn, plain):
        log = []
        with monkeypatch.context() as mp:
            rec = _Recorder(lib.load(), log)
            mp.setattr(lib, "load", lambda: rec)
            xd = x.clone().requires_grad_(True)
            y = ops.batchnorm_lrelu(xd, mod, 0.2)
            y.backward(torch.ones_like(y))
        assert log == ["odvae_batchnorm_workspace_bytes", "odvae_batchnorm_lrelu_fwd_" + sfx,
                       "odvae_batchnorm_workspace_bytes", "odvae_batchnorm_lrelu_bwd_" + sfx], log
        assert not any("sync" in name for name in log)
