"""Synchronised BatchNorm + LeakyReLU(0.2): sharded inputs, the float64 reference on the concatenated rows, a host model of the kernels.

"Ranks" are shards of one [1, c, rows, 1] tensor along the rows.  `make_shards` puts consecutive shards on opposite sides of zero:

    x_w = side_w (r sign_c + SEP) + randn,   side_w = +1, -1, +1, ...   (sign_c alternates from channel to channel, SEP = 2)

so that the shards' means differ by 2 (r + SEP) standard deviations of a shard and the variance of the concatenated rows is carried by
the delta^2 term of the merge, at r = 0 already (4 SEP^2 n_a n_b / n^2 against 1 within a shard).  Inside a shard the mean lies
r + SEP deviations from zero: the ladder of tests/bn_offset_inputs.py, which the per-shard pivot sums have to stand.

The reference everywhere is `bn_offset_inputs.ref64` / `backward_refs` on the CONCATENATED tensor (float64 F.batch_norm in training
mode), torch f32 on it for the yardstick of `gn_offset_inputs.figure`.

`model` is csrc/gan_norm.hip's synchronised route in float64 on the host: per shard a record {rows, mean, M2}, the records merged
pairwise in index order by Chan's update, mean and rstd rounded to f32 as the merge kernel stores them, the running estimates with the
unbiased variance over the total count, y from the merged statistics, per-shard sums (sum g, sum g xhat) added in index order, dx with
the total count.  `fault=` plants one of FAULTS, the mistakes a synchronised BatchNorm is prone to; tests/test_syncbn_inputs.py shows
the acceptance rule admits the model and rejects each of them on these inputs.
Plain module: no fixtures, no device.
"""
import torch

import bn_offset_inputs as B
import gn_offset_inputs as G

SEP = 2.0
FAULTS = ("no_delta_term",          # var = mean of the per-shard variances: M2 = sum M2_w
          "local_unbiased_count",   # running_var corrected by n_local / (n_local - 1) of shard `rank`
          "dx_over_local_rows",     # dx of a shard divided by its own row count
          "equal_weights")          # the merge weighs every shard as if all held n / world rows


def sides(world):
    return [1.0 - 2.0 * (w % 2) for w in range(world)]


def make_shards(counts, c, r, seed_salt=37):
    """list of f32 [1, c, n_w, 1], consecutive shards on opposite sides of zero (module docstring)"""
    out = []
    for w, (n, side) in enumerate(zip(counts, sides(len(counts)))):
        g = torch.Generator().manual_seed(G.seed_of((len(counts), c, n, w), r, 1.0, seed_salt))
        centre = side * (r * B.channel_signs(c) + SEP).view(1, c, 1, 1)
        out.append((centre + torch.randn(1, c, n, 1, generator=g)).float())
    return out


def concat(shards):
    return torch.cat(shards, 2)


def split(t, counts):
    return list(torch.split(t, list(counts), 2))


def record64(x):
    """(rows, mean [c], M2 [c]) of one shard in float64"""
    v = B.rows_of(x.double())
    mean = v.mean(0)
    return float(v.shape[0]), mean, ((v - mean) ** 2).sum(0)


def merge64(records, fault=None):
    """Chan's pairwise update in index order: (n, mean, M2) of the union"""
    world = len(records)
    n_all = sum(rec[0] for rec in records)
    count = (lambda rec: n_all / world) if fault == "equal_weights" else (lambda rec: rec[0])
    n, mu, m2 = count(records[0]), records[0][1].clone(), records[0][2].clone()
    for rec in records[1:]:
        nb = count(rec)
        nt = n + nb
        delta = rec[1] - mu
        mu = mu + delta * (nb / nt)
        m2 = m2 + rec[2] + (0.0 if fault == "no_delta_term" else delta * delta * (n * nb / nt))
        n = nt
    return n_all, mu, m2


def model(shards, gamma, beta, rm0, rv0, dys=None, fault=None, rank=0, eps=B.EPS, momentum=B.MOMENTUM, slope=B.SLOPE):
    """The synchronised route in float64.  dict: mean, rstd (f32, as stored), running_mean, running_var (f32), y (list per shard,
    float64) and, given dys, dx (list per shard), dgamma, dbeta (the sums over the shards of the local ones)."""
    c = shards[0].shape[1]
    records = [record64(x) for x in shards]
    n, mu, m2 = merge64(records, fault)
    var = (m2 / n).clamp_min(0.0)
    mean, rstd = mu.float(), (1.0 / torch.sqrt(var + eps)).float()
    n_unb = records[rank][0] if fault == "local_unbiased_count" else n
    unbiased = var * n_unb / (n_unb - 1.0) if n_unb > 1 else var
    out = {"mean": mean, "rstd": rstd, "rows": n,
           "running_mean": ((1.0 - momentum) * rm0.double() + momentum * mu).float(),
           "running_var": ((1.0 - momentum) * rv0.double() + momentum * unbiased).float()}
    v = lambda t: t.double().view(1, c, 1, 1)
    xh = [(x.double() - v(mean)) * v(rstd) for x in shards]
    u = [h * v(gamma) + v(beta) for h in xh]
    out["y"] = [torch.where(t > 0, t, slope * t) for t in u]
    if dys is not None:
        g = [dy.double() * torch.where(t > 0, 1.0, slope) for dy, t in zip(dys, u)]
        local = [(B.rows_of(gi).sum(0), B.rows_of(gi * hi).sum(0)) for gi, hi in zip(g, xh)]
        sum_g, sum_gxh = local[0][0].clone(), local[0][1].clone()
        for a, b in local[1:]:
            sum_g, sum_gxh = sum_g + a, sum_gxh + b
        out["dx"] = []
        for gi, hi, rec in zip(g, xh, records):
            m = rec[0] if fault == "dx_over_local_rows" else n
            out["dx"].append(v(gamma) * v(rstd) * (gi - (v(sum_g) + hi * v(sum_gxh)) / m))
        out["dbeta"], out["dgamma"] = sum_g, sum_gxh
    return out


class Reference:
    """float64 and torch-f32 BatchNorm + LeakyReLU on the concatenated shards, computed once per case"""

    def __init__(self, shards, with_backward=True, dy_round=None):
        self.counts = [x.shape[2] for x in shards]
        self.x = concat(shards)
        c = self.c = self.x.shape[1]
        self.gamma, self.beta = B.affine(c)
        self.rm0, self.rv0 = B.running_start(c)
        self.mean64, self.var64, self.rstd64 = B.stats64(self.x)
        self.y64, self.rm64, self.rv64 = B.ref64(self.x, self.gamma, self.beta, self.rm0, self.rv0)
        self.y32, self.rm32, self.rv32, self.mean32, self.rstd32 = B.ref32(self.x, self.gamma, self.beta, self.rm0, self.rv0)
        if with_backward:
            dy = B.kink_free_dy(B.preact64(self.x, self.gamma, self.beta), G.seed_of(self.x.shape, 0, 1.0, 41))
            self.dy = dy if dy_round is None else dy_round(dy)
            self.dys = split(self.dy, self.counts)
            self.back = B.backward_refs(self.x, self.gamma, self.beta, self.dy)

    def stat_figures(self, mean, rstd, running_mean, running_var, prefix=""):
        std, var = (self.var64 + B.EPS).sqrt(), self.var64 + B.EPS
        figs = G.stat_figures(mean, rstd, self.mean64, self.rstd64, self.mean32, self.rstd32, prefix)
        figs.append(G.figure(prefix + "running_mean / std64", running_mean.cpu().double() / std, self.rm64 / std, self.rm32.double() / std, G.FLOOR_FWD))
        figs.append(G.figure(prefix + "running_var / var64", running_var.cpu().double() / var, self.rv64 / var, self.rv32.double() / var, G.FLOOR_FWD))
        return figs

    def y_figure(self, ys, prefix=""):
        return G.figure(prefix + "y", concat([t.detach().cpu().double() for t in ys]), self.y64, self.y32, G.FLOOR_FWD)

    def backward_figures(self, dxs, dgamma, dbeta, prefix=""):
        got = (concat([t.detach().cpu().double() for t in dxs]), dgamma, dbeta)
        return [G.figure(prefix + name, q, q64, q32, floor) for name, q, q64, q32, floor in
                zip(("dx", "dgamma", "dbeta"), got, self.back[64], self.back[32], (G.FLOOR_DX, G.FLOOR_PARAM, G.FLOOR_PARAM))]

    def model_figures(self, out, prefix=""):
        figs = self.stat_figures(out["mean"], out["rstd"], out["running_mean"], out["running_var"], prefix) + [self.y_figure(out["y"], prefix)]
        if "dx" in out:
            figs += self.backward_figures(out["dx"], out["dgamma"], out["dbeta"], prefix)
        return figs
