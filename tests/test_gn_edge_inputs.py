"""The GroupNorm edge cases say what they claim, and their expectations can be trusted (CPU only).

tests/test_groupnorm_edges_gpu.py holds the kernels to the tables, exact inputs, references and host-built partial sums of
tests/gn_edge_inputs.py; here each of those is checked on its own: the branch facts of every case recomputed from the shape, the
exact inputs' arithmetic claims, the float64 references against autograd, the partial sums against the statistics and gradients they
must add up to, torch f32 alone inside the acceptance rule, and the refused-shape tables against the `make_shape` restatements.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_edge_inputs as E
import gn_offset_inputs as G

ALL = [(dt, case) for dt in ("f32", "bf16") for case in E.CASES[dt]]
ALL_IDS = ["%s-%s" % (dt, E.case_id(case)) for dt, case in ALL]
SMALL = [(dt, case) for dt, case in ALL if case[0] * case[1] * case[3] <= 200000]      # the float64 autograd checks: every branch but the two largest tensors
SMALL_IDS = ["%s-%s" % (dt, E.case_id(case)) for dt, case in SMALL]


@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_claimed_branch_facts_hold(dt, case):
    n, c, g, hw, claimed = case
    assert E.shape_of(dt, n, hw, c, g) is not None, "the library refuses this shape"
    got = E.facts(dt, n, c, g, hw)
    for key, want in claimed.items():
        assert got[key] == want, "%s: %s is %r, the table says %r" % (E.case_id(case), key, got[key], want)
    s = E.shape_of(dt, n, hw, c, g)
    assert (s["chunks"] - 1) * s["ppc"] < hw <= s["chunks"] * s["ppc"] and 1 <= s["last"] <= s["ppc"]
    assert s["ppp"] * s["c"] <= (2048 if dt == "bf16" else 1024)        # the LDS rows psub * C + c of the statistics kernels
    assert n * c * hw * 4 <= 11e6                                       # "the largest tensor is about 10 MB"


def test_the_tables_cover_the_branches():
    f = [E.facts("f32", *c[:4]) for c in E.F32_CASES]
    b = [E.facts("bf16", *c[:4]) for c in E.BF16_CASES]
    assert {3, 5, 6, 12} <= {x["cpg"] for x in f if x["generic"]}                       # CB < 64
    assert {1, 2} <= {x["cpg"] for x in f} and {1, 2, 4} <= {x["cpg"] for x in b}       # groups narrower than a quad / an octet
    assert sum(x["wide"] for x in f) >= 2 and sum(x["wide"] for x in b) >= 2
    assert any(x["wide"] and x["chunks"] > 1 for x in f) and any(x["wide"] and x["chunks"] > 1 for x in b)
    assert {4, 1024} <= {c[1] for c in E.F32_CASES} and {8, 2048} <= {c[1] for c in E.BF16_CASES}
    assert {1, 256} <= {c[2] for c in E.F32_CASES} and {1, 256} <= {c[2] for c in E.BF16_CASES}
    assert 1 in {c[3] for c in E.F32_CASES} and 1 in {c[3] for c in E.BF16_CASES}
    assert any(c[3] < x["ppp"] for c, x in zip(E.F32_CASES, f)) and any(c[3] < x["ppp"] for c, x in zip(E.BF16_CASES, b))
    assert any(x["last"] < x["ppp"] for x in f + b)                                     # a last chunk shorter than one pass
    assert {255, 256, 257} <= {c[3] for c in E.F32_CASES}
    assert {True, False} <= {x["read_once"] for x in f}
    # read-once items (sample x 32-channel slab) beyond two per block of a grid of at most 2 x 256 blocks: the refill of gn_bwd_fused_kernel
    assert any(x["read_once"] and c[0] * (c[1] // 32) > 2 * 512 for c, x in zip(E.F32_CASES, f))
    assert all(c[1] % 8 == 0 for c in E.BF16_CASES) and sum(c[1] % 8 == 0 for c in E.F32_CASES) >= 10      # the dropout forms' cases


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_exact_inputs_sum_exactly_and_predict_one_rounding(dt, case, regime):
    n, c, g, hw, _ = case
    ex = E.exact_case(case, regime)
    x = ex.x64
    assert ex.x.dtype == torch.float32 and tuple(ex.x.shape) == (n, hw, c) and np.array_equal(ex.x.numpy().astype(np.int64), x)
    assert E.is_bf16(ex.x) and np.abs(x).max() <= 256                          # integers of at most 8 significant bits
    xg = x.reshape(n, hw, g, c // g).transpose(0, 2, 1, 3).reshape(n, g, -1)
    assert (np.abs(xg).sum(2) < 2 ** 24).all() and ((xg * xg).sum(2) < 2 ** 24).all()      # every partial sum, in any order, is an integer below 2^24
    # three summation orders in f32: memory order, reversed, and pairwise (numpy's own), all equal to the integer sums
    xf = xg.astype(np.float32)
    for name, arr in (("x", xf), ("x^2", xf * xf)):
        exact = (xg if name == "x" else xg * xg).sum(2)
        seq = np.cumsum(arr, axis=2, dtype=np.float32)[..., -1]
        rev = np.cumsum(arr[..., ::-1], axis=2, dtype=np.float32)[..., -1]
        pair = arr.sum(2, dtype=np.float32)
        perm = np.cumsum(arr[..., np.random.default_rng(3).permutation(arr.shape[2])], axis=2, dtype=np.float32)[..., -1]
        for got in (seq, rev, pair, perm):
            assert np.array_equal(got.astype(np.int64), exact), name
    # mean and variance are the predicted ones
    assert np.array_equal(xg.sum(2), ex.m * ex.count)
    assert np.array_equal(((xg - ex.m[:, :, None]) ** 2).sum(2), ex.s * ex.s * (ex.count - ex.count % 2))
    # the ratio is on the intended side of the threshold by a factor of two or more
    ratio = np.abs(ex.m) / np.sqrt(ex.var)
    if regime == "near":
        assert ratio.max() <= E.RECENTRE_RATIO / 2 and ex.recentred == 0
    else:
        assert ratio.min() >= 2 * E.RECENTRE_RATIO and ex.recentred == n * g
    # neighbouring groups and samples differ in (m, s)
    ms = np.stack([ex.m, ex.s], 2)
    if g > 1:
        assert (ms[:, 1:] != ms[:, :-1]).any(2).all()
    if n > 1:
        assert (ms[1:] != ms[:-1]).any(2).all()
    # both evaluation orders of the finalize kernel give the predicted f32 statistics: E[x^2] - E[x]^2 and the centred sums
    cnt = np.float64(ex.count)
    mu = xg.sum(2).astype(np.float64) / cnt
    eps = np.float64(np.float32(E.EPS))
    var_un = np.maximum((xg * xg).sum(2).astype(np.float64) / cnt - mu * mu, 0.0)
    var_ce = ((xg - ex.m[:, :, None]) ** 2).sum(2).astype(np.float64) / cnt
    assert (mu * mu > 64.0 * var_un).all() if regime == "far" else not (mu * mu > 64.0 * var_un).any()
    for var in (var_un, var_ce):
        assert np.array_equal((1.0 / np.sqrt(var + eps)).astype(np.float32), ex.rstd.numpy())
    assert np.array_equal(mu.astype(np.float32), ex.mean.numpy())
    # y: a float64 evaluation rounded once; bf16: rounded once more; nothing under- or overflows
    assert torch.equal(ex.y64().float(), ex.y) and torch.isfinite(ex.y).all()
    assert E.is_bf16(ex.y_bf16) and ((ex.y_bf16.double() - ex.y.double()).abs() <= E.half_ulp_bf16(ex.y.double())).all()
    assert (ex.y[ex.y != 0].abs() >= 2.0 ** -60).all() and int((ex.y == 0).sum()) == n * g * (ex.count % 2)      # zero only at an odd group's one m
    # gamma: powers of two, all different inside an octet
    gm = ex.gamma
    assert torch.equal(torch.frexp(gm.abs())[0], torch.full((c,), 0.5))
    for o in range(0, c, 8):
        assert len(set(gm[o:o + 8].abs().tolist())) == min(8, c - o)
    # agreement with plain float64 GroupNorm to f32 accuracy (the prediction is not a private convention)
    ref = E.nhwc(G.ref64(E.nchw(ex.x), ex.gamma, ex.beta, False, g))
    assert (ref - ex.y.double()).abs().max().item() <= 4e-7 * ref.abs().max().item()


@pytest.mark.parametrize("dt,case", [(dt, c) for dt, c in ALL if c[1] % 8 == 0 and c[0] * c[1] * c[3] <= 200000],
                         ids=lambda v: v if isinstance(v, str) else E.case_id(v))
def test_dropout_expectations(dt, case):
    ex = E.exact_case(case, "near")
    base = ex.y_bf16 if dt == "bf16" else ex.y
    assert torch.equal(ex.dropped(0.0, dt), base)
    assert (ex.dropped(1.0, dt) == 0).all()
    half = ex.dropped(0.5, dt)
    kept = half != 0
    assert torch.equal(half[kept], 2 * base[kept])                             # scale 2 commutes with either rounding
    live = base != 0
    frac = kept[live].float().mean().item()
    assert abs(frac - 0.5) <= 4 * 0.5 / live.sum().item() ** 0.5 + 1e-9        # four sigma of a fair coin


def test_bf16_helpers():
    t = torch.tensor([1.0, 1.00390625, 1.01171875, -3.0e-5, 65280.0, 0.0, 2.0 ** -130, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert torch.equal(E.bf16_round(t), t.to(torch.bfloat16).float())          # torch rounds to nearest even too
    g = torch.Generator().manual_seed(1)
    r = torch.randn(4096, generator=g) * torch.exp(4 * torch.randn(4096, generator=g))
    assert torch.equal(E.bf16_round(r), r.to(torch.bfloat16).float())
    assert torch.equal(E.bf16_bits(r).to(torch.int16), r.to(torch.bfloat16).view(torch.int16))
    q = torch.tensor([1.0, 1.999, 2.0, 0.75, -0.75, 0.0, 3e-39], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -9, 2.0 ** -134, 2.0 ** -134], dtype=torch.float64)
    assert torch.equal(E.half_ulp_bf16(q), want)
    assert ((E.bf16_round(r).double() - r.double()).abs() <= E.half_ulp_bf16(r.double())).all()


@pytest.mark.parametrize("dt,case", SMALL, ids=SMALL_IDS)
def test_references_agree_with_float64_autograd(dt, case):
    """gn_offset_inputs' references with `groups` passed, and this module's closed-form backward sums, against torch autograd in float64"""
    n, c, g, hw, _ = case
    rc = E.rule_case(dt, case, 4)
    for swish in (False, True):
        x = rc.x4.double().requires_grad_(True)
        gm, bt = rc.gamma.double().requires_grad_(True), rc.beta.double().requires_grad_(True)
        y = F.group_norm(x, g, gm, bt, eps=E.EPS)
        y = F.silu(y) if swish else y
        y.backward(rc.dy4.double())
        y64 = rc.forward_refs(swish)[0]
        refs = rc.backward_refs(swish)[64]
        assert torch.equal(E.nchw(y64), y.detach())
        assert torch.equal(E.nchw(refs[0]), x.grad) and torch.equal(refs[1], gm.grad) and torch.equal(refs[2], bt.grad)
        # the per-element sums the backward partials are cut from: summed over samples and pixels they are dgamma and dbeta
        per = E.bwd_pixel_sums(rc.x, rc.dy, rc.gamma, rc.beta, swish, g)
        scale = max(1.0, gm.grad.abs().max().item(), bt.grad.abs().max().item())
        assert (per[:, :, 0].sum((0, 1)) - gm.grad).abs().max().item() <= 1e-10 * scale
        assert (per[:, :, 1].sum((0, 1)) - bt.grad).abs().max().item() <= 1e-10 * scale
    mean, rstd = G.stats64(rc.x4, g)
    xg = rc.x4.double().reshape(n, g, -1)
    assert torch.allclose(mean, xg.mean(2), rtol=0, atol=1e-14) and torch.allclose(rstd, (xg.var(2, unbiased=False) + E.EPS).rsqrt(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dt,case", ALL, ids=ALL_IDS)
def test_forward_partials_reproduce_the_statistics(dt, case):
    n, c, g, hw, _ = case
    count = float(hw * (c // g))
    for x, exact in ((E.exact_case(case, "far").x, True), (E.rule_case(dt, case, 4).x, False)):
        mean64, rstd64 = G.stats64(E.nchw(x), g)
        for chunks in E.FWD_CHUNK_COUNTS:
            p = E.fwd_partials(x, g, chunks)
            assert p.dtype == torch.float32 and tuple(p.shape) == (n, chunks, g, 2) and p.is_contiguous()
            b = E.cuts(hw, chunks, 101 * chunks)
            assert b[0] == 0 and b[-1] == hw and (np.diff(b) >= 0).all() and len(b) == chunks + 1
            tot = p.double().sum(1)
            mu = tot[..., 0] / count
            var = (tot[..., 1] / count - mu * mu).clamp(min=0)
            if exact:      # integers: the cut changes no bit
                xg = x.double().reshape(n, hw, g, c // g)
                assert torch.equal(tot[..., 0], xg.sum((1, 3))) and torch.equal(tot[..., 1], (xg * xg).sum((1, 3)))
            else:          # f32 partials: 2^-24 of each sum, amplified by (1 + r^2) = 17 in the variance
                assert ((mu - mean64) * rstd64).abs().max().item() <= 1e-6
                assert ((var + E.EPS).rsqrt() / rstd64 - 1).abs().max().item() <= 1e-5
    if hw >= 3:
        assert len({tuple(E.cuts(hw, 3, s)) for s in range(8)}) > 1           # arbitrary boundaries, not an even split


@pytest.mark.parametrize("dt,case", SMALL, ids=SMALL_IDS)
def test_backward_partials_reproduce_the_float64_sums(dt, case):
    n, c, g, hw, _ = case
    rc = E.rule_case(dt, case, 4)
    for swish in (False, True):
        refs = rc.backward_refs(swish)[64]
        scale = max(1.0, refs[1].abs().max().item(), refs[2].abs().max().item())
        for chunks in E.BWD_CHUNK_COUNTS:
            p = E.bwd_partials(rc.x, rc.dy, rc.gamma, rc.beta, swish, g, chunks)
            assert p.dtype == torch.float32 and tuple(p.shape) == (n, chunks, 2, c) and p.is_contiguous()
            tot = p.double().sum((0, 1))
            # f32 rounding of n * chunks partials, each below the scale of a whole gradient entry
            assert (tot[0] - refs[1]).abs().max().item() <= 1e-6 * scale * n
            assert (tot[1] - refs[2]).abs().max().item() <= 1e-6 * scale * n


@pytest.mark.parametrize("r", E.RULE_RATIOS)
@pytest.mark.parametrize("dt,case", SMALL, ids=SMALL_IDS)
def test_torch_f32_alone_is_inside_the_rule(dt, case, r):
    """the reference's own arithmetic under the rule the kernels are held to; bf16: its f32 result rounded once"""
    n, c, g, hw, _ = case
    rc = E.rule_case(dt, case, r)
    ratio = G.realised_ratio(rc.x4, g)
    assert torch.isfinite(ratio).all() and ratio.max().item() <= (4 if r == 0 else 8 * r)      # (the mean of 8 or more normal values: 4 std would be 11 sigma)
    assert rc.rstd64.max().item() <= 20          # no near-constant group: rstd would amplify every rounding of x - mean
    for swish in (False, True):
        y64, y32, mean32, rstd32 = rc.forward_refs(swish)
        figs = G.stat_figures(mean32, rstd32, rc.mean64, rc.rstd64, mean32, rstd32)
        bw = rc.backward_refs(swish)
        if dt == "bf16":
            figs.append(E.bf16_elementwise("y", E.bf16_round(y32), y64, y32, G.FLOOR_FWD))
            figs.append(E.bf16_elementwise("dx", E.bf16_round(bw[32][0]), bw[64][0], bw[32][0], G.FLOOR_DX))
        else:
            figs.append(G.figure("y", y32, y64, y32, G.FLOOR_FWD))
            figs.append(G.figure("dx", bw[32][0], bw[64][0], bw[32][0], G.FLOOR_DX))
        figs += [G.figure("dgamma", bw[32][1], bw[64][1], bw[32][1], G.FLOOR_PARAM), G.figure("dbeta", bw[32][2], bw[64][2], bw[32][2], G.FLOOR_PARAM)]
        G.check(figs, "torch f32 %s %s r%d swish%d" % (dt, E.case_id(case), r, swish))
    assert len(set(rc.gamma.tolist())) == c and rc.gamma.abs().min().item() >= 0.5


def test_the_bf16_figure_can_fail():
    q64 = torch.tensor([1.0, 0.3, -2.5], dtype=torch.float64)
    good = E.bf16_round(q64.float())
    assert G.inside(E.bf16_elementwise("q", good, q64, q64.float(), G.FLOOR_FWD))
    bad = good.clone()
    bad[1] += 2.0 ** -9                                                        # one bf16 ulp at 0.3
    assert not G.inside(E.bf16_elementwise("q", bad, q64, q64.float(), G.FLOOR_FWD))
    nan = good.clone()
    nan[2] = float("nan")
    assert not G.inside(E.bf16_elementwise("q", nan, q64, q64.float(), G.FLOOR_FWD))


def test_refused_shapes_agree_with_the_restatements():
    for n, c, g, hw, why in E.F32_REFUSED:
        assert E.shape_f32(n, hw, c, g) is None, why
    for n, c, g, hw, why in E.BF16_REFUSED:
        assert E.shape_bf16(n, hw, c, g) is None, why
    for n, c, g, hw, why in E.F32_REFUSED_DROP_ONLY:
        assert E.shape_f32(n, hw, c, g) is not None and c % 8 != 0, why
    # each refusal is caused by the reason given: the nearest shape without it is taken
    assert E.shape_f32(1, 8, 8, 1) and E.shape_f32(1, 4, 1024, 4) and E.shape_f32(1, 4, 256, 256) and E.shape_f32(65535, 1, 4, 1)
    assert E.shape_f32(1, 8, 96, 32) and E.shape_bf16(1, 8, 128, 32) and E.shape_bf16(1, 8, 8, 1) and E.shape_bf16(1, 2, 2048, 32)
    assert E.shape_bf16(1, 4, 1024, 256) and E.shape_bf16(65535, 1, 8, 1)
    # what the issue lists
    assert {6, 1028} <= {r[1] for r in E.F32_REFUSED} and 257 in {r[2] for r in E.F32_REFUSED} and 65536 in {r[0] for r in E.F32_REFUSED}
    assert {96, 4, 4096} <= {r[1] for r in E.BF16_REFUSED} and 512 in {r[2] for r in E.BF16_REFUSED}
    assert any(r[1] % r[2] for r in E.F32_REFUSED) and E.F32_REFUSED_DROP_ONLY[0][1] == 100


def test_workspace_restatement():
    s = E.shape_f32(2, 70, 96, 32)
    assert E.workspace_floats(s, "fwd") == 2 * 2 * 32 * 2 and E.workspace_floats(s, "bwd") == 2 * 2 * 2 * 96 + 2 * 2 * 96 + 2 * 32 * 2
    assert E.workspace_bytes("f32", s) == 4 * E.workspace_floats(s, "bwd")
    s = E.shape_f32(2, 1, 128, 64)        # read-once: 8 items -> 256 bytes of counters, [N][1][2][C] partials, chan, grp
    assert E.workspace_bytes("f32", s) == 256 + 4 * (2 * 2 * 128 + 2 * 2 * 128 + 2 * 64 * 2)
    s = E.shape_bf16(2, 3, 2048, 256)     # forward larger than nothing here: backward dominates
    assert E.workspace_bytes("bf16", s) == 4 * (2 * 1 * 2 * 2048 + 2 * 2 * 2048 + 2 * 256 * 2)
