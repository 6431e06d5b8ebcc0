"""GroupNorm held to float64 when a group's mean is far from zero.

Every producer of GroupNorm statistics here sums x and x^2 in f32 and ends in `gn_finalize_kernel` (csrc/gn_finalize.h), which forms
var = E[x^2] - E[x]^2: the standalone f32 pass (csrc/groupnorm.hip), the output transform of the F(4x4) Winograd conv, plain and
Upsample (csrc/conv3x3_wino4_f32.hip), the bf16 pass and the bf16 conv epilogue (csrc/bf16_ops.hip, csrc/conv_bf16.hip).  The
subtraction loses ~ u r^2 of the variance, r = |mean| / std of a (sample, group); where mu^2 > GN_RECENTRE_RATIO^2 var the finalize
kernel therefore re-reads the group and takes centred sums, and counts it (`odvae_groupnorm_recentred`).

The ladder of tests/gn_offset_inputs.py -- r in {0, 4, 16, 64, 256, 1000} at scales 1 and 0.01 -- runs through every producer and
through the three backward forms, under that module's acceptance rule against float64 (eight times torch f32's own error, or a
quarter of the project's tolerances).  The recentring must not run at r <= 4, the regime training is known to be in, and must have
run for every group from r = 16 on: there the uncentred sums of the smallest groups leave the rule, and from r = 64 on those of every
producer do (profiles/gn_offset.md has the figures with and without it).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import gn_offset_inputs as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

RUNG = pytest.mark.parametrize("rung", G.RUNGS, ids=G.rung_id)
_sid = lambda s: "x".join(map(str, s))

# (n, c, h, w): ragged chunks; one, two, eight and sixteen channels per group (and four); one block per sample
PASS_SHAPES = [(2, 64, 16, 32), (1, 256, 20, 36), (3, 128, 12, 20), (2, 32, 8, 8), (1, 512, 16, 16)]
CONV_CASES = [(2, 64, 64, 16, 32), (3, 128, 256, 36, 68)]                 # (n, cin, cout, h, w) of the OUTPUT
UP_CASES = [(2, 64, 64, 8, 16), (3, 128, 256, 18, 34)]                    # (n, cin, cout, h, w) of the INPUT: outputs as above
BF16_CASES = [(2, 64, 128, 16, 16), (1, 256, 512, 8, 16)]                 # the two smallest of test_groupnorm_statistics_from_the_bf16_conv_epilogue
BWD_SHAPES = [(2, 128, 16, 16), (2, 64, 20, 36)]                          # one block per item (read-once by default); five members, ragged


def recentred(L):
    return L.odvae_groupnorm_recentred(0)


def check_recentred(L, before, r, groups_normalised):
    """none at r <= 4; every (sample, group) of every forward call from r = 16 on (each group of the ladder has the same ratio)"""
    ran = recentred(L) - before
    if r <= 4:
        assert ran == 0, "%d groups were recentred at r = %g" % (ran, r)
    else:
        assert ran == groups_normalised, "%d of %d groups were recentred at r = %g" % (ran, groups_normalised, r)


def affine(c, on, seed=11):
    if not on:
        return torch.ones(c), torch.zeros(c)
    g = torch.Generator().manual_seed(seed + c)
    return torch.randn(c, generator=g), torch.randn(c, generator=g)


def forward_figures(xd, output=True):
    """GroupNorm of the device tensor xd (f32 or bf16, possibly carrying a conv's epilogue statistics) through ops.group_norm, first
    with gamma = 1, beta = 0 and no swish, then with random gamma, beta and swish.  The float64 and the torch f32 references are
    GroupNorm of the values xd holds.  Figures: the output (f32 only: a bf16 output's rounding, 2^-9, would hide what is looked for)
    and the saved statistics in units of the group, for both calls."""
    from odvae_amd import ops
    xh = xd.detach().float().cpu().contiguous()
    c = xh.shape[1]
    mean64, rstd64 = G.stats64(xh)
    figs = []
    for on in (False, True):
        gamma, beta = affine(c, on)
        y32, mean32, rstd32 = G.ref32(xh, gamma, beta, on)
        y = ops.group_norm(xd, gamma.to(DEV).requires_grad_(True), beta.to(DEV), 32, G.EPS, swish=on)
        mean, rstd = y.grad_fn.saved_tensors[3:5]
        tag = "affine + swish: " if on else "plain: "
        assert torch.isfinite(y.float()).all(), tag + "non-finite output"
        if output:
            figs.append(G.figure(tag + "y", y, G.ref64(xh, gamma, beta, on), y32, G.FLOOR_FWD))
        figs += G.stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32, tag)
    return figs


def conv_weight(cout, cin, s, seed):
    g = torch.Generator().manual_seed(seed)
    return s * torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin), 0.1 * s * torch.randn(cout, generator=g), g


def offset_map(shape, r, s):
    """s r sign_g on every pixel"""
    n, c, h, w = shape
    return (s * r * G.group_signs(c)).view(1, c, 1, 1).expand(n, c, h, w).contiguous()


# ---- producers, each a function of the rung that returns (figures, groups normalised) so that a measuring script can call it too ----
def pass_f32(shape, rung):
    return forward_figures(G.make_input(shape, *rung).to(DEV)), 2 * shape[0] * 32


def conv_epilogue_f32(case, rung):
    """stride-1 F(4x4) conv, the offset through the residual: y = s (conv(randn) + r sign_g)"""
    from odvae_amd import ops
    n, cin, cout, h, w = case
    r, s = rung
    wt, b, g = conv_weight(cout, cin, s, G.seed_of(case, r, s, 1))
    x = torch.randn(n, cin, h, w, generator=g)
    y = ops.conv3x3(x.to(DEV), wt.to(DEV), b.to(DEV), offset_map((n, cout, h, w), r, s).to(DEV), gn_stats=True)
    assert ops._gn_partials_of(y, 32) is not None          # not the standalone pass
    return forward_figures(y), 2 * n * 32


def up_epilogue_f32(case, rung):
    """Upsample F(4x4) conv, the offset through the bias (per channel, equal within a group)"""
    from odvae_amd import ops
    n, cin, cout, h, w = case
    r, s = rung
    wt, b, g = conv_weight(cout, cin, s, G.seed_of(case, r, s, 2))
    x = torch.randn(n, cin, h, w, generator=g)
    y = ops.conv3x3(x.to(DEV), wt.to(DEV), (s * r * G.group_signs(cout)).to(DEV), None, mode=2, gn_stats=True)
    assert tuple(y.shape) == (n, cout, 2 * h, 2 * w) and ops._gn_partials_of(y, 32) is not None
    return forward_figures(y), 2 * n * 32


def cl_bf16(t):
    return t.to(DEV).to(BF).contiguous(memory_format=torch.channels_last)


def pass_bf16(case, rung):
    n, _, c, h, w = case
    return forward_figures(cl_bf16(G.make_input((n, c, h, w), *rung)), output=False), 2 * n * 32


def conv_epilogue_bf16(case, rung):
    """bf16 stride-1 conv, the offset through the residual; the statistics are those of the bf16 tensor the conv stored"""
    from odvae_amd import ops
    n, cin, cout, h, w = case
    r, s = rung
    wt, b, g = conv_weight(cout, cin, s, G.seed_of(case, r, s, 3))
    x = torch.randn(n, cin, h, w, generator=g)
    y = ops.conv3x3(cl_bf16(x), wt.to(BF).float().to(DEV), b.to(DEV), cl_bf16(offset_map((n, cout, h, w), r, s)), gn_stats=True)
    assert y.dtype == BF and ops._gn_partials_of(y, 32) is not None
    return forward_figures(y, output=False), 2 * n * 32


def _producer_test(L, monkeypatch, fn, case, rung):
    from odvae_amd import ops
    for switch in ("WINOGRAD4", "UPCONV_WINOGRAD4", "GN_FUSED_STATS"):
        monkeypatch.setattr(ops, switch, True)
    before = recentred(L)
    figs, groups = fn(case, rung)
    check_recentred(L, before, rung[0], groups)
    G.check(figs, "%s %s %s" % (fn.__name__, _sid(case), G.rung_id(rung)))


@RUNG
@pytest.mark.parametrize("shape", PASS_SHAPES, ids=_sid)
def test_statistics_pass_f32(hip_lib, monkeypatch, shape, rung):
    _producer_test(hip_lib, monkeypatch, pass_f32, shape, rung)


@RUNG
@pytest.mark.parametrize("case", CONV_CASES, ids=_sid)
def test_statistics_from_the_f4x4_conv_epilogue(hip_lib, monkeypatch, case, rung):
    _producer_test(hip_lib, monkeypatch, conv_epilogue_f32, case, rung)


@RUNG
@pytest.mark.parametrize("case", UP_CASES, ids=_sid)
def test_statistics_from_the_f4x4_upsample_conv_epilogue(hip_lib, monkeypatch, case, rung):
    _producer_test(hip_lib, monkeypatch, up_epilogue_f32, case, rung)


@RUNG
@pytest.mark.parametrize("case", BF16_CASES, ids=_sid)
def test_statistics_pass_bf16(hip_lib, monkeypatch, case, rung):
    _producer_test(hip_lib, monkeypatch, pass_bf16, case, rung)


@RUNG
@pytest.mark.parametrize("case", BF16_CASES, ids=_sid)
def test_statistics_from_the_bf16_conv_epilogue(hip_lib, monkeypatch, case, rung):
    _producer_test(hip_lib, monkeypatch, conv_epilogue_bf16, case, rung)


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def backward_case(shape, rung, with_skip, salt):
    n, c, h, w = shape
    x = G.make_input(shape, *rung)
    g = torch.Generator().manual_seed(G.seed_of(shape, rung[0], rung[1], salt))
    dy = torch.randn(n, c, h, w, generator=g)
    dskip = torch.randn(n, c, h, w, generator=g) if with_skip else None
    gamma, beta = affine(c, True)
    return x, dy, dskip, gamma, beta


def backward_figures(got, refs, prefix=""):
    return [G.figure(prefix + name, v, q64, q32, floor)
            for name, v, q64, q32, floor in zip(("dx", "dgamma", "dbeta"), got, refs[64], refs[32], (G.FLOOR_DX, G.FLOOR_PARAM, G.FLOOR_PARAM))]


def bwd_through_ops(shape, rung, with_skip):
    from odvae_amd import ops
    x, dy, dskip, gamma, beta = backward_case(shape, rung, with_skip, 4)
    xd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    if with_skip:
        y, xs = ops.group_norm_skip(xd, gd, bd, 32, G.EPS, swish=True)
        torch.autograd.backward([y, xs], [dy.to(DEV), dskip.to(DEV)])
    else:
        ops.group_norm(xd, gd, bd, 32, G.EPS, swish=True).backward(dy.to(DEV))
    return backward_figures((xd.grad, gd.grad, bd.grad), G.backward_refs(x, gamma, beta, dy, True, dskip))


def bwd_through_the_abi(L, shape, rung, mode):
    """odvae_groupnorm_bwd_f32 in the two-kernel form (0) and the read-once form with teams (1), mean and rstd from the forward under test"""
    from odvae_amd import lib as _lib, ops
    n, c, h, w = shape
    x, dy, dskip, gamma, beta = backward_case(shape, rung, True, 5)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y = ops.group_norm(x.to(DEV), gd.clone().requires_grad_(True), bd, 32, G.EPS, swish=True)
    mean, rstd = y.grad_fn.saved_tensors[3:5]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    xn, dyn, skn = nhwc(x), nhwc(dy), nhwc(dskip)
    dx, dg, db = torch.empty_like(xn), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    wp, wn = ops._ws(L.odvae_groupnorm_workspace_bytes(n, h * w, c, 32), xn)
    prev = L.odvae_groupnorm_select_backward(mode)
    try:
        _lib.check(L.odvae_groupnorm_bwd_f32(xn.data_ptr(), dyn.data_ptr(), n, h * w, c, 32, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(),
                                             rstd.data_ptr(), 1, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), skn.data_ptr(), wp, wn,
                                             _lib.stream_ptr()), "groupnorm_bwd")
    finally:
        L.odvae_groupnorm_select_backward(prev)
    return backward_figures((dx.permute(0, 3, 1, 2), dg, db), G.backward_refs(x, gamma, beta, dy, True, dskip))


def bwd_through_the_conv_link(case, rung):
    """conv3x3(swish(GroupNorm(x))): the conv's data gradient leaves the first-pass sums of the GroupNorm's backward (GN_FUSED_BWD).
    The references are the GroupNorm's backward of the very gradient tensor the conv handed down, so conv error is excluded."""
    from odvae_amd import ops
    n, c, cout, h, w = case
    x, _, _, gamma, beta = backward_case((n, c, h, w), rung, False, 6)
    g = torch.Generator().manual_seed(G.seed_of(case, rung[0], rung[1], 7))
    wt = torch.randn(cout, c, 3, 3, generator=g) / (3.0 * c ** 0.5)
    gy = torch.randn(n, cout, h, w, generator=g)
    xd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    hits = ops.GN_FUSED_BWD_HITS
    a = ops.group_norm(xd.contiguous(memory_format=torch.channels_last), gd, bd, 32, G.EPS, swish=True)
    seen = []
    a.register_hook(lambda grad: seen.append(grad.detach().cpu().contiguous()))
    ops.conv3x3(a, wt.to(DEV), None, None).backward(gy.to(DEV))
    assert ops.GN_FUSED_BWD_HITS - hits == 1               # the GroupNorm's reduce pass did not run
    return backward_figures((xd.grad, gd.grad, bd.grad), G.backward_refs(x, gamma, beta, seen[0], True))


@RUNG
@pytest.mark.parametrize("with_skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_sid)
def test_backward_through_the_op_layer(hip_lib, shape, rung, with_skip):
    G.check(bwd_through_ops(shape, rung, with_skip), "backward %s %s" % (_sid(shape), G.rung_id(rung)))
    assert hip_lib.odvae_groupnorm_fused_timeouts() == 0


@RUNG
@pytest.mark.parametrize("mode", [0, 1], ids=["two-kernel", "read-once"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_sid)
def test_backward_through_the_c_abi(hip_lib, shape, rung, mode):
    G.check(bwd_through_the_abi(hip_lib, shape, rung, mode), "backward (C ABI, form %d) %s %s" % (mode, _sid(shape), G.rung_id(rung)))
    assert hip_lib.odvae_groupnorm_fused_timeouts() == 0


@RUNG
@pytest.mark.parametrize("case", [(2, 64, 64, 16, 32)], ids=_sid)
def test_backward_sums_from_the_conv_data_gradient(hip_lib, monkeypatch, case, rung):
    from odvae_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    monkeypatch.setattr(ops, "GN_FUSED_BWD", True)
    G.check(bwd_through_the_conv_link(case, rung), "backward (sums from the data gradient) %s %s" % (_sid(case), G.rung_id(rung)))
    assert hip_lib.odvae_groupnorm_fused_timeouts() == 0


# ---- degenerate groups ---------------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPE = (2, 64, 16, 32)       # two channels per group


def degenerate_input(kind):
    """randn everywhere but in group 5 of sample 0 and group 30 of sample 1 (channels 10-11, 60-61), which are of the given kind"""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(DEGENERATE_SHAPE, generator=g)
    for n, c0 in ((0, 10), (1, 60)):
        blk = x[n, c0:c0 + 2]
        if kind == "0.75":
            blk.fill_(0.75)
        elif kind == "0.1":
            blk.fill_(0.1)
        elif kind == "std 1e-3 around 1":
            blk.mul_(1e-3).add_(1.0)
        elif kind == "spike":
            blk.zero_()
            blk[1, 7, 19] = 1e3
    return x


def test_a_constant_group_comes_out_as_beta(hip_lib):
    """0.75 everywhere: the sums are exact, var is exactly 0 and x - mu is exactly 0, so y = 0 * rstd * gamma + beta = beta, bit for bit"""
    from odvae_amd import ops
    x = degenerate_input("0.75")
    gamma, beta = affine(64, True)
    y = ops.group_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, G.EPS, swish=False).cpu()
    for n, c0 in ((0, 10), (1, 60)):
        assert torch.equal(y[n, c0:c0 + 2], beta[c0:c0 + 2].view(2, 1, 1).expand(2, 16, 32))
    assert torch.isfinite(y).all()


def test_a_constant_conv_output_comes_out_as_beta(hip_lib, monkeypatch):
    """the same through the conv epilogue: zero weights, bias 0.75, no residual"""
    from odvae_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    monkeypatch.setattr(ops, "GN_FUSED_STATS", True)
    n, c, h, w = DEGENERATE_SHAPE
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(3))
    y = ops.conv3x3(x.to(DEV), torch.zeros(c, c, 3, 3, device=DEV), torch.full((c,), 0.75, device=DEV), None, gn_stats=True)
    assert ops._gn_partials_of(y, 32) is not None
    assert torch.equal(y.cpu(), torch.full((n, c, h, w), 0.75))
    gamma, beta = affine(c, True)
    z = ops.group_norm(y, gamma.to(DEV), beta.to(DEV), 32, G.EPS, swish=False).cpu()
    assert torch.equal(z, beta.view(1, c, 1, 1).expand(n, c, h, w))


@pytest.mark.parametrize("kind", ["0.1", "std 1e-3 around 1", "spike"])
def test_degenerate_groups_stay_inside_the_rule(hip_lib, kind):
    G.check(forward_figures(degenerate_input(kind).to(DEV)), "degenerate group: " + kind)
