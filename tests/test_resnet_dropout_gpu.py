"""`ddconfig.dropout` on the HIP path: the seeded ResnetBlock dropout inside the separate-pass GroupNorm (+ swish) kernels.

The mask is a pure function of (seed, element index, p) that odvae_amd/dropout_mask.py restates on the host, so the checks are exact:
the zero set IS the host mask's dropped set, kept values are the p = 0 kernel's times the scale bit for bit, and the backward of the
dropout form on dy is the p = 0 backward fed dy * keep * scale bit for bit.  "The p = 0 backward" there is the two-kernel form
(odvae_groupnorm_select_backward(0)): the dropout form never takes the read-once kernel, whose sums are added in another order.
Tolerances against float64 are those of the p = 0 tests of the same kernels: tests/test_ops_gpu.py (f32: forward 2e-4, dx 5e-4,
dgamma / dbeta 2e-3, relative to max(1, max|ref|)) and tests/test_bf16_gpu.py (bf16 outputs 1e-2, dgamma / dbeta 2e-3, relative to
max|ref|); module level: tests/test_modules_gpu.py (outputs 1e-3, gradients 3e-3 of max|ref|)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
YAML = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")
SEED = 0x1234_5678_9ABC_DEF1      # both key words in use

# N = 2: one channel per group with ragged tails / the f32 fallback branch (256 % (C / 4) != 0; the bf16 kernels take no such C) /
# several statistics chunks and the unrolled loops
SHAPES = [(32, 5, 7), (96, 4, 4), (128, 64, 64)]
CASES = [(dt, s) for dt in ("f32", "bf16") for s in SHAPES if not (dt == "bf16" and s[0] == 96)]
CASE_IDS = ["%s-c%d-%dx%d" % (dt, s[0], s[1], s[2]) for dt, s in CASES]
EXACT_P = {"f32": (0.1, 0.7), "bf16": (0.5, 0.75)}      # bf16: scales 2 and 4 commute with the rounding


def _dtype(dt):
    return BF if dt == "bf16" else torch.float32


def cl(t, dtype):
    return t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)


def rel_close(a, b, tol, what, floor=1.0):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    assert a.shape == b.shape and torch.isfinite(a).all(), what
    err, ref = (a - b).abs().max().item(), max(floor, b.abs().max().item())
    print("%s: max err %.3e of %.3e (tol %.1e)" % (what, err, ref, tol))
    assert err <= tol * ref, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, ref)


def tols(dt):
    """(forward, dx, dgamma / dbeta, floor of the reference's scale) of the p = 0 tests of the same kernels"""
    return (2e-4, 5e-4, 2e-3, 1.0) if dt == "f32" else (1e-2, 1e-2, 2e-3, 1e-6)


def keep_mask(p, n, c, h, w, seed=SEED):
    from odvae_amd import dropout_mask as dm
    return dm.resnet_dropout_keep(seed, p, n, c, h, w)      # CPU, logical NCHW, f32: 0 or scale


class _Problem:
    """One (dtype, shape): inputs, the p = 0 forward (y0, mean, rstd) and the float64 pre-dropout reference, made once."""

    def __init__(self, dt, shape, swish=True):
        c, h, w = shape
        self.dt, self.dtype, self.n, self.c, self.h, self.w, self.swish = dt, _dtype(dt), 2, c, h, w, swish
        g = torch.Generator().manual_seed(c + h)
        rnd = (lambda t: t.to(BF).float()) if dt == "bf16" else (lambda t: t)
        self.x = rnd(torch.randn(2, c, h, w, generator=g) * 1.5 + 0.3)
        self.gamma = 1 + 0.3 * torch.randn(c, generator=g)
        self.beta = 0.2 * torch.randn(c, generator=g)
        self.dy = rnd(torch.randn(2, c, h, w, generator=g))
        self.dskip = rnd(torch.randn(2, c, h, w, generator=g))
        self.xd, self.gd, self.bd = cl(self.x, self.dtype), self.gamma.to(DEV), self.beta.to(DEV)
        self.y0, self.mean, self.rstd = self.forward(None)

    # raw entry points: what the op layer calls, with the statistics handed back
    def forward(self, drop):
        from odvae_amd import lib
        L = lib.load()
        n, c, h, w = self.n, self.c, self.h, self.w
        y = torch.empty_like(self.xd)
        mean = torch.empty(n, 32, device=DEV)
        rstd = torch.empty(n, 32, device=DEV)
        sfx = "_bf16" if self.dt == "bf16" else "_f32"
        ws_fn = L.odvae_groupnorm_bf16_workspace_bytes if self.dt == "bf16" else L.odvae_groupnorm_workspace_bytes
        wp, wn = lib.workspace.get(ws_fn(n, h * w, c, 32), self.xd.device)
        head = (self.xd.data_ptr(), n, h * w, c, 32, self.gd.data_ptr(), self.bd.data_ptr(), 1e-6, int(self.swish))
        tail = (y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), wp, wn, lib.stream_ptr())
        if drop is None:
            lib.check(getattr(L, "odvae_groupnorm_fwd" + sfx)(*head, *tail), "fwd")
        else:
            lib.check(getattr(L, "odvae_groupnorm_fwd_drop" + sfx)(*head, float(drop[0]), int(drop[1]), *tail), "fwd_drop")
        return y, mean, rstd

    def backward(self, dy_dev, drop, dx_add=None):
        from odvae_amd import lib
        L = lib.load()
        n, c, h, w = self.n, self.c, self.h, self.w
        dx = torch.empty_like(self.xd)
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        sfx = "_bf16" if self.dt == "bf16" else "_f32"
        ws_fn = L.odvae_groupnorm_bf16_workspace_bytes if self.dt == "bf16" else L.odvae_groupnorm_workspace_bytes
        wp, wn = lib.workspace.get(ws_fn(n, h * w, c, 32), self.xd.device)
        head = (self.xd.data_ptr(), dy_dev.data_ptr(), n, h * w, c, 32, self.gd.data_ptr(), self.bd.data_ptr(), self.mean.data_ptr(),
                self.rstd.data_ptr(), int(self.swish))
        tail = (dx.data_ptr(), dg.data_ptr(), db.data_ptr(), lib.ptr(dx_add), wp, wn, lib.stream_ptr())
        if drop is None:
            prev = L.odvae_groupnorm_select_backward(0)      # the two-kernel form: the arithmetic the dropout form runs on dy_eff
            try:
                lib.check(getattr(L, "odvae_groupnorm_bwd" + sfx)(*head, *tail), "bwd")
            finally:
                L.odvae_groupnorm_select_backward(prev)
        else:
            lib.check(getattr(L, "odvae_groupnorm_bwd_drop" + sfx)(*head, float(drop[0]), int(drop[1]), *tail), "bwd_drop")
        return dx, dg, db

    def reference(self, mask, with_skip):
        """float64 autograd of mask * act(GroupNorm(x)) (+ the skip gradient): (y, dx, dgamma, dbeta)"""
        x, g, b = (t.double().clone().requires_grad_(True) for t in (self.x, self.gamma, self.beta))
        u = F.group_norm(x, 32, g, b, eps=1e-6)
        y = (u * torch.sigmoid(u) if self.swish else u) * mask.double()
        y.backward(self.dy.double())
        return y.detach(), x.grad + (self.dskip.double() if with_skip else 0.0), g.grad, b.grad


_PROBLEMS = {}


def problem(dt, shape, swish=True):
    key = (dt, shape, swish)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(dt, shape, swish)
    return _PROBLEMS[key]


def _check_forward(pr, p):
    mask = keep_mask(p, pr.n, pr.c, pr.h, pr.w)
    y, mean, rstd = pr.forward((p, SEED))
    assert torch.equal(mean, pr.mean) and torch.equal(rstd, pr.rstd)      # the statistics come before the dropout
    yc, y0c = y.float().cpu(), pr.y0.float().cpu()
    assert (y0c != 0).all()      # (so that a zero of y can only be a dropped element)
    assert torch.equal(yc == 0, mask == 0), "zero set != the host mask's dropped set (p=%g)" % p
    return mask, y, yc, y0c


@pytest.mark.parametrize("dt,shape", CASES, ids=CASE_IDS)
def test_forward_is_the_plain_output_times_the_host_mask_bit_for_bit(hip_lib, dt, shape):
    pr = problem(dt, shape)
    for p in EXACT_P[dt]:
        mask, y, yc, y0c = _check_forward(pr, p)
        if dt == "f32":
            want = pr.y0 * cl(mask, torch.float32)      # one f32 multiply on the device
        else:
            want = (pr.y0.float() * cl(mask, torch.float32)).to(BF)      # scale 2 / 4: exact, the rounding changes nothing
            assert torch.equal(want.float(), pr.y0.float() * cl(mask, torch.float32))
        assert torch.equal(y, want), "kept values != plain output * scale (p=%g)" % p
        ref = pr.reference(mask, False)[0]
        rel_close(y, ref, tols(dt)[0], "%s %s p=%g forward vs float64" % (dt, shape, p), tols(dt)[3])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != 96], ids=lambda s: "c%d-%dx%d" % s)
def test_forward_bf16_at_a_scale_that_does_not_commute_with_rounding(hip_lib, shape):
    """p = 0.1: scale = f32(1 / 0.9) is applied in f32 before the single rounding, so the plain bf16 output times the scale is NOT the
    expectation; a float64 restatement with the host mask is, at the tolerance tests/test_bf16_gpu.py holds the p = 0 kernel to."""
    pr = problem("bf16", shape)
    mask, y, _, _ = _check_forward(pr, 0.1)
    rel_close(y, pr.reference(mask, False)[0], 1e-2, "bf16 %s p=0.1 forward vs float64" % (shape,), 1e-6)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_plain_form_without_swish(hip_lib, dt):
    pr = problem(dt, (32, 5, 7), swish=False)
    p = EXACT_P[dt][0]
    mask, y, _, _ = _check_forward(pr, p)
    assert torch.equal(y.float(), pr.y0.float() * cl(mask, torch.float32)) if dt == "f32" else torch.equal(y, (pr.y0.float() * cl(mask, torch.float32)).to(BF))
    dyd = cl(pr.dy, pr.dtype)
    got = pr.backward(dyd, (p, SEED))
    want = pr.backward((dyd.float() * cl(mask, torch.float32)).to(pr.dtype), None)
    for a, b, what in zip(got, want, ("dx", "dgamma", "dbeta")):
        assert torch.equal(a, b), what
    ref = pr.reference(mask, False)
    for a, b, tol, what in zip(got, ref[1:], tols(dt)[1:3] + tols(dt)[2:3], ("dx", "dgamma", "dbeta")):
        rel_close(a, b, tol, "%s identity %s vs float64" % (dt, what), tols(dt)[3])


@pytest.mark.parametrize("with_skip", [False, True], ids=["no-skip", "dx_add"])
@pytest.mark.parametrize("dt,shape", CASES, ids=CASE_IDS)
def test_backward_is_the_plain_backward_on_the_masked_gradient_bit_for_bit(hip_lib, dt, shape, with_skip):
    """dx, dgamma, dbeta of the dropout form on dy == the two-kernel p = 0 backward fed dy * keep * scale (f32: the product made in f32 on
    the device, any p; bf16: p = 0.5 / 0.75, where the product is exact in bf16), and both against float64 autograd of
    mask * swish(GroupNorm(x)), with and without the folded skip gradient."""
    pr = problem(dt, shape)
    dyd = cl(pr.dy, pr.dtype)
    add = cl(pr.dskip, pr.dtype) if with_skip else None
    for p in EXACT_P[dt]:
        mask = keep_mask(p, pr.n, pr.c, pr.h, pr.w)
        got = pr.backward(dyd, (p, SEED), add)
        dy_eff = dyd * cl(mask, torch.float32) if dt == "f32" else (dyd.float() * cl(mask, torch.float32)).to(BF)
        want = pr.backward(dy_eff, None, add)
        for a, b, what in zip(got, want, ("dx", "dgamma", "dbeta")):
            assert torch.equal(a, b), "%s of the dropout form != plain backward on dy * keep * scale (p=%g)" % (what, p)
        ref = pr.reference(mask, with_skip)
        for a, b, tol, what in zip(got, ref[1:], tols(dt)[1:3] + tols(dt)[2:3], ("dx", "dgamma", "dbeta")):
            rel_close(a, b, tol, "%s %s p=%g %s vs float64" % (dt, shape, p, what), tols(dt)[3])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != 96], ids=lambda s: "c%d-%dx%d" % s)
def test_backward_bf16_p01_against_float64(hip_lib, shape):
    pr = problem("bf16", shape)
    mask = keep_mask(0.1, pr.n, pr.c, pr.h, pr.w)
    got = pr.backward(cl(pr.dy, BF), (0.1, SEED), cl(pr.dskip, BF))
    for a, b, tol, what in zip(got, pr.reference(mask, True)[1:], (1e-2, 2e-3, 2e-3), ("dx", "dgamma", "dbeta")):
        rel_close(a, b, tol, "bf16 %s p=0.1 %s vs float64" % (shape, what), 1e-6)


@pytest.mark.parametrize("dt,shape", CASES, ids=CASE_IDS)
def test_p_one_gives_exact_finite_zeros(hip_lib, dt, shape):
    pr = problem(dt, shape)
    y, _, _ = pr.forward((1.0, SEED))
    dx, dg, db = pr.backward(cl(pr.dy, pr.dtype), (1.0, SEED))
    for t, what in ((y, "y"), (dx, "dx"), (dg, "dgamma"), (db, "dbeta")):
        assert torch.isfinite(t.float()).all() and (t.float() == 0).all(), what


def test_entry_points_check_their_arguments(hip_lib):
    from odvae_amd import lib
    pr = problem("f32", (32, 5, 7))
    for bad in (-0.25, 1.5, float("nan")):
        with pytest.raises(lib.HipLibraryError, match="between 0 and 1"):
            pr.forward((bad, SEED))
        with pytest.raises(lib.HipLibraryError, match="between 0 and 1"):
            pr.backward(cl(pr.dy, torch.float32), (bad, SEED))
    prb = problem("bf16", (32, 5, 7))
    with pytest.raises(lib.HipLibraryError, match="between 0 and 1"):
        prb.forward((2.0, SEED))
    # C % 8: C = 4 * 33 passes the f32 GroupNorm's own shape check (C % 4, C % G) and has no octets
    L, c = lib.load(), 132
    x = torch.zeros(1, 4, 4, c, device=DEV)
    v = torch.zeros(c, device=DEV)
    st = torch.zeros(1, 33, device=DEV)
    rc = L.odvae_groupnorm_apply_drop_f32(x.data_ptr(), 1, 16, c, 33, v.data_ptr(), v.data_ptr(), st.data_ptr(), st.data_ptr(), 1, 0.5, 1,
                                          x.data_ptr(), lib.stream_ptr())
    assert rc == 1 and b"C % 8" in L.odvae_last_error()


# ---- statistics from the producing conv's epilogue ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_statistics_from_the_conv_epilogue_feed_the_dropout_form(hip_lib, monkeypatch, dt):
    """conv3x3(gn_stats=True) -> group_norm(drop_p): the fwd_partials dropout form.  Same statistics as its p = 0 twin (kept values = that
    twin's output times the scale, bit for bit, at p = 0.5), and against the statistics-pass dropout form: the same bits where the p = 0
    forms agree bit for bit, their tolerance (tests/test_ops_gpu.py 2e-5, tests/test_bf16_gpu.py 8e-3, of max|ref|) elsewhere."""
    from odvae_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    monkeypatch.setattr(ops, "GN_FUSED_STATS", True)
    dtype = _dtype(dt)
    n, cin, cout, h, w = (2, 64, 128, 16, 32) if dt == "f32" else (2, 64, 128, 16, 16)
    g = torch.Generator().manual_seed(n + cin + cout + h)
    x = cl(torch.randn(n, cin, h, w, generator=g), dtype)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV) * 0.1
    gamma, beta = torch.randn(cout, generator=g).to(DEV), torch.randn(cout, generator=g).to(DEV)
    y = ops.conv3x3(x, wt, b, None, gn_stats=True)
    assert ops._gn_partials_of(y, 32) is not None
    y_plain = y.clone(memory_format=torch.preserve_format)      # a copy carries no statistics: the statistics pass runs
    assert ops._gn_partials_of(y_plain, 32) is None
    p = 0.5
    mask = cl(keep_mask(p, n, cout, h, w), torch.float32)
    z0_part, z0_pass = ops.group_norm(y, gamma, beta, 32, 1e-6, True), ops.group_norm(y_plain, gamma, beta, 32, 1e-6, True)
    zd_part = ops.group_norm(y, gamma, beta, 32, 1e-6, True, drop_p=p, drop_seed=SEED)
    zd_pass = ops.group_norm(y_plain, gamma, beta, 32, 1e-6, True, drop_p=p, drop_seed=SEED)
    assert torch.equal(zd_part.float(), z0_part.float() * mask)
    assert torch.equal(zd_pass.float(), z0_pass.float() * mask)
    same = torch.equal(z0_part, z0_pass)
    print("%s: p = 0 forms agree bit for bit: %s" % (dt, same))
    if same:
        assert torch.equal(zd_part, zd_pass)
    tol = 2e-5 if dt == "f32" else 8e-3
    assert (zd_part.float() - zd_pass.float()).abs().max().item() <= tol * zd_pass.float().abs().max().item()


# ---- the fused backward forms are bypassed -------------------------------------------------------------------------------------------------
def test_dropout_bypasses_the_fused_backward_forms(hip_lib, monkeypatch):
    """GN_FUSED_BWD_HITS counts GroupNorm backwards that took their sums from the conv data gradient's epilogue.  At 64 ch, 16x32 (the
    F(4x4) route) a swish-GroupNorm in front of a conv moves it at p = 0 and does not with dropout; across a ResnetBlock backward the
    count moves by 2 at p = 0 (norm1, norm2) and by norm1's 1 alone with dropout -- norm2, the dropped norm, never takes the form."""
    from odvae_amd import modules, ops
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    monkeypatch.setattr(ops, "GN_FUSED_BWD", True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 32, generator=g)
    wt = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).to(DEV)
    gamma, beta = torch.randn(64, generator=g).to(DEV), torch.randn(64, generator=g).to(DEV)
    moved = {}
    for p in (0.0, 0.3):
        xd = cl(x, torch.float32).requires_grad_(True)
        hits = ops.GN_FUSED_BWD_HITS
        a = ops.group_norm(xd, gamma, beta, 32, 1e-6, True, drop_p=p, drop_seed=SEED)
        assert (getattr(a, "_gn_bwd_link", None) is not None) == (p == 0.0)
        ops.conv3x3(a, wt, None, None).sum().backward()
        moved[p] = ops.GN_FUSED_BWD_HITS - hits
    assert moved == {0.0: 1, 0.3: 0}, moved
    torch.manual_seed(5)
    block = modules.ResnetBlock(in_channels=64, out_channels=64, dropout=0.3, temb_channels=0).to(DEV).train()
    moved = {}
    for mode in ("eval", "train"):
        getattr(block, mode)()
        xd = cl(x, torch.float32).requires_grad_(True)
        hits = ops.GN_FUSED_BWD_HITS
        block(xd).sum().backward()
        moved[mode] = ops.GN_FUSED_BWD_HITS - hits
    assert moved == {"eval": 2, "train": 1}, moved


# ---- module level ----------------------------------------------------------------------------------------------------------------------
class _HostMask(torch.nn.Module):
    """Stands in for the oracle block's nn.Dropout: multiplies by the mask the HIP block used."""

    def __init__(self, keep):
        super().__init__()
        self.keep = keep

    def forward(self, x):
        return x * self.keep


def _grads(block):
    return {k: v.grad.detach().clone() for k, v in block.named_parameters()}


@pytest.mark.parametrize("h,w", [(8, 8), (16, 32)], ids=["8x8", "16x32-F(4x4)"])
def test_resnet_block_matches_the_oracle_with_the_host_mask(hip_lib, monkeypatch, h, w):
    from odvae_amd import dropout_mask as dm, modules, ops
    from oracle import ldm_model
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    torch.manual_seed(23)
    ref = ldm_model.ResnetBlock(in_channels=64, out_channels=128, dropout=0.3, temb_channels=0).train()
    net = modules.ResnetBlock(in_channels=64, out_channels=128, dropout=0.3, temb_channels=0)
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, h, w, generator=g)
    gy = torch.randn(2, 128, h, w, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    y.backward(gy.to(DEV))
    assert net.last_dropout_seed is not None
    ref.dropout = _HostMask(dm.resnet_dropout_keep(net.last_dropout_seed, 0.3, 2, 128, h, w))
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr, None)
    y_ref.backward(gy)
    rel_close(y, y_ref, 1e-3, "block output", 1e-12)
    rel_close(xd.grad, xr.grad, 3e-3, "block input gradient", 1e-12)
    refp = dict(ref.named_parameters())
    scale = max(p.grad.abs().max().item() for p in refp.values())
    for name, p in net.named_parameters():
        rel_close(p.grad, refp[name].grad, 3e-3, "block d" + name, 1e-3 * scale)


def test_eval_mode_is_the_dropout_free_block(hip_lib):
    from odvae_amd import modules
    torch.manual_seed(4)
    drop = modules.ResnetBlock(in_channels=64, out_channels=128, dropout=0.3, temb_channels=0).to(DEV).eval()
    plain = modules.ResnetBlock(in_channels=64, out_channels=128, dropout=0.0, temb_channels=0).to(DEV).eval()
    plain.load_state_dict(drop.state_dict())
    g = torch.Generator().manual_seed(2)
    x, gy = torch.randn(2, 64, 8, 8, generator=g), torch.randn(2, 128, 8, 8, generator=g).to(DEV)
    outs = []
    state = torch.get_rng_state()
    for blk in (drop, plain):
        xd = x.to(DEV).requires_grad_(True)
        y = blk(xd)
        y.backward(gy)
        outs.append((y.detach(), xd.grad, _grads(blk)))
    assert torch.equal(torch.get_rng_state(), state) and drop.last_dropout_seed is None      # no seed is drawn in eval mode
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for k in outs[0][2]:
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k


def test_manual_seed_reproduces_a_run(hip_lib):
    from odvae_amd import modules
    torch.manual_seed(4)
    blk = modules.ResnetBlock(in_channels=64, out_channels=64, dropout=0.3, temb_channels=0).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    x, gy = torch.randn(2, 64, 8, 8, generator=g), torch.randn(2, 64, 8, 8, generator=g).to(DEV)

    def run(k):
        torch.manual_seed(k)
        blk.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        y = blk(xd)
        y.backward(gy)
        return y.detach(), xd.grad, _grads(blk), blk.last_dropout_seed

    a, b, c = run(11), run(11), run(12)
    assert a[3] == b[3] != c[3]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert not torch.equal(a[0], c[0])      # another seed, another zero set behind conv2


DD = dict(double_z=True, z_channels=16, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2, 4],
          num_res_blocks=2, attn_resolutions=[16], dropout=0.3)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_decoder_checkpoint_policies_redraw_the_same_masks(hip_lib, precision):
    """Decoder (ch = 32 geometry of tests/test_modules_gpu.py, dropout 0.3) without checkpointing, with "unit" (torch.utils.checkpoint restores
    the CPU generator for the recompute, which draws the same seeds in the same order) and with "norm" (the re-make carries (p, seed)): after
    torch.manual_seed(k) output and every gradient are bit-identical, as tests/test_model_gpu.py requires of the policies at p = 0."""
    from odvae_amd import modules
    torch.manual_seed(23)
    nets = {pol: modules.Decoder(activation_checkpoint=pol, **DD) for pol in (False, "unit", "norm")}
    for pol, net in nets.items():
        net.load_state_dict(nets[False].state_dict())
        net.to(DEV).train()
        if precision == "bf16":
            net.compute_dtype = BF
    g = torch.Generator().manual_seed(1)
    z, gy = torch.randn(2, 16, 4, 4, generator=g), torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    outs = {}
    for pol, net in nets.items():
        torch.manual_seed(77)
        zd = z.to(DEV).requires_grad_(True)
        y = net(zd)
        seeds = [m.last_dropout_seed for m in net.modules() if isinstance(m, modules.ResnetBlock)]
        y.backward(gy)
        assert seeds == [m.last_dropout_seed for m in net.modules() if isinstance(m, modules.ResnetBlock)]      # a recompute re-drew the same
        outs[pol] = (y.detach(), zd.grad, _grads(net), seeds)
    base = outs[False]
    assert len(set(base[3])) == len(base[3]) and None not in base[3]      # every block drew its own seed
    assert base[1].abs().max().item() > 0
    for pol in ("unit", "norm"):
        o = outs[pol]
        assert o[3] == base[3], pol
        assert torch.equal(o[0], base[0]), pol
        assert torch.equal(o[1], base[1]), pol
        for k in base[2]:
            assert torch.equal(o[2][k], base[2][k]), (pol, k)


def test_one_trainer_step_with_ddconfig_dropout(hip_lib, tmp_path):
    """The yaml-shaped model (ch = 32, 64 x 64) with ddconfig.dropout: 0.1: a training step gives a finite loss and finite gradients
    everywhere, validation runs with the dropout inactive (the numbers of the dropout-free model on the same weights, no seed drawn), and a
    checkpoint round trip keeps the state_dict keys."""
    from odvae_amd import modules, synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer

    def build(dropout):
        torch.manual_seed(23)
        mcfg, cfg = synthetic.model_config(YAML, latent_hw=4, ch=32)
        mcfg.params.ddconfig["dropout"] = dropout
        m = instantiate_from_config(mcfg)
        m.learning_rate = 12 * cfg.model.base_learning_rate
        return m.to(DEV)

    model, plain = build(0.1), build(0.0)
    plain.load_state_dict(model.state_dict(), strict=True)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    blocks = [m for m in model.modules() if isinstance(m, modules.ResnetBlock)]
    assert blocks and all(b.dropout.p == 0.1 for b in blocks)
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    fresh = lambda: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    # gradients of one training step (no optimizer yet: the weights stay those of `plain`)
    model.train()
    model._global_step = plain._global_step = 1      # past the first step: the reconstruction and KL terms are in the total
    model.injected_noise = plain.injected_noise = noise
    loss = model.training_step(fresh(), 0, 0)
    loss.backward()
    assert torch.isfinite(loss).item()
    seeds = [b.last_dropout_seed for b in blocks]
    assert None not in seeds and len(set(seeds)) == len(seeds)
    got = 0
    for name, p in model.named_parameters():
        if p.grad is not None:
            got += 1
            assert torch.isfinite(p.grad).all(), name
    assert got > 100 and model.decoder.conv_in.weight.grad.abs().max().item() > 0
    model.zero_grad(set_to_none=True)
    # validation: eval mode, no seed drawn, the dropout-free model's numbers on the same weights
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
    vals = [trainer.validate([fresh()]), Trainer(plain, gradient_clip_val=1.0, optimizer_indices=(0,)).validate([fresh()])]
    assert [b.last_dropout_seed for b in blocks] == seeds and model.training
    assert vals[0].keys() == vals[1].keys() and "val/rec_loss" in vals[0]
    for k in vals[0]:
        a, b = float(vals[0][k]), float(vals[1][k])
        assert a == b or (math.isnan(a) and math.isnan(b)), k
    # one trainer step, then the checkpoint round trip
    out = trainer.training_batch(fresh(), 0)[0]
    assert math.isfinite(out.item())
    assert [b.last_dropout_seed for b in blocks] != seeds
    path = trainer.save_checkpoint(os.path.join(tmp_path, "drop.ckpt"))
    sd = torch.load(path, map_location="cpu")["state_dict"]
    assert list(sd.keys()) == list(plain.state_dict().keys())
    again = build(0.1)
    Trainer(again, gradient_clip_val=1.0, optimizer_indices=(0,)).load_checkpoint(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
