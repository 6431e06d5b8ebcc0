"""The conv-less resamplers and the decoder's tanh on the device, through ops (odvae_avgpool2x2_* / odvae_upsample2x_* / odvae_tanh_*):
values against float64 on the host, the GroupNorm statistics they leave for the Normalize that reads them next, and that consumer.

Bounds (u = 2^-24; derived, not measured):
  f32 average pool   y = 0.25 ((a + b) + (c + d)): every input passes two f32 additions, the scaling by 0.25 is exact:
                     |y - exact| <= 2u (1 + u) avgpool(|x|) <= 4u avgpool(|x|) elementwise
  bf16 average pool  the f32 sum of four bf16 values is exact up to u, then ONE rounding: within one bf16 ulp of the rounded float64 result
  integer inputs     |x| <= 64: every sum is an integer <= 256 and every quarter of it has <= 8 significant bits: bit-exact in both formats
  nearest upsample   a copy: torch.equal
  pool backward      0.25 dy is exact in both formats: torch.equal, with exact zeros in a dropped row / column
  upsample backward  the 2x2 sum: 4u sumpool(|dy|) (f32), one bf16 ulp of the rounded float64 sum (bf16)
  partials           2e-5 max|want| -- what tests/test_ops_gpu.py holds the conv epilogue's partials to
  consumer           tagged against untagged 2e-5 max|ref|, against torch on the host 5e-4 (tests/test_ops_gpu.py's rules for the conv);
                     bf16 outputs: a last-bit difference of the statistics can flip one rounding, 2^-7 |ref| elementwise on top of that
                     (seen: one flipped rounding, dx 2.9e-4 of max|ref| at (2,128,36,68); every other bf16 output identical or within 3e-7; profiles/resample.md); against float64 GroupNorm + swish of the
                     stored bf16 y on the host: the f32 rule above for the arithmetic plus the ONE rounding on the way out,
                     5e-4 max|ref| + one bf16 ulp of the reference elementwise
  tanh               no bound fixed in advance: 4x the worst deviation from float64 MEASURED on these inputs (profiles/resample.md):
                     forward 6.1e-8 (seen 6.013e-8 on the flat array, 4.534e-8 on (2,3,5,7)), backward 6.8e-8 (seen 6.779e-8, 5.450e-8);
                     absolute, |dy| <= 1"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32_SHAPES = [(2, 32, 4, 4), (1, 64, 7, 10), (3, 128, 34, 66), (1, 96, 6, 6), (2, 4, 5, 3)]
BF16_SHAPES = [(2, 32, 4, 4), (1, 64, 7, 10), (2, 128, 18, 34), (1, 8, 3, 5)]
CASES = [(torch.float32, s) for s in F32_SHAPES] + [(torch.bfloat16, s) for s in BF16_SHAPES]
IDS = ["%s-%dx%dx%dx%d" % (("f32" if d == torch.float32 else "bf16",) + s) for d, s in CASES]
TANH_FWD_TOL = 4 * 6.1e-8
TANH_BWD_TOL = 4 * 6.8e-8


def dev():
    return torch.device("cuda:0")


def stats_ok(c):
    cpg = c // 32
    return c % 32 == 0 and 1 <= cpg <= 32 and (cpg & (cpg - 1)) == 0


def to_dev(t, dtype):
    return t.to(dtype).to(dev()).contiguous(memory_format=torch.channels_last)


def host(t):
    return t.detach().float().cpu().double()


def bf16_ulp(v):
    """One unit in the last place of the bf16 number format at |v| (8 significant bits); the smallest normal's below that."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126).float())
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 8).double())


def make_input(dtype, shape, integer=False, seed=0):
    g = torch.Generator().manual_seed(sum(shape) + seed)
    if integer:
        x = torch.randint(-64, 65, shape, generator=g).float()
    else:
        x = torch.randn(shape, generator=g) * 1.5 + 0.25
    return x.to(dtype).float()      # what the device holds, as f32 on the host


def chunks_of(L, dtype, h, w):
    return L.odvae_conv_bf16_stats_chunks(h, w) if dtype == torch.bfloat16 else L.odvae_conv3x3_wino4_stats_chunks(h, w)


def check_pool_values(got, x, dtype, integer):
    want = F.avg_pool2d(x.double(), 2, 2)
    got = host(got)
    assert got.shape == want.shape
    if integer:
        assert torch.equal(got, want)
    elif dtype == torch.float32:
        excess = ((got - want).abs() - 4 * U * F.avg_pool2d(x.abs().double(), 2, 2)).max().item()
        assert excess <= 0.0, excess
    else:
        ref = want.to(torch.bfloat16).double()
        excess = ((got - ref).abs() - bf16_ulp(ref)).max().item()
        assert excess <= 0.0, excess


def check_partials(ops, L, y, dtype):
    n, c, ho, wo = y.shape
    part = ops._gn_partials_of(y, 32)
    if not stats_ok(c):
        assert part is None and getattr(y, "_gn_partials", None) is None
        return
    assert part is not None
    assert tuple(part.shape) == (n, chunks_of(L, dtype, ho, wo), 32, 2)
    yc = host(y).reshape(n, 32, c // 32, ho * wo)
    want = torch.stack([yc.sum(dim=(2, 3)), (yc * yc).sum(dim=(2, 3))], dim=-1)
    got = part.double().cpu().sum(dim=1)
    err = (got - want).abs().max().item()
    print("partials %s: %.3e of max|want|" % (tuple(y.shape), err / want.abs().max().item()))
    assert err <= 2e-5 * want.abs().max().item()
    assert ops._gn_partials_of(y.clone(), 32) is None
    y.mul_(1.0)      # an in-place write: the statistics no longer describe "this tensor, as it is now"
    assert ops._gn_partials_of(y, 32) is None


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_avg_pool_forward_and_partials(hip_lib, monkeypatch, dtype, shape):
    from odvae_amd import ops
    for integer in (False, True):
        x = make_input(dtype, shape, integer)
        y = ops.avg_pool2x2(to_dev(x, dtype), gn_stats=True)
        assert y.dtype == dtype and tuple(y.shape) == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
        check_pool_values(y, x, dtype, integer)
        plain = ops.avg_pool2x2(to_dev(x, dtype))
        assert getattr(plain, "_gn_partials", None) is None and torch.equal(plain, y)
        monkeypatch.setattr(ops, "GN_FUSED_STATS", False)
        off = ops.avg_pool2x2(to_dev(x, dtype), gn_stats=True)
        monkeypatch.setattr(ops, "GN_FUSED_STATS", True)
        assert getattr(off, "_gn_partials", None) is None and torch.equal(off, y)
        check_partials(ops, hip_lib, y, dtype)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_upsample_forward_and_partials(hip_lib, monkeypatch, dtype, shape):
    from odvae_amd import ops
    x = make_input(dtype, shape)
    y = ops.upsample2x(to_dev(x, dtype), gn_stats=True)
    assert y.dtype == dtype
    assert torch.equal(y.float().cpu(), F.interpolate(x, scale_factor=2.0, mode="nearest"))
    plain = ops.upsample2x(to_dev(x, dtype))
    assert getattr(plain, "_gn_partials", None) is None and torch.equal(plain, y)
    monkeypatch.setattr(ops, "GN_FUSED_STATS", False)
    off = ops.upsample2x(to_dev(x, dtype), gn_stats=True)
    monkeypatch.setattr(ops, "GN_FUSED_STATS", True)
    assert getattr(off, "_gn_partials", None) is None and torch.equal(off, y)
    check_partials(ops, hip_lib, y, dtype)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_avg_pool_backward_is_exact_with_zeros_in_the_dropped_edge(hip_lib, dtype, shape):
    from odvae_amd import ops
    n, c, h, w = shape
    x = make_input(dtype, shape)
    gy = make_input(dtype, (n, c, h // 2, w // 2), seed=1)
    xd = to_dev(x, dtype).requires_grad_(True)
    y = ops.avg_pool2x2(xd, gn_stats=True)
    gyd = to_dev(gy, dtype)
    torch.cuda.synchronize()
    stale = torch.full((n, h, w, c), float("nan"), dtype=dtype, device=dev())      # the block the backward's torch.empty gets next
    torch.cuda.synchronize()
    del stale
    y.backward(gyd)
    want = torch.zeros(n, c, h, w, dtype=torch.float64)
    want[:, :, :2 * (h // 2), :2 * (w // 2)] = F.interpolate(0.25 * gy.double(), scale_factor=2.0, mode="nearest")
    assert xd.grad.dtype == dtype and torch.equal(host(xd.grad), want)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_upsample_backward_is_the_2x2_sum(hip_lib, dtype, shape):
    from odvae_amd import ops
    n, c, h, w = shape
    x = make_input(dtype, shape)
    gy = make_input(dtype, (n, c, 2 * h, 2 * w), seed=1)
    xd = to_dev(x, dtype).requires_grad_(True)
    ops.upsample2x(xd, gn_stats=True).backward(to_dev(gy, dtype))
    want = 4.0 * F.avg_pool2d(gy.double(), 2, 2)
    got = host(xd.grad)
    if dtype == torch.float32:
        excess = ((got - want).abs() - 4 * U * 4.0 * F.avg_pool2d(gy.abs().double(), 2, 2)).max().item()
    else:
        ref = want.to(torch.bfloat16).double()
        excess = ((got - ref).abs() - bf16_ulp(ref)).max().item()
    assert xd.grad.dtype == dtype and excess <= 0.0, excess


def _consumer(ops, make_y, c, dtype, seed):
    """group_norm_skip(swish) on the resampler's tagged output against the same call on its clone (statistics pass) and torch on the host."""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    outs = []
    for tagged in (True, False):
        gd, bd = gamma.to(dev()).requires_grad_(True), beta.to(dev()).requires_grad_(True)
        y, leaf = make_y()
        assert ops._gn_partials_of(y, 32) is not None
        y.retain_grad()      # the GroupNorm's own dx (with the folded skip gradient); the resamplers' backward passes have tests of their own
        yin = y if tagged else y.clone()
        assert (ops._gn_partials_of(yin, 32) is not None) == tagged
        z, skip = ops.group_norm_skip(yin, gd, bd, 32, 1e-6, swish=True)
        gz = make_input(dtype, tuple(z.shape), seed=seed + 1)
        gs = make_input(dtype, tuple(z.shape), seed=seed + 2)
        torch.autograd.backward([z, skip], [to_dev(gz, dtype), to_dev(gs, dtype)])
        assert leaf.grad is not None and torch.isfinite(leaf.grad).all()
        outs.append((z.detach(), y.grad, gd.grad, bd.grad, y.detach()))
    assert torch.equal(outs[0][4], outs[1][4])
    yh = host(outs[0][4])
    ref = F.silu(F.group_norm(yh, 32, gamma.double(), beta.double(), eps=1e-6))
    for a, b, what in zip(outs[0][:4], outs[1][:4], ("z", "dx", "dgamma", "dbeta")):
        a, b = host(a), host(b)
        slack = 2.0 ** -7 * b.abs() if (dtype == torch.bfloat16 and what in ("z", "dx")) else 0.0
        excess = ((a - b).abs() - slack).max().item()
        print("consumer %s %s: tagged vs untagged %.3e of max|ref|" % (tuple(yh.shape), what, (a - b).abs().max().item() / b.abs().max().item()))
        assert excess <= 2e-5 * b.abs().max().item(), what
    err = (host(outs[0][0]) - ref).abs()
    print("consumer %s: vs torch %.3e of max|ref|" % (tuple(yh.shape), err.max().item() / ref.abs().max().item()))
    if dtype == torch.float32:
        assert err.max().item() <= 5e-4 * ref.abs().max().item()
    else:
        over = (err - bf16_ulp(ref)).max().item()
        print("consumer %s: vs torch beyond one bf16 ulp %.3e of max|ref|" % (tuple(yh.shape), max(over, 0.0) / ref.abs().max().item()))
        assert over <= 5e-4 * ref.abs().max().item()


@pytest.mark.parametrize("dtype,shape", [c for c in CASES if stats_ok(c[1][1])], ids=[i for i, c in zip(IDS, CASES) if stats_ok(c[1][1])])
@pytest.mark.parametrize("op", ["avg_pool2x2", "upsample2x"])
def test_group_norm_reads_the_resamplers_statistics(hip_lib, op, dtype, shape):
    from odvae_amd import ops
    x = make_input(dtype, shape)

    def make_y():
        leaf = to_dev(x, dtype).requires_grad_(True)
        return getattr(ops, op)(leaf, gn_stats=True), leaf
    _consumer(ops, make_y, shape[1], dtype, seed=7)


@pytest.mark.parametrize("op,shape", [("avg_pool2x2", (1, 64, 16, 16)), ("upsample2x", (1, 64, 4, 4))])
def test_group_norm_on_an_offset_resampler_output(hip_lib, op, shape):
    """Mean = 100 std per group in the (1, 64, 8, 8) result: E[x^2] - E[x]^2 from f32 partials is useless there; the finalize kernel's
    recentring (gn_finalize.h) takes centred sums from the tensor itself, whoever made the partials."""
    from odvae_amd import ops
    g = torch.Generator().manual_seed(11)
    std = torch.rand(1, 32, 1, 1, generator=g) + 0.5
    x = (torch.randn(1, 32, 2, *shape[2:], generator=g) * std.unsqueeze(2) + 100.0 * std.unsqueeze(2)).reshape(shape)

    def make_y():
        leaf = to_dev(x, torch.float32).requires_grad_(True)
        return getattr(ops, op)(leaf, gn_stats=True), leaf
    before = hip_lib.odvae_groupnorm_recentred(0)
    _consumer(ops, make_y, 64, torch.float32, seed=13)
    assert hip_lib.odvae_groupnorm_recentred(0) > before


def test_resampler_entry_points_validate_their_arguments(hip_lib):
    from odvae_amd import lib
    L = hip_lib
    x = torch.zeros(1, 4, 4, 8, device=dev())
    y = torch.zeros(1, 8, 8, 8, device=dev())
    p = torch.zeros(1, 1, 2, 2, device=dev())
    s = lib.stream_ptr()
    assert L.odvae_avgpool2x2_f32(x.data_ptr(), y.data_ptr(), 1, 4, 4, 6, None, 0, 0, s) != 0 and b"C % 4" in L.odvae_last_error()
    assert L.odvae_avgpool2x2_f32(None, y.data_ptr(), 1, 4, 4, 8, None, 0, 0, s) != 0
    assert L.odvae_avgpool2x2_f32(x.data_ptr(), y.data_ptr(), 1, 1, 4, 8, None, 0, 0, s) != 0           # nothing to pool
    assert L.odvae_avgpool2x2_f32(x.data_ptr(), y.data_ptr(), 1, 4, 4, 8, p.data_ptr(), 3, 1, s) != 0   # 3 groups do not divide 8 channels
    assert L.odvae_avgpool2x2_f32(x.data_ptr(), y.data_ptr(), 1, 4, 4, 8, p.data_ptr(), 2, 0, s) != 0   # statistics need chunks > 0
    assert L.odvae_avgpool2x2_f32(x.data_ptr() + 4, y.data_ptr(), 1, 4, 4, 4, None, 0, 0, s) != 0       # 16-byte alignment
    assert L.odvae_avgpool2x2_bf16(x.data_ptr(), y.data_ptr(), 1, 4, 4, 12, None, 0, 0, s) != 0 and b"C % 8" in L.odvae_last_error()
    assert L.odvae_avgpool2x2_bwd_f32(x.data_ptr(), y.data_ptr(), 1, 4, 4, 2052, s) != 0
    assert L.odvae_upsample2x_f32(x.data_ptr(), y.data_ptr(), 0, 4, 4, 8, None, 0, 0, s) != 0
    assert L.odvae_upsample2x_bf16(x.data_ptr(), None, 1, 4, 4, 8, None, 0, 0, s) != 0
    assert L.odvae_tanh_f32(x.data_ptr(), y.data_ptr(), 0, s) != 0
    assert L.odvae_tanh_bwd_f32(x.data_ptr(), None, y.data_ptr(), 4, s) != 0
    # statistics with several chunks and more chunks than pixels: every slot written (zeros for the empty runs)
    xs = torch.ones(1, 4, 4, 8, device=dev())
    ys = torch.empty(1, 2, 2, 8, device=dev())
    part = torch.full((1, 7, 2, 2), float("nan"), device=dev())
    assert L.odvae_avgpool2x2_f32(xs.data_ptr(), ys.data_ptr(), 1, 4, 4, 8, part.data_ptr(), 2, 7, s) == 0
    assert torch.equal(ys.cpu(), torch.ones(1, 2, 2, 8))
    got = part.cpu()
    assert torch.isfinite(got).all() and torch.equal(got.sum(dim=1), torch.full((1, 2, 2), 16.0))
    assert int((got[0, :, 0, 0] == 0).sum()) == 3      # four pixels in seven runs


@pytest.mark.parametrize("shape,unaligned", [((2, 3, 5, 7), False), ((1031,), False), ((1031,), True)], ids=["2x3x5x7", "flat-1031", "flat-1031-unaligned"])
def test_tanh_forward_and_backward(hip_lib, shape, unaligned):
    """unaligned: the same 1031 values and gradients one float past a 16-byte boundary -- the kernels' scalar form (no float4 body)."""
    from odvae_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g) * 2.0
    special = torch.tensor([0.0, 1e-4, -1e-4, 8.0, -8.0, 20.0, -20.0])
    x.view(-1)[:7] = special
    gy = torch.rand(shape, generator=g) * 2.0 - 1.0
    xd = x.to(dev())
    if len(shape) == 4:
        xd = xd.contiguous(memory_format=torch.channels_last)      # the layout conv_out hands over
    gyd = gy.to(dev())
    if unaligned:
        xd, gyd = torch.cat([xd.new_zeros(1), xd])[1:], torch.cat([gyd.new_zeros(1), gyd])[1:]
        assert xd.data_ptr() % 16 == 4 and gyd.data_ptr() % 16 == 4 and xd.is_contiguous()
    xd.requires_grad_(True)
    y = ops.tanh(xd)
    y.backward(gyd)
    want = torch.tanh(x.double())
    fwd = (host(y) - want).abs().max().item()
    bwd = (host(xd.grad) - gy.double() * (1.0 - want * want)).abs().max().item()
    print("tanh %s: forward %.3e backward %.3e (absolute, against float64)" % (shape, fwd, bwd))
    assert y.shape == x.shape and y.stride() == xd.stride()
    sat, gsat = y.detach().cpu().reshape(-1)[5:7], xd.grad.cpu().reshape(-1)[5:7]      # (reshape: logical order, whatever the layout)
    assert torch.equal(sat, torch.tensor([1.0, -1.0])) and torch.equal(gsat, torch.zeros(2))      # saturated: exactly +-1, zero gradient
    assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all()
    assert y.detach().cpu().reshape(-1)[0].item() == 0.0
    assert fwd <= TANH_FWD_TOL and bwd <= TANH_BWD_TOL, (fwd, bwd)
