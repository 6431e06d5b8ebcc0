"""The linear-attention kernels (csrc/linattn_f32.hip) through the C ABI, and ops.linear_attention_qkv around them, bit for bit.

Every case of tests/linattn_exact_inputs.py runs on selector columns: the softmax over the tokens is 2^-j on a chosen token set and 0
off it, q, v and dOut are small whole numbers, every reduction is exact in f32 in any order (`assert_exactly_summable`, on the very
tensors), so the statistics, ctx, dk and dv of each entry point -- and out, dq, dk, dv of the whole op -- must EQUAL the float64 closed
form: torch.equal, no tolerance.  Outputs are NaN-filled with canaries behind them, workspaces are exactly as long as the library asks
with a canary behind them, a second launch must give the same bits.  Each case runs on the packed layout the op passes (ld = 3C, k and v
thirds of one buffer) and on an independent one (own buffers, ld = 3C + 8, stride = T ld + 12, ldo = C + 4) whose input gaps hold NaN and
whose output gaps hold a value that must survive.  Random-normal operands at the two multi-split shapes and non-finite k run under the
rule of tests/linattn_ref.py; the argument contract follows tests/test_conv3x3_f32_exact_gpu.py `refuse`.
profiles/linattn_exact.md has the cases, the fault matrix, the figures and the kernel mutations these tests were shown to catch."""
import pytest
import torch

import linattn_exact_inputs as X
import linattn_ref as R
from canary_buffers import DEV, assert_canary, assert_workspace_canary, call, out_buf, padded, workspace

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_WORKSPACE = 1, 2
NAN = float("nan")
GAPVAL = -777.0                 # what the gaps of a strided output hold
LAYOUTS = ("packed", "independent")
_CASES, _GOT = {}, {}


def case_of(shape):
    """(case, closed form) of one shape, made once, held to the condition before anything runs on it"""
    if shape not in _CASES:
        case = X.make_case(*shape)
        ref = X.closed_form(case)
        X.assert_exactly_summable(case, ref)
        _CASES[shape] = (case, ref)
    return _CASES[shape]


# ------------------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------------------
def lay(x, ld, stride, off=0, into=None, fill=NAN):
    """host [N, C, T] -> flat [N * stride]: token rows of C floats, ld apart, images stride apart, from float `off`"""
    n, c, t = x.shape
    buf = into if into is not None else torch.full((n * stride,), fill)
    buf.as_strided((n, t, c), (stride, ld, 1), off).copy_(x.permute(0, 2, 1).float())
    return buf


def unlay(flat, n, c, t, ld, stride, off=0):
    return flat.as_strided((n, t, c), (stride, ld, 1), off).permute(0, 2, 1).contiguous()


class Operands:
    """k and v of a case on the device in one of LAYOUTS, and NaN-filled dk / dv buffers in the layout's output form"""

    def __init__(self, case, layout):
        n, c, t = case["n"], case["c"], case["t"]
        self.n, self.c, self.t, self.layout = n, c, t, layout
        if layout == "packed":
            self.ld = self.ldo = 3 * c
            self.stride = self.stride_o = t * 3 * c
            host = lay(case["q"], self.ld, self.stride)
            lay(case["k"], self.ld, self.stride, c, host)
            lay(case["v"], self.ld, self.stride, 2 * c, host)
            buf, view = padded(host)
            self.held = [buf]
            self.k, self.v = view.data_ptr() + 4 * c, view.data_ptr() + 8 * c
            self.out_offs = (c, 2 * c)
        else:
            self.ld, self.ldo = 3 * c + 8, c + 4
            self.stride, self.stride_o = t * self.ld + 12, t * self.ldo + 20
            kb, vb = padded(lay(case["k"], self.ld, self.stride)), padded(lay(case["v"], self.ld, self.stride))
            self.held = [kb[0], vb[0]]
            self.k, self.v = kb[1].data_ptr(), vb[1].data_ptr()
            self.out_offs = (0, 0)
        assert self.k % 16 == 0 and self.v % 16 == 0

    def new_outputs(self):
        """[(buffer, view)] for dk and dv (packed: the same pair twice), output elements NaN, gaps GAPVAL; pointers (dk, dv)"""
        n, c, t = self.n, self.c, self.t
        blank = torch.full((n, c, t), NAN)
        host = torch.full((n * self.stride_o,), GAPVAL)
        if self.layout == "packed":
            for off in self.out_offs:
                lay(blank, self.ldo, self.stride_o, off, host)
            pair = padded(host)
            return [pair, pair], (pair[1].data_ptr() + 4 * self.out_offs[0], pair[1].data_ptr() + 4 * self.out_offs[1])
        pairs = [padded(lay(blank, self.ldo, self.stride_o, 0, host.clone())) for _ in range(2)]
        return pairs, (pairs[0][1].data_ptr(), pairs[1][1].data_ptr())

    def read_outputs(self, pairs):
        """(dk, dv) host [N, C, T]; asserts that every gap still holds GAPVAL"""
        n, c, t = self.n, self.c, self.t
        res, flats = [], {}
        for (buf, view), off in zip(pairs, self.out_offs):
            flat = flats.setdefault(id(buf), view.cpu().clone())
            res.append(unlay(view.cpu(), n, c, t, self.ldo, self.stride_o, off))
            lay(torch.full((n, c, t), GAPVAL), self.ldo, self.stride_o, off, flat)
        for flat in flats.values():
            assert (flat == GAPVAL).all().item(), "the kernel wrote into a gap of a strided output"
        return res


def put(t):
    """(buffer with canary, device view) of a host tensor as f32"""
    return padded(t.float().contiguous())


# ------------------------------------------------------------------------------------------------------------------------------
# 1, 2. each entry point alone
# ------------------------------------------------------------------------------------------------------------------------------
def run_entry_points(L, case, ref, layout):
    """dict m, rinv, ctx, dk, dv (host f32) of the three entry points, each on the float64 values of what precedes it"""
    n, c, t = case["n"], case["c"], case["t"]
    op = Operands(case, layout)
    got = {}

    def twice(launch, outs, names):
        """launch, read, re-fill with NaN, launch again: the same bits"""
        launch()
        torch.cuda.synchronize()
        first = [v.cpu().clone() for _, v in outs]
        for _, v in outs:
            v.fill_(NAN)
        launch()
        torch.cuda.synchronize()
        for name, a, (_, v) in zip(names, first, outs):
            assert torch.equal(a, v.cpu()), name + ": two launches differ"
            assert not torch.isnan(a).any().item(), name + ": an element was never written"
        assert_canary(*[b for b, _ in outs], *op.held)
        return first

    # column statistics
    mb, rb = out_buf(n * c), out_buf(n * c)
    nbytes = L.odvae_linattn_colstats_workspace_bytes(n, t, c)
    assert nbytes == n * X.ceil_div(t, X.STAT_SPLIT) * c * 8
    ws = workspace(nbytes)
    m, rinv = twice(lambda: call(L.odvae_linattn_colstats_f32, op.k, op.ld, op.stride, n, t, c, mb[1].data_ptr(), rb[1].data_ptr(),
                                 ws.data_ptr(), nbytes), [mb, rb], ["m", "rinv"])
    assert_workspace_canary(ws)
    got["m"], got["rinv"] = m.view(n, c), rinv.view(n, c)
    # context product, on the float64 statistics
    m64, r64 = put(ref["m"]), put(ref["rinv"])
    cb = out_buf(n * c * c)
    nbytes = L.odvae_linattn_ctx_workspace_bytes(n, t, c)
    assert nbytes == n * X.ceil_div(t, X.CTX_SPLIT) * c * c * 4
    ws = workspace(nbytes)
    ws_f32 = ws[:nbytes].view(torch.float32)
    ws_f32.fill_(NAN)                     # a partial tile the first kernel skips poisons the sum
    ctx, = twice(lambda: call(L.odvae_linattn_ctx_f32, op.k, op.v, op.ld, op.stride, m64[1].data_ptr(), r64[1].data_ptr(), n, t, c,
                              cb[1].data_ptr(), ws.data_ptr(), nbytes), [cb], ["ctx"])
    assert_workspace_canary(ws)
    assert_canary(m64[0], r64[0])
    got["ctx"] = ctx.view(n, c, c)
    # backward for k and v, on the float64 dctx and g
    dc64, g64 = put(ref["dctx"]), put(ref["g"])
    pairs, (dkp, dvp) = op.new_outputs()
    launch = lambda: call(L.odvae_linattn_dkv_f32, op.k, op.v, op.ld, op.stride, m64[1].data_ptr(), r64[1].data_ptr(), dc64[1].data_ptr(),
                          g64[1].data_ptr(), n, t, c, dkp, dvp, op.ldo, op.stride_o)
    launch()
    torch.cuda.synchronize()
    got["dk"], got["dv"] = op.read_outputs(pairs)
    pairs2, (dkp, dvp) = op.new_outputs()
    launch()
    torch.cuda.synchronize()
    again = op.read_outputs(pairs2)
    for name, a in zip(("dk", "dv"), again):
        assert torch.equal(got[name], a), name + ": two launches differ"
        assert not torch.isnan(a).any().item(), name + ": an element was never written"
    assert_canary(*[b for b, _ in pairs + pairs2], *op.held, m64[0], r64[0], dc64[0], g64[0])
    return got


def mismatch(got, want):
    bad = (got.double() != want).nonzero()
    return "%d of %d elements differ, first at %s: %r vs %r" % (len(bad), want.numel(), bad[0].tolist(), got[tuple(bad[0])].item(),
                                                                  want[tuple(bad[0])].item())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", X.CASES, ids=str)
def test_each_entry_point_equals_float64(hip_lib, shape, layout):
    case, ref = case_of(shape)
    got = run_entry_points(hip_lib, case, ref, layout)
    for name in ("m", "rinv", "ctx", "dk", "dv"):
        same = torch.equal(got[name].double(), ref[name])
        assert same, "%s %s %s: %s" % (shape, layout, name, mismatch(got[name], ref[name]))
    _GOT[(shape, layout)] = got
    other = _GOT.get((shape, LAYOUTS[1 - LAYOUTS.index(layout)]))
    if other is not None:           # the two layouts, bit for bit (-0.0 against 0.0 would pass the comparison with float64)
        for name in got:
            assert torch.equal(got[name].view(torch.int32), other[name].view(torch.int32)), name


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the whole op
# ------------------------------------------------------------------------------------------------------------------------------
class highest_precision:
    """float32 matmul precision `highest` inside, whatever was set before restored afterwards"""

    def __enter__(self):
        import odvae_amd
        from odvae_amd import ops
        self.before = ops.get_float32_matmul_precision()
        odvae_amd.set_float32_matmul_precision("highest")

    def __exit__(self, *exc):
        import odvae_amd
        odvae_amd.set_float32_matmul_precision(self.before)


def run_op(q, k, v, do, form="channels_last"):
    """dict as linattn_ref.host_model returns it (host tensors) from ops.linear_attention_qkv and its backward; form: how the packed
    projection is laid out when the op receives it"""
    from odvae_amd import ops
    n, c, t = q.shape
    packed = R.pack(q.float(), k.float(), v.float()).to(DEV)
    if form == "channels_last":
        leaf = packed.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        qkv = leaf
    elif form == "nchw":
        leaf = packed.contiguous().requires_grad_(True)
        qkv = leaf
    else:
        assert form == "slice"
        leaf = torch.cat([packed, packed.flip(1) + 1.0], dim=1).requires_grad_(True)
        qkv = leaf[:, :3 * c]
    o = ops.linear_attention_qkv(qkv)
    _, ctx, stats = o.grad_fn.saved_tensors
    o.backward(do.float().reshape(o.shape).to(DEV))
    grad = leaf.grad
    if form == "slice":
        assert float(grad[:, 3 * c:].abs().max()) == 0.0
        grad = grad[:, :3 * c]
    dq, dk, dv = grad.reshape(n, 3, c, t).unbind(1)
    res = dict(out=o.detach().reshape(n, c, t), ctx=ctx, m=stats[0], rinv=stats[1], dq=dq, dk=dk, dv=dv)
    return {name: x.detach().cpu().contiguous() for name, x in res.items()}


@pytest.mark.parametrize("shape", X.CASES, ids=str)
def test_whole_op_equals_float64(hip_lib, shape):
    """the three batched GEMM calls and rowdot as autograd wires them, the strided lda = 3C included"""
    case, ref = case_of(shape)
    with highest_precision():
        for form in ("channels_last", "nchw", "slice"):
            got = run_op(case["q"], case["k"], case["v"], case["do"], form)
            for name in X.NAMES:
                same = torch.equal(got[name].double(), ref[name])
                assert same, "%s %s %s: %s" % (shape, form, name, mismatch(got[name], ref[name]))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. random-normal operands at the multi-split shapes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,t,a", [(3, 96, 2051, 0), (3, 96, 2051, 90), (2, 128, 1025, 0)], ids=str)
def test_random_normal_at_the_multi_split_shapes(hip_lib, n, c, t, a):
    """the rule of tests/linattn_ref.py where splits, tiles and images multiply; offset 90 overflows exp without the column maximum"""
    assert a in R.OFFSETS
    q, k, v, do = R.make_qkv(n, c, t, offset=a)
    refs = R.core_refs(q, k, v, do)
    with highest_precision():
        got = run_op(q, k, v, do)
    assert all(torch.isfinite(x).all() for x in got.values())
    R.check(R.core_figures(got, refs), "N%d C%d T%d offset %g" % (n, c, t, a))        # prints every figure before it asserts


# ------------------------------------------------------------------------------------------------------------------------------
# 5. non-finite k
# ------------------------------------------------------------------------------------------------------------------------------
NF_SHAPE = (2, 64, 33)
NF_D, NF_T = 37, 21             # the poisoned column of image 0 and its token: second tile, second 16-token chunk, odd


def test_minus_inf_tokens_are_a_mask(hip_lib):
    """-inf at a few tokens of some columns (never a whole column): everything stays finite and within the rule of the float64
    reference of the same tensors, and dk is exactly 0 there"""
    q, k, v, do = R.make_qkv(*NF_SHAPE)
    mask = torch.zeros(NF_SHAPE, dtype=torch.bool)
    for b, d, toks in ((0, 0, (0,)), (0, 5, (1, 8, 9, 32)), (0, NF_D, (NF_T, 32)), (1, 63, tuple(range(0, 32))), (1, 33, (16, 17, 31))):
        mask[b, d, list(toks)] = True
    assert not mask.all(-1).any()
    k = k.masked_fill(mask, -float("inf"))
    refs = R.core_refs(q, k, v, do)
    assert all(torch.isfinite(x).all() for x in refs[64].values())
    with highest_precision():
        got = run_op(q, k, v, do)
    for name, x in got.items():
        assert torch.isfinite(x).all().item(), name
    R.check(R.core_figures(got, refs), "-inf tokens")
    assert float(got["dk"][mask].abs().max()) == 0.0


@pytest.mark.parametrize("bad", [NAN, float("inf")], ids=["nan", "plus_inf"])
def test_nan_and_plus_inf_never_give_a_finite_context_row(hip_lib, bad):
    """one NaN (+inf) in column d of image 0: m or 1 / l of the column, the whole context row d and all of image 0's out are
    non-finite -- detect_anomaly sees it -- and image 1 has the bits of the run without it"""
    q, k, v, do = R.make_qkv(*NF_SHAPE)
    kb = k.clone()
    kb[0, NF_D, NF_T] = bad
    with highest_precision():
        clean, got = run_op(q, k, v, do), run_op(q, kb, v, do)
    assert not (torch.isfinite(got["m"][0, NF_D]).item() and torch.isfinite(got["rinv"][0, NF_D]).item())
    assert not torch.isfinite(got["ctx"][0, NF_D]).any().item(), "a finite element in the context row of a non-finite column"
    assert not torch.isfinite(got["out"][0]).any().item()
    for name in got:
        assert torch.equal(got[name][1], clean[name][1]), name + ": image 1 changed"


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the argument contract
# ------------------------------------------------------------------------------------------------------------------------------
def refuse(L, what, call_, code, name, outs, held, ws=None):
    L.odvae_conv3x3_wgrad_f32(0, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, None, 0, None)      # leaves another entry point's message
    stale = L.odvae_last_error()
    assert call_() == code, what
    msg = L.odvae_last_error()
    assert msg and msg != stale and name in msg, what + ": no message of its own"
    torch.cuda.synchronize()
    for buf, view in outs:
        assert torch.isnan(view).all().item(), what + ": a refused call wrote an output"
    if ws is not None:
        assert torch.isnan(ws[:-64].view(torch.float32)).all().item(), what + ": a refused call wrote its workspace"
        assert_workspace_canary(ws)
    assert_canary(*[b for b, _ in outs], *held)


def test_argument_contract(hip_lib):
    """what a launcher refuses, it refuses before it launches anything: the code, a message of its own, outputs still all NaN"""
    from odvae_amd import lib
    L, s = hip_lib, lib.stream_ptr()
    n, c, t = 2, 64, 33
    ld, ldo = 3 * c + 8, c + 4
    stride, stride_o = t * ld + 12, t * ldo + 20
    kb, vb = put(torch.zeros(n * stride)), put(torch.zeros(n * stride))
    mb, rb, gb, dcb = put(torch.zeros(n * c)), put(torch.ones(n * c)), put(torch.zeros(n * c)), put(torch.zeros(n * c * c))
    held = [b for b, _ in (kb, vb, mb, rb, gb, dcb)]
    K, V, M, RI, G, DC = (x[1].data_ptr() for x in (kb, vb, mb, rb, gb, dcb))
    # dkv
    dkb, dvb = out_buf(n * stride_o), out_buf(n * stride_o)
    DK, DV = dkb[1].data_ptr(), dvb[1].data_ptr()
    f = L.odvae_linattn_dkv_f32

    def dkv(k=K, v=V, ld=ld, stride=stride, m=M, ri=RI, dc=DC, g=G, n=n, t=t, c=c, dk=DK, dv=DV, ldo=ldo, stride_o=stride_o):
        return lambda: f(k, v, ld, stride, m, ri, dc, g, n, t, c, dk, dv, ldo, stride_o, s)

    tight = (t - 1) * ld + c            # the smallest image stride, itself a multiple of 4
    assert tight % 4 == 0
    refusals = [
        ("ld + 1", dkv(ld=ld + 1)), ("ld + 2", dkv(ld=ld + 2)), ("stride + 1", dkv(stride=stride + 1)), ("stride + 2", dkv(stride=stride + 2)),
        ("k off by 4 bytes", dkv(k=K + 4)), ("v off by 4 bytes", dkv(v=V + 4)), ("m off by 4 bytes", dkv(m=M + 4)),
        ("1/l off by 4 bytes", dkv(ri=RI + 4)), ("dctx off by 4 bytes", dkv(dc=DC + 4)),
        ("ldo < C", dkv(ldo=c - 4)), ("stride_o one float short", dkv(stride_o=(t - 1) * ldo + c - 1)),
        ("ld < C", dkv(ld=c - 4, stride=stride)), ("stride one float short", dkv(stride=tight - 1)),
        ("stride four floats short", dkv(stride=tight - 4)),
        ("N = 0", dkv(n=0)), ("C = 48", dkv(c=48)), ("C = 0", dkv(c=0)), ("T = 0", dkv(t=0)),
    ] + [("%s null" % name, dkv(**{name: None})) for name in ("k", "v", "m", "ri", "dc", "g", "dk", "dv")]
    for what, fn in refusals:
        refuse(L, "dkv " + what, fn, ERR_ARG, b"linattn_dkv", [dkb, dvb], held)
    # colstats
    mo, ro = out_buf(n * c), out_buf(n * c)
    MO, RO = mo[1].data_ptr(), ro[1].data_ptr()
    nb = L.odvae_linattn_colstats_workspace_bytes(n, t, c)
    assert nb > 0 and L.odvae_linattn_colstats_workspace_bytes(0, t, c) == 0
    ws = workspace(nb)
    ws[:nb].view(torch.float32).fill_(NAN)
    f1 = L.odvae_linattn_colstats_f32

    def colstats(k=K, ld=ld, stride=stride, n=n, t=t, c=c, m=MO, ri=RO, w=ws.data_ptr(), nbytes=nb):
        return lambda: f1(k, ld, stride, n, t, c, m, ri, w, nbytes, s)

    refusals = [("N = 0", colstats(n=0)), ("C = 48", colstats(c=48)), ("T = 0", colstats(t=0)), ("ld < C", colstats(ld=c - 1)),
                ("stride one float short", colstats(stride=tight - 1))]
    refusals += [("%s null" % name, colstats(**{name: None})) for name in ("k", "m", "ri", "w")]
    for what, fn in refusals:
        refuse(L, "colstats " + what, fn, ERR_ARG, b"linattn_colstats", [mo, ro], held, ws)
    refuse(L, "colstats workspace one byte short", colstats(nbytes=nb - 1), ERR_WORKSPACE, b"linattn_colstats", [mo, ro], held, ws)
    # ctx
    co = out_buf(n * c * c)
    CO = co[1].data_ptr()
    nb = L.odvae_linattn_ctx_workspace_bytes(n, t, c)
    assert nb > 0 and L.odvae_linattn_ctx_workspace_bytes(n, 0, c) == 0
    ws = workspace(nb)
    ws[:nb].view(torch.float32).fill_(NAN)
    f2 = L.odvae_linattn_ctx_f32

    def ctx(k=K, v=V, ld=ld, stride=stride, m=M, ri=RI, n=n, t=t, c=c, o=CO, w=ws.data_ptr(), nbytes=nb):
        return lambda: f2(k, v, ld, stride, m, ri, n, t, c, o, w, nbytes, s)

    refusals = [("N = 0", ctx(n=0)), ("C = 48", ctx(c=48)), ("T = 0", ctx(t=0)), ("ld < C", ctx(ld=c - 1)),
                ("stride one float short", ctx(stride=tight - 1))]
    refusals += [("%s null" % name, ctx(**{name: None})) for name in ("k", "v", "m", "ri", "o", "w")]
    for what, fn in refusals:
        refuse(L, "ctx " + what, fn, ERR_ARG, b"linattn_ctx", [co], held, ws)
    refuse(L, "ctx workspace one byte short", ctx(nbytes=nb - 1), ERR_WORKSPACE, b"linattn_ctx", [co], held, ws)
