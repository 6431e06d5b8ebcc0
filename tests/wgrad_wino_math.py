"""Host-side mathematics of the Winograd-domain weight gradient (conv3x3_wgrad_wino_f32.hip) and of its bf16-split main loop, in float64
on the CPU, for tests/test_wgrad_wino_split.py and tests/test_wgrad_wino_split_gpu.py.  Plain module: no fixtures, no device.

    V[xi] = (B^T d B)[xi] of the 4x4 input patch, dM[xi] = (A dY A^T)[xi] of the 2x2 output-gradient tile, xi = 4 r + c
    dU[xi][ci][co] = sum over tiles V[xi][tile][ci] dM[xi][tile][co],   dw[co][ci] = G^T dU G

Exact recipes (in the manner of tests/exact_inputs.py): operands on which every product the split loop keeps is a whole number, every
partial sum stays below 2^20 in magnitude (so it is exact in f32 in any order, and so are the halves and quarters the G^T . G reduction
makes of it), and the three products it drops (mid lo, lo mid, lo lo) are all zero -- the split loop must then return the float64
gradient bit for bit.  No single recipe can populate all six kept products with the dropped ones zero, so there are three:
    "x3"  V has hi, mid and lo planes, dM only hi            -> lo hi, mid hi, hi hi carry the result
    "dy3" dM has hi, mid and lo planes, V only hi            -> hi lo, hi mid, hi hi
    "22"  both have hi and mid planes, no lo                 -> mid mid, mid hi, hi mid, hi hi
make_exact() asserts all of this on the transformed tensors."""
import torch
import torch.nn.functional as F

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
A = torch.tensor([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
HI, MID, LO = 0, 1, 2
KEPT = ((LO, HI), (HI, LO), (MID, MID), (MID, HI), (HI, MID), (HI, HI))      # the loop's order, smallest first
DROPPED = ((MID, LO), (LO, MID), (LO, LO))
CHUNK = 16                                                                    # tiles per k step of the bf16 MFMA


def domain(x, dy):
    """x [N][Cin][H][W], dy [N][Cout][H][W] float64 -> V [16][tiles][Cin], dM [16][tiles][Cout], tiles in the kernel's order (image, tile
    row, tile column)."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)            # [N][Cin][TY][TX][4][4]
    v = BT @ d @ BT.t()
    t = dy.unfold(2, 2, 2).unfold(3, 2, 2)                               # [N][Cout][TY][TX][2][2]
    m = A @ t @ A.t()
    v = v.permute(4, 5, 0, 2, 3, 1).reshape(16, -1, cin)
    m = m.permute(4, 5, 0, 2, 3, 1).reshape(16, -1, cout)
    return v, m


def to_weights(du):
    """dU [16][Cin][Cout] -> dw [Cout][Cin][3][3]"""
    u = du.reshape(4, 4, du.shape[1], du.shape[2])
    return torch.einsum("ra,rcio,cb->oiab", G, u, G)


def wgrad_f64(x, dy):
    """The float64 weight and bias gradient of F.conv2d(x, w, b, stride=1, padding=1)."""
    cin, cout = x.shape[1], dy.shape[1]
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, b, padding=1).backward(dy)
    return w.grad, b.grad


def sbar(x, dy):
    """max entry of |G|^T (sum over tiles |V| |dM|) |G|: the weight-domain image of sum |a| |b|"""
    v, m = domain(x, dy)
    s = torch.einsum("xti,xto->xio", v.abs(), m.abs()).reshape(4, 4, x.shape[1], dy.shape[1])
    return torch.einsum("ra,rcio,cb->oiab", G.abs(), s, G.abs()).max().item()


def planes(t):
    """float64 tensor of f32 values -> (hi, mid, lo) as float64: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), round to
    nearest even, the differences taken in f32 (where they are exact)"""
    v = t.float()
    hi = v.bfloat16().float()
    r = v - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi.double(), mid.double(), lo.double()


def split_sum(v, m, pairs=KEPT, keep=None):
    """sum over `pairs` of (plane p of V)^T (plane q of dM) -> dU [16][Cin][Cout], float64.  keep: optional [tiles] 0/1 mask per operand
    element [16][tiles][channels] multiplied into the V planes (to model a loader that loses something)."""
    vp, mp = planes(v), planes(m)
    du = torch.zeros(16, v.shape[2], m.shape[2], dtype=torch.float64)
    for p, q in pairs:
        a = vp[p] if keep is None else vp[p] * keep
        du += torch.einsum("xti,xto->xio", a, mp[q])
    return du


def _three_plane_values(g, shape, density):
    """sparse +-(2^16 + 256 q + s), q, s in 1..255: 17 significant bits, all three bf16 planes populated"""
    q = torch.randint(1, 256, shape, generator=g).double()
    s = torch.randint(1, 256, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    on = (torch.rand(shape, generator=g) < density).double()
    return on * sign * (65536.0 + 256.0 * q + s)


def _two_plane_values(g, shape, density):
    """sparse +-(256 + odd s), s below 64: nine significant bits, hi and mid populated, sums of four still without a lo plane"""
    s = (torch.randint(0, 32, shape, generator=g) * 2 + 1).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    on = (torch.rand(shape, generator=g) < density).double()
    return on * sign * (256.0 + s)


def _few_units(g, shape, per_channel):
    """+-1 at `per_channel` pixels of every (image-independent) channel, 0 elsewhere"""
    n, c, h, w = shape
    t = torch.zeros(shape, dtype=torch.float64)
    for ch in range(c):
        for _ in range(per_channel):
            i = int(torch.randint(0, n * h * w, (1,), generator=g))
            t[i // (h * w), ch, (i // w) % h, i % w] = float(int(torch.randint(0, 2, (1,), generator=g)) * 2 - 1)
    return t


def make_exact(recipe, n, cin, cout, h, w, seed=0):
    """x, dy (float64, every value an f32) of an exact recipe; asserts the recipe's conditions on V and dM."""
    g = torch.Generator().manual_seed(seed)
    if recipe == "x3":
        x = _three_plane_values(g, (n, cin, h, w), 1.0 / 8)
        dy = _few_units(g, (n, cout, h, w), 3)
    elif recipe == "dy3":
        x = _few_units(g, (n, cin, h, w), 1)
        dy = _three_plane_values(g, (n, cout, h, w), 1.0 / 16)
    elif recipe == "22":
        x = _two_plane_values(g, (n, cin, h, w), 1.0 / 16)
        dy = _two_plane_values(g, (n, cout, h, w), 1.0 / 128)
    else:
        raise ValueError(recipe)
    v, m = domain(x, dy)
    vp, mp = planes(v), planes(m)
    assert all(torch.equal(p, p.round()) for p in vp + mp), "planes are whole numbers"
    assert torch.equal(vp[0] + vp[1] + vp[2], v) and torch.equal(mp[0] + mp[1] + mp[2], m), "the split is exact"
    bound = torch.einsum("xti,xto->xio", v.abs(), m.abs()).max().item()
    # every partial sum of every kept product is a whole number below this; 2^20 leaves the reduction's quarters exact in f32
    assert bound * (1 + 2.0 ** -7) ** 2 < 2.0 ** 20, "%s: sum |V| |dM| = %g is not below 2^20" % (recipe, bound)
    for p, q in DROPPED:
        assert torch.einsum("xti,xto->xio", vp[p].abs(), mp[q].abs()).max().item() == 0.0, "%s: a dropped product is populated" % recipe
    want = {"x3": ((LO, HI), (MID, HI), (HI, HI)), "dy3": ((HI, LO), (HI, MID), (HI, HI)), "22": ((MID, MID), (MID, HI), (HI, MID), (HI, HI))}[recipe]
    for p, q in want:
        assert torch.einsum("xti,xto->xio", vp[p], mp[q]).abs().max().item() > 0.0, "%s: product %s is empty" % (recipe, (p, q))
    return x, dy


def populated(recipe):
    return {"x3": ((LO, HI), (MID, HI), (HI, HI)), "dy3": ((HI, LO), (HI, MID), (HI, HI)), "22": ((MID, MID), (MID, HI), (HI, MID), (HI, HI))}[recipe]
