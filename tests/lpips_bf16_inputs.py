"""Host model of the bf16 perceptual net (gan.LPIPSStyle.set_precision("bf16")), its inputs and its planted faults.

The model is torch on the CPU and follows the rounding chain of the HIP path store by store:
  * conv weights are rounded to bf16 once (the packs), biases stay f32;
  * every feature map and every feature gradient is rounded to nearest even exactly once, where the kernel stores it;
  * sums are formed in the working dtype `dt` in between: float32 for the model proper (the kernels accumulate in f32), float64 for
    the bit-for-bit tests on exactly summable operands, where no f32 addition rounds and the float64 value rounded once IS the answer;
  * the distance arithmetic (norms, quotients, the lin product, the spatial mean) is done in `dt` in the order of lpips_distance_kernel;
  * a ReLU's backward rides with whoever produces its incoming gradient: `mask > 0 ? value : 0` in front of the one rounding.
The backward is written out by hand (no autograd), so that each rounding sits where the kernels have it.

`fault` plants one mistake the GPU tests exist to catch (tests/test_lpips_bf16_inputs.py shows each is rejected):
  relu_after_round   the ReLU is a max applied to the rounded value and drops a NaN
  mask_wrong_layer   a conv's data gradient is masked with the conv's own output instead of its input
  mask_ge            mask >= 0 instead of mask > 0
  tap_round_twice    the tap's own gradient is rounded to bf16 before the next slice's gradient is added
  pool_tie_other     a pool tie goes to the LAST maximum of the window
Plain module: no fixtures, no device.
"""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
FAULTS = ("relu_after_round", "mask_wrong_layer", "mask_ge", "tap_round_twice", "pool_tie_other")


def rne(t):
    """one rounding to bf16 (nearest even), the value handed back in t's own dtype"""
    return t.float().to(BF).to(t.dtype)


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------------------------------------
# layers
# ------------------------------------------------------------------------------------------------------------------------------
def scaling_fwd(x, shift, scale):
    return rne((x - shift.view(1, -1, 1, 1)) / scale.view(1, -1, 1, 1))


def conv_relu_fwd(x, w, b, fault=None):
    s = F.conv2d(x, w, b, padding=1)
    if fault == "relu_after_round":
        r = rne(s)
        return torch.where(r > 0, r, torch.zeros_like(r))
    return rne(torch.relu(s))


def conv_dgrad(dy, w):
    """d conv3x3(stride 1, pad 1) / d x applied to dy, unrounded"""
    return F.conv_transpose2d(dy, w, padding=1)


def apply_mask(g, mask, fault=None):
    keep = (mask >= 0) if fault == "mask_ge" else (mask > 0)
    return torch.where(keep, g, torch.zeros_like(g))


def _windows(t, ho, wo):
    return [t[:, :, 0:2 * ho:2, 0:2 * wo:2], t[:, :, 0:2 * ho:2, 1:2 * wo:2], t[:, :, 1:2 * ho:2, 0:2 * wo:2], t[:, :, 1:2 * ho:2, 1:2 * wo:2]]


def pool_fwd(x):
    ho, wo = x.shape[2] // 2, x.shape[3] // 2
    return torch.stack(_windows(x, ho, wo)).amax(0)       # amax hands a NaN on


def pool_bwd(x, dy, mask=None, fault=None):
    """torch's rule: dy goes to the window's first maximum in row-major order (in a NaN window to its first NaN); a dropped odd row /
    column gets 0; with a mask the element is kept only where mask > 0"""
    ho, wo = x.shape[2] // 2, x.shape[3] // 2
    m = pool_fwd(x)
    dx = torch.zeros_like(x)
    done = torch.zeros_like(m, dtype=torch.bool)
    order = (3, 2, 1, 0) if fault == "pool_tie_other" else (0, 1, 2, 3)
    xw, dw = _windows(x, ho, wo), _windows(dx, ho, wo)
    for k in order:
        hit = ~done & ((xw[k] == m) | (torch.isnan(m) & torch.isnan(xw[k])))
        dw[k].copy_(torch.where(hit, dy, torch.zeros_like(dy)))
        done = done | hit
    if mask is not None:
        dx = apply_mask(dx, mask, fault)
    return dx


def dist_fwd(f0, f1, w):
    """[N] = spatial mean of sum_c w[c] (f0/n0 - f1/n1)^2, n = sqrt(sum f^2) + 1e-10, in the dtype of the features"""
    ia = 1.0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
    ib = 1.0 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
    t = f0 * ia - f1 * ib
    return (w.view(1, -1, 1, 1) * t * t).sum(1).mean((1, 2))


def dist_bwd(f0, f1, w, g, dnext=None, mask=None, fault=None):
    """gradient w.r.t. f1 at the tap, as lpips_distance_bwd_bf16_kernel forms it; the normalisation term is 0 at an all-zero f1"""
    hw = f1.shape[2] * f1.shape[3]
    gs = (g / hw).view(-1, 1, 1, 1)
    s1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
    n1 = s1 + 1e-10
    ia, ib = 1.0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10), 1.0 / n1
    gb = -2.0 * w.view(1, -1, 1, 1) * (f0 * ia - f1 * ib)
    dot = (gb * f1).sum(1, keepdim=True)
    coef = torch.where(s1 > 0, dot / (n1 * n1 * torch.where(s1 > 0, s1, torch.ones_like(s1))), torch.zeros_like(s1))
    o = gs * (gb * ib - coef * f1)
    if fault == "tap_round_twice":
        o = rne(o)
    if dnext is not None:
        o = o + dnext
    if mask is not None:
        o = apply_mask(o, mask, fault)
    return rne(o)


# ------------------------------------------------------------------------------------------------------------------------------
# the net: slices of conv+ReLU layers with a pool in front of every slice but the first and an optional distance tap behind each
# ------------------------------------------------------------------------------------------------------------------------------
def net_params(state_dict, slices):
    """(shift, scale, [[(w, b), ...] per slice], [lin_k]) of a gan.LPIPSStyle / oracle LPIPSStyle state_dict (f32, host)"""
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
    convs = [[(sd["net.%s.%d.weight" % (name, idx)], sd["net.%s.%d.bias" % (name, idx)]) for idx, _, _ in layers] for name, layers in slices]
    lins = [sd["lin%d.model.1.weight" % k].reshape(-1) for k in range(len(slices))]
    return sd["scaling_layer.shift"].reshape(-1), sd["scaling_layer.scale"].reshape(-1), convs, lins


def features(x, shift, scale, convs, dt, fault=None):
    """-> (per slice: the tap feature), (per layer: its input) of one branch"""
    h = scaling_fwd(x.to(dt), shift.to(dt), scale.to(dt))
    taps, inputs = [], []
    for k, layers in enumerate(convs):
        if k > 0:
            h = pool_fwd(h)
        ins = []
        for w, b in layers:
            ins.append(h)
            h = conv_relu_fwd(h, rne(w.to(dt)), None if b is None else b.to(dt), fault)
        taps.append(h)
        inputs.append(ins)
    return taps, inputs


def net(x0, x1, shift, scale, convs, lins, g, g_pass=None, dt=torch.float32, fault=None):
    """d [N] (the sum over the taps) and its gradient w.r.t. x1 (f32 arithmetic, 3 channels) for upstream gradient g [N] of d; g_pass: an
    extra gradient arriving at the LAST tap's feature from above (the pass-through output of ops.lpips_tap_bf16).  lins[k] None: no tap
    behind slice k -- the pool that follows then reads a plain ReLU output and carries its mask.
    -> dict d, dx, taps (features of x1), dtaps (gradient stored at each tap feature)"""
    f0, _ = features(x0, shift, scale, convs, dt, fault)
    f1, ins = features(x1, shift, scale, convs, dt, fault)
    g = g.to(dt)
    lins = [None if l is None else l.to(dt) for l in lins]
    d = sum(dist_fwd(f0[k], f1[k], lins[k]) for k in range(len(convs)) if lins[k] is not None)
    dh = None if g_pass is None else g_pass.to(dt)
    dtaps = [None] * len(convs)
    for k in reversed(range(len(convs))):
        if lins[k] is not None:
            dh = dist_bwd(f0[k], f1[k], lins[k], g, dnext=dh, mask=f1[k], fault=fault)
        dtaps[k] = dh
        for j in reversed(range(len(convs[k]))):
            w = rne(convs[k][j][0].to(dt))
            du = conv_dgrad(dh, w)
            if j > 0:          # the layer's input is the ReLU output of the layer below
                below = ins[k][j]
                if fault == "mask_wrong_layer":      # the layer's own output (same shape: these layers keep the channel count)
                    below = ins[k][j + 1] if j + 1 < len(convs[k]) else f1[k]
                dh = rne(apply_mask(du, below, fault))
            elif k > 0:        # the layer's input is the pool's output; the pool's backward carries a mask only without a tap below it
                dh = pool_bwd(f1[k - 1], rne(du), mask=None if lins[k - 1] is not None else f1[k - 1], fault=fault)
            else:              # the image layer: f32, the image's channels, through the scaling backward
                dx = du / scale.to(dt).view(1, -1, 1, 1)
    return {"d": d, "dx": dx, "taps": f1, "dtaps": dtaps}


# ------------------------------------------------------------------------------------------------------------------------------
# exactly summable operands
# ------------------------------------------------------------------------------------------------------------------------------
LIMIT = float(2 ** 24)


def chain_case(n=2, h=9, w=17, seed=3):
    """scaling -> conv+ReLU(3 -> 64) -> conv+ReLU(64 -> 64) -> pool -> conv+ReLU(64 -> 128) -> tap, small whole-number weights:
    shift / scale powers of two, images multiples of 1/2, weights in {-1, 0, 1} (one in eight kept past the image layer), biases whole
    numbers, the pass-through gradient whole numbers in [-4, 4].  Everything is a multiple of 1/2 and the partial sums stay far below
    2^24 units (assert_chain_summable checks it on these very tensors), so float64 with one rounding per store is the exact answer."""
    g = gen(seed, n, h, w)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).double()
    keep = lambda shape, p: (torch.rand(shape, generator=g) < p).double()
    c = {"shift": torch.tensor([0.5, -1.0, 0.0], dtype=torch.float64), "scale": torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)}
    c["x0"], c["x1"] = ri((n, 3, h, w), -4, 4) / 2, ri((n, 3, h, w), -4, 4) / 2
    c["convs"] = [[(ri((64, 3, 3, 3), -1, 1), ri((64,), -2, 2)), (ri((64, 64, 3, 3), -1, 1) * keep((64, 64, 3, 3), 0.125), ri((64,), -8, 2))],
                  [(ri((128, 64, 3, 3), -1, 1) * keep((128, 64, 3, 3), 0.125), ri((128,), -40, 8))]]
    c["lins"] = [None, torch.rand(128, generator=g).double() / 128]
    c["g"] = torch.zeros(n, dtype=torch.float64)          # the distance's own gradient is not exactly summable: seeded through the pass-through
    c["g_pass"] = ri((n, 128, h // 2, w // 2), -4, 4)
    return c


def assert_chain_summable(c, unit=0.5):
    """sum of |terms| of every conv sum, forward and backward, in units, from the tensors of the case (rounded features only grow by
    1 + 2^-8 per store, which the factor below covers)"""
    grow = 1.0 + 2.0 ** -8
    h = ((c["x1"].abs().max(c["x0"].abs()) + c["shift"].abs().view(1, -1, 1, 1)) / c["scale"].view(1, -1, 1, 1))
    pre_pool = []
    for k, layers in enumerate(c["convs"]):
        if k > 0:
            pre_pool.append(h.shape[2:])
            h = pool_fwd(h)
        for w, b in layers:
            h = grow * F.conv2d(h, w.abs(), b.abs(), padding=1)
            assert h.max().item() / unit < LIMIT, "forward sum of |terms| %.3g units" % (h.max().item() / unit)
    dh = c["g_pass"].abs()
    for k in reversed(range(len(c["convs"]))):
        for j in reversed(range(len(c["convs"][k]))):
            dh = grow * conv_dgrad(dh, c["convs"][k][j][0].abs())
            assert dh.max().item() < LIMIT, "backward sum of |terms| %.3g units" % dh.max().item()
        if k > 0:      # the pool's backward moves values, it adds nothing
            up = torch.zeros(dh.shape[0], dh.shape[1], *pre_pool[k - 1], dtype=dh.dtype)
            for wnd in _windows(up, dh.shape[2], dh.shape[3]):
                wnd.copy_(dh)
            dh = up


def conv_case(cin, cout, n, h, w, seed=0, nan_at=None):
    """One conv + ReLU layer on recipe A of exact_inputs (x, dy integers in [-4, 4], w multiples of 1/4, bias multiples of 1/8): x doubles
    as the ReLU mask of the data gradient (it holds zeros, negative and positive values).  cin = 3: the image layer, x padded to 8."""
    import exact_inputs as E
    c = E.make_case("A", 0, n, cin, cout, h, w, bias=True, residual=False, seed=seed, cx=8 if cin == 3 else None)
    if nan_at is not None:
        c["x"][nan_at] = float("nan")
    return c


def conv_case_references(c):
    """y = rne(relu(conv + b)); dx = rne(x > 0 ? dgrad(dy) : 0) (float64; a NaN in x spreads to its 3x3 neighbourhood of y and masks nothing)"""
    cin = c["w"].shape[1]
    y = torch.relu(F.conv2d(c["x"][:, :cin], c["w"], c["b"], padding=1))
    du = conv_dgrad(c["dy"], c["w"])
    return {"y": y.float().to(BF), "y_exact": F.conv2d(c["x"][:, :cin], c["w"], c["b"], padding=1),
            "dx_masked": apply_mask(du, c["x"][:, :cin]).float().to(BF), "dx_plain": du.float().to(BF), "dx_f32": du.float()}


def pool_case(n, c, h, w, seed=0):
    """bf16 values with ties in most windows (small whole numbers), -inf, one NaN window per image, and a mask that is zero at some argmax"""
    g = gen(seed, n, c, h, w)
    x = torch.randint(-2, 3, (n, c, h, w), generator=g).double()
    x[torch.rand(x.shape, generator=g) < 0.05] = float("-inf")
    if h >= 4 and w >= 4:
        x[:, 0, 2, 2] = float("nan")
        x[:, c - 1, 3, 3] = float("nan")
    x[:, 1 % c, 0, 0] = float("-inf"); x[:, 1 % c, 0, 1] = float("-inf"); x[:, 1 % c, 1, 0] = float("-inf"); x[:, 1 % c, 1, 1] = float("-inf")
    dy = torch.randint(-4, 5, (n, c, h // 2, w // 2), generator=g).double()
    mask = torch.randint(-1, 2, (n, c, h, w), generator=g).double()
    return x, dy, mask


def nan_equal_bits(got, want, what):
    """NaN exactly where the reference has NaN; every other element equal in bits (-0 == +0: exact_inputs.assert_bits_equal, summed)"""
    import exact_inputs as E
    gn, wn = torch.isnan(got.float().cpu()), torch.isnan(want.float().cpu())
    assert torch.equal(gn, wn), "%s: NaN at %d places, the reference at %d" % (what, int(gn.sum()), int(wn.sum()))
    z = torch.zeros((), dtype=got.dtype)
    E.assert_bits_equal(torch.where(gn, z, got.cpu()), torch.where(wn, z.to(want.dtype), want.cpu()), what)
