"""Inputs, references and acceptance rules for the pose head: the dense layers of linear_f32.hip and the nine loss terms of pose_f32.hip.
The derivations are in profiles/pose_head_exact.md.  Plain module: no fixtures, no device; float64 values, float32 inputs, on the host.

Dense layers.  `pick_splits`, `kper`, `used_splits` and `workspace_bytes` mirror the launch rule of linear_f32.hip.  `make_linear_case`
makes exactly summable operands (recipe A of gemm_exact_inputs: x, dy integers in [-8, 8], w multiples of 1/4 in [-2, 2], bias multiples
of 1/8 in [-2, 2], all optionally scaled by a power of two): no f32 addition rounds in any order, so y, pre, dx and dw must EQUAL float64.

Pose terms.  `pose_model` evaluates the formulas of contperceptual.py (as restated in oracle/losses.py::PoseLoss.pose_terms) and their
analytic gradients in any dtype; in float64, with log1p and sigmoid(-x) in place of log(1 + e) and 1 - p, it is the reference (`pose_reference`), and in float32 with a
planted fault it is the host model the rule must reject.  `pose_reference` also returns, per output and per gradient element, the bound
of the acceptance rule: (n + r) 2^-24 sum|term| for a sum of n terms of r roundings each, plus what the documented ulp bounds of the
accurate f32 sin, cos, exp, log1p and pow admit, propagated through the formulas.
"""
import math

import torch

from gemm_exact_inputs import LIMIT, _assert_multiples, _ints, ceil_div

U = 2.0 ** -24                 # unit roundoff of f32: one rounding moves a value by at most U of its magnitude
ETA = 2.0 ** -126              # smallest normal f32: what an underflowing operation may lose whether or not subnormals are flushed
FLOOR = 2.0 ** -118            # ETA times 2^8: an underflow inside a leaf is amplified by bce * gamma <= 200 < 2^8 at the most
# documented worst errors, in ulps, of the accurate f32 functions (OpenCL C numerical compliance table, which the device math library is
# built to; the host's are tighter): a k-ulp function has a relative error of at most k 2^-23
ULP = {"sin": 4, "cos": 4, "exp": 3, "log1p": 2, "pow": 16}


def _d(name):
    return ULP[name] * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------------------
# linear_f32.hip: the launch rule, mirrored
# ------------------------------------------------------------------------------------------------------------------------------
def pick_splits(i, j, k):
    tiles = ceil_div(i, 32) * ceil_div(j, 32)
    return min(max(1, 512 // tiles), max(1, k // 64))


def kper(k, splits):
    return (ceil_div(k, splits) + 7) // 8 * 8


def used_splits(i, j, k):
    return ceil_div(k, kper(k, pick_splits(i, j, k)))


def split_lengths(i, j, k):
    """reduction length of every split that runs"""
    kp = kper(k, pick_splits(i, j, k))
    return [min(kp, k - s * kp) for s in range(ceil_div(k, kp))]


def workspace_bytes(m, n, k):
    return max(pick_splits(m, n, k) * m * n, pick_splits(m, k, n) * m * k) * 4


EPILOGUE_CAP = 1024 * 256      # elements one pass of the epilogue grid covers

# (M, N, K) of the bit-for-bit cases
TILE_SHAPES = [(1, 1, 1), (32, 4, 19), (1, 4, 19), (31, 33, 7), (33, 31, 9), (32, 32, 8), (64, 65, 16), (65, 64, 17)]
FWD_SPLIT_SHAPES = [(3, 5, 128), (3, 5, 129), (3, 5, 200), (2, 40, 4100), (5, 27, 500), (32, 500, 4096)]
DGRAD_SPLIT_SHAPES = [(4, 129, 40), (4, 200, 24), (3, 4100, 40)]
WGRAD_SHAPES = [(1, 5, 40), (7, 33, 9), (8, 5, 40), (9, 40, 5), (67, 31, 9)]
CAP_SHAPES = [(65, 4100, 8), (65, 8, 4100)]
LINEAR_SHAPES = TILE_SHAPES + FWD_SPLIT_SHAPES + DGRAD_SPLIT_SHAPES + WGRAD_SHAPES + CAP_SHAPES
# what each split case is there for: (M, N, K) -> (product, picked, lengths of the splits that run)
SPLIT_INTENT = {(3, 5, 128): ("fwd", 2, [64, 64]), (3, 5, 129): ("fwd", 2, [72, 57]), (3, 5, 200): ("fwd", 3, [72, 72, 56]),
                (2, 40, 4100): ("fwd", 64, [72] * 56 + [68]), (32, 500, 4096): ("fwd", 32, [128] * 32),
                (4, 129, 40): ("dgrad", 2, [72, 57]), (4, 200, 24): ("dgrad", 3, [72, 72, 56]),
                (3, 4100, 40): ("dgrad", 64, [72] * 56 + [68])}
ACT_SHAPES = [(33, 31, 9), (32, 64, 100), (5, 27, 500)]      # tanh and swish: one split, one split, seven


def product_dims(product, m, n, k):
    """(I, J, reduction) of the three products of one layer"""
    return {"fwd": (m, n, k), "dgrad": (m, k, n), "wgrad": (n, k, m)}[product]


# ------------------------------------------------------------------------------------------------------------------------------
# exactly summable operands of one dense layer
# ------------------------------------------------------------------------------------------------------------------------------
def make_linear_case(m, n, k, bias=True, scale=1.0, zero_pre=False, seed=0):
    """x [M][K], dy [M][N] integers in [-8, 8]; w [N][K] multiples of 1/4 in [-2, 2]; b [N] multiples of 1/8 in [-2, 2] -- drawn per
    position from a seeded generator, so a dropped, doubled or misplaced k step or tile changes the float64 answer.  scale (a power
    of two) multiplies x and b.  zero_pre plants pre == 0 where that leaves the case its purpose: a zero row of w under a zero bias
    when N >= 2, a zero row of x when M >= 2 -- never the only row, so x, w, pre - b and dw of every case keep non-zero entries
    (`assert_case_is_live`); with M = 1 or a bias the zero column of w alone plants pre == 0, and (1, 1, 1) has none."""
    assert math.frexp(scale)[0] == 0.5
    g = torch.Generator().manual_seed(7919 * seed + 131 * m + 17 * n + 3 * k + int(bias))
    c = {"m": m, "n": n, "k": k, "x": _ints(g, (m, k), -8, 8), "w": _ints(g, (n, k), -8, 8) / 4, "dy": _ints(g, (m, n), -8, 8),
         "b": _ints(g, (n,), -16, 16) / 8 if bias else None}
    for name, fill in (("x", 3.0), ("w", 0.75), ("dy", -5.0)):      # the one-element case must not draw a zero
        if c[name][0, 0] == 0:
            c[name][0, 0] = fill
    if zero_pre and n >= 2:
        c["w"][n // 2] = 0.0
        if bias:
            c["b"][n // 2] = 0.0
    if zero_pre and m >= 2:
        c["x"][m // 2] = 0.0
    c["x"] = c["x"] * scale
    if bias:
        c["b"] = c["b"] * scale
    c["units"] = {"x": scale, "w": 0.25, "b": 0.125 * scale, "dy": 1.0}
    return c


def linear_references(c, act="none"):
    """float64: pre, y, dpre, dx, dw, db for act none or relu (relu'(0) = 0)"""
    pre = c["x"] @ c["w"].t()
    if c["b"] is not None:
        pre = pre + c["b"]
    if act == "relu":
        y, dpre = pre.clamp_min(0.0), c["dy"] * (pre > 0)
    else:
        assert act == "none"
        y, dpre = pre, c["dy"]
    return {"pre": pre, "y": y, "dpre": dpre, "dx": dpre @ c["w"], "dw": dpre.t() @ c["x"], "db": dpre.sum(0)}


def assert_case_is_live(c):
    """x, w, the products' part of pre and dw (act none) all have non-zero entries, and more than the planted zeros are left: a forward
    that ignored x, or a weight gradient that dropped its only reduction step, changes an asserted value"""
    r = linear_references(c)
    prod = r["pre"] - (c["b"] if c["b"] is not None else 0.0)
    for name, t in (("x", c["x"]), ("w", c["w"]), ("pre - b", prod), ("dx", r["dx"]), ("dw", r["dw"])):
        assert (t != 0).any(), "%s of case (%d, %d, %d) is identically zero" % (name, c["m"], c["n"], c["k"])
    assert (c["x"] != 0).any(1).sum() >= max(1, c["m"] - 1) and (c["w"] != 0).any(1).sum() >= max(1, c["n"] - 1)


def assert_exactly_summable(c):
    """every operand is made of f32 numbers that are whole multiples of its unit, and for each of the three products -- forward (I = M,
    J = N, reduce K, bias joined), data gradient (I = M, J = K, reduce N) and weight gradient (I = N, J = K, reduce M) -- the sum of
    |terms| stays below 2^24 units.  |dpre| <= |dy| for act none and relu, so dy stands for dpre."""
    u = c["units"]
    for name in ("x", "w", "b", "dy"):
        if c[name] is not None:
            _assert_multiples(c[name], u[name], name)
    x, w, dy = c["x"].abs(), c["w"].abs(), c["dy"].abs()
    fwd = x @ w.t() + (c["b"].abs() if c["b"] is not None else 0.0)
    fu = min(u["x"] * u["w"], u["b"]) if c["b"] is not None else u["x"] * u["w"]
    out = {"fwd": fwd.max().item() / fu, "dgrad": (dy @ w).max().item() / (u["dy"] * u["w"]),
           "wgrad": (dy.t() @ x).max().item() / (u["dy"] * u["x"]), "bgrad": dy.sum(0).max().item() / u["dy"]}
    for kind, units in out.items():
        assert units < LIMIT, "%s: sum of |terms| is %.4g units, not below 2^24: f32 additions may round" % (kind, units)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# tanh and swish: pre bit for bit, y and dpre within 4x the distance of torch's own f32 from float64
# ------------------------------------------------------------------------------------------------------------------------------
ACT_SCALE = 2.0 ** -3          # pre = (sum of <= K products of 1/4 units) / 8 + bias / 8: steps of 1/64 across [-12, 12] and beyond
PLANTED_PRE = (20.0, -20.0, 88.0, -88.0, 100.0, -100.0)


def make_act_case(m, n, k, seed=0):
    """make_linear_case scaled by 2^-3, with a zero row of x under a bias that starts with +-20, +-88, +-100: pre takes these values"""
    assert n >= len(PLANTED_PRE) + 1
    c = make_linear_case(m, n, k, bias=True, scale=ACT_SCALE, seed=seed + 500)
    c["x"][m // 2] = 0.0
    c["b"][:len(PLANTED_PRE)] = torch.tensor(PLANTED_PRE, dtype=torch.float64)
    return c


def act_f64(pre, act):
    """float64 (y, act'(pre)) at float64 pre, in forms that neither cancel nor overflow"""
    if act == "tanh":
        y = torch.tanh(pre)
        return y, 4.0 / (torch.exp(pre) + torch.exp(-pre)) ** 2          # 1 / cosh^2: no 1 - t^2 cancellation
    assert act == "swish"
    s = torch.sigmoid(pre)
    sm = torch.sigmoid(-pre)                                              # 1 - s without the cancellation
    return pre * s, s * (1.0 + pre * sm)


def ulp_distance(got, ref64):
    """|got - ref| in ulps of the f32 format at ref (spacing 2^(e - 23), 2^-149 below the normal range); inf where got is NaN or inf, or
    non-zero where the float64 value is zero: no finite bound admits those"""
    got = got.double()
    mag = ref64.abs().clamp_min(2.0 ** -126)
    ulp = 2.0 ** (torch.floor(torch.log2(mag)) - 23)
    d = (got - ref64).abs() / ulp
    bad = ~torch.isfinite(got) | ((ref64 == 0) & (got != 0))
    return torch.where(bad, torch.full_like(d, float("inf")), d)


ACT_BODY = 12.0


def act_error_figures(y, dpre, pre, dy, act):
    """the measured figures of an activation evaluated in f32 at the f32 `pre`, against float64 of the same pre, as a dict:
      y_body, y_tail   worst ulp distance of y, over |pre| <= 12 and beyond
      g_body, g_tail   worst ulp distance of dpre = dy act'(pre), likewise
      g_abs            worst |dpre - dy act'(pre)| in units of 2^-24 |dy|: act' is of order 1, and where it has lost all its bits to
                       1 - t^2 or 1 - s (torch's f32 included) a ulp distance says little, an absolute one still does"""
    y64, g64 = act_f64(pre.double(), act)
    want = dy.double() * g64
    nz = dy != 0
    body = pre.abs() <= ACT_BODY
    worst = lambda d, sel: d[sel].max().item() if sel.any() else 0.0
    dy_, dg = ulp_distance(y, y64), ulp_distance(dpre, want)
    g_abs = torch.where(nz, (dpre.double() - want).abs() / (dy.double().abs().clamp_min(1e-300) * U), dg)      # dy == 0: dpre must be 0
    return {"y_body": worst(dy_, body), "y_tail": worst(dy_, ~body), "g_body": worst(dg, body), "g_tail": worst(dg, ~body),
            "g_abs": worst(g_abs, torch.ones_like(body))}


# worst figures of torch's own f32 forward and autograd backward on the host against float64, on the pre values of ACT_SHAPES
# (tests/test_pose_head_inputs.py measures them again and holds them to these); the kernel gets 4x
TORCH_ACT_FIGURES = {"tanh": {"y_body": 0.51, "y_tail": 0.0012, "g_body": 1.68e7, "g_tail": 1.68e7, "g_abs": 1.4},
                     "swish": {"y_body": 1.61, "y_tail": 1.62e7, "g_body": 199.0, "g_tail": 1.59e7, "g_abs": 15.8}}
ACT_MARGIN = 4.0


def act_bounds(act):
    """4x torch's figure per key.  The keys that carry weight are y_body, g_abs, tanh's y_tail (a saturated tanh must be exactly +-1)
    and swish's g_body; where torch's own figure is near 2^24 ulp (g_body and g_tail of tanh: 1 - t^2 of a t that has rounded to 1;
    y_tail and g_tail of swish: exp(-x) overflows below -88.7) the bound asks for finite values and no more."""
    return {k: ACT_MARGIN * f for k, f in TORCH_ACT_FIGURES[act].items()}


# ------------------------------------------------------------------------------------------------------------------------------
# pose cases
# ------------------------------------------------------------------------------------------------------------------------------
PI = math.pi
YAWS = [0.0, 1e-3, PI, 3 * PI + 0.1, 100.0, 1000.0, 2000.0, PI / 2, PI / 2]      # predicted yaw; the last two against gt 0 and -pi/2
YAW_GT = {7: 0.0, 8: -PI / 2}
LOGITS = [0.0, 20.0, -20.0, 50.0, -50.0, 88.0, -88.0, 100.0, -100.0]
_F = torch.float32
LOGVARS = [-30.0, torch.nextafter(torch.tensor(-30.0, dtype=_F), torch.tensor(-100.0, dtype=_F)).item(), 20.0,
           torch.nextafter(torch.tensor(20.0, dtype=_F), torch.tensor(100.0, dtype=_F)).item(), 0.0]
G9 = [1.0, 0.7, 1.3, 0.4, 2e-3, 0.0, 0.0, 0.0, 0.0]       # upstream gradient: all five loss weights non-zero


def make_prior(L, seed=0):
    """[L][3][8]: mean | var | logvar per label, f32.  Label 0 mixes variances of 1e-6 and 1e3 with ordinary ones; label 1 is all 1e-6,
    label 2 all 1e3.  logvar = log(var) as DiagonalGaussianDistribution holds it."""
    g = torch.Generator().manual_seed(77 + seed)
    mean = torch.randn(L, 8, generator=g)
    var = torch.exp(torch.randn(L, 8, generator=g))
    var[0, 1], var[0, 5] = 1e-6, 1e3
    if L > 1:
        var[1] = 1e-6
    if L > 2:
        var[2] = 1e3
    var = var.float()
    return torch.stack([mean.float(), var, torch.log(var.double()).float()], dim=1).contiguous()


def make_pose_case(name, B, NC=11, L=3, bg_idx=1, l2=False, yaw=True, gamma=2.0, alpha=0.25, fg="mixed", prior_neg=False, seed=0):
    """One batch, f32 inputs.  Rows carry, cyclically: the predicted yaws of YAWS (|sin a - sin b| exactly 1 and 2 among them), the
    logits of LOGITS in positive and negative columns, the raw log-variances of LOGVARS and two beyond the clamp, dec_pose == gt in two
    translation entries, every class id from 0 to NC (NC has no positive column).  fg: "mixed", "last" (foreground only at B - 1),
    "tail" (only at b >= 256), "none"."""
    g = torch.Generator().manual_seed(1009 * seed + 31 * B + NC)
    W = 8 + NC
    dp = (torch.randn(B, W, generator=g) * 1.5).float()
    mo = torch.randn(B, 16, generator=g).float()
    pg = (torch.randn(B, 4, generator=g) * 2).float()
    bg = torch.randn(B, 3, generator=g).float()
    fgt = torch.rand(B, generator=g).float()
    r = torch.arange(B)
    cls = (r * 5 + r // (NC + 1)) % (NC + 1)
    if fg == "none":
        cls[:] = bg_idx
    elif fg == "last":
        cls[:] = bg_idx
        cls[B - 1] = (bg_idx + 1) % (NC + 1)
    elif fg == "tail":
        cls[:256] = bg_idx
        cls[256:] = torch.where(cls[256:] == bg_idx, torch.full_like(cls[256:], (bg_idx + 1) % (NC + 1)), cls[256:])
    # -1 ("background" label) on every (L + 1)-th row, starting at row L: B = 1 keeps a prior row and runs the KL
    pidx = ((r + 1) % (L + 1)) - 1 if not prior_neg else torch.full((B,), -1)
    for b in range(B):
        s = b % 11
        if s < len(YAWS):
            dp[b, 3] = YAWS[s]
            if s in YAW_GT:
                pg[b, 3] = YAW_GT[s]
        if b % 2 == 0:
            for k in range(NC):
                dp[b, 8 + k] = LOGITS[(b // 2 + 1 + k) % len(LOGITS)]
            if int(cls[b]) < NC:
                dp[b, 8 + int(cls[b])] = LOGITS[(b // 2) % len(LOGITS)]
        if b % 3 == 0:
            lvs = LOGVARS + [25.0, -40.0]
            for i in range(8):
                mo[b, 8 + i] = lvs[(b // 3 + i) % len(lvs)]
        if b % 5 == 1:
            pg[b, 0], pg[b, 2] = dp[b, 0], dp[b, 2]
    return {"name": name, "B": B, "NC": NC, "L": L, "bg_idx": bg_idx, "l2": l2, "yaw": yaw, "gamma": gamma, "alpha": alpha,
            "dec_pose": dp, "moments": mo, "pose_gt": pg, "bbox_gt": bg, "fill_gt": fgt, "class_gt": cls.long(),
            "prior": make_prior(L, seed), "prior_idx": pidx.int()}


def _pose_cases():
    out = [make_pose_case("B%d" % b, b) for b in (1, 2, 255, 256, 257, 513, 1000)]
    out += [make_pose_case("fg_last", 257, fg="last"), make_pose_case("fg_tail", 513, fg="tail"), make_pose_case("all_bg", 37, fg="none"),
            make_pose_case("prior_neg", 37, prior_neg=True)]
    out += [make_pose_case("NC%d_L%d_bg%d" % (nc, L, bgi), 37, NC=nc, L=L, bg_idx=bgi, seed=nc)
            for nc, L, bgi in ((1, 1, 1), (1, 3, 0), (8, 3, 1), (8, 1, 0), (11, 1, 0), (40, 3, 0), (40, 1, 1))]
    out += [make_pose_case("%s_yaw%d" % ("l2" if l2 else "l1", yaw), 37, l2=l2, yaw=yaw, seed=3)
            for l2 in (False, True) for yaw in (True, False)]
    out += [make_pose_case("gamma%g_alpha%g" % (ga, al), 37, gamma=ga, alpha=al, seed=5)
            for ga in (2.0, 1.5, 1.0, 0.0) for al in (0.25, 0.5)]
    return out


POSE_CASES = _pose_cases()
EDGE_CASE = "gamma2_alpha0.25"      # B = 37, NC = 11: every listed yaw, logit and log-variance is in it (the CPU test checks)


def pose_case(name):
    return next(c for c in POSE_CASES if c["name"] == name)


# ------------------------------------------------------------------------------------------------------------------------------
# the pose terms and their Jacobians, analytic, in any dtype; faults for the rule to reject
# ------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("mask_dropped", "inv_nb_over_B", "clamp_exclusive", "focal_dpt_sign", "cross_sum_over_i", "yaw_phase")


def _pow(base, ex):
    """base ** ex with 0 ** 0 = 1, base >= 0"""
    if ex == 0.0:
        return torch.ones_like(base)
    if ex == 1.0:
        return base
    if ex == 2.0:
        return base * base
    return torch.pow(base, ex)


def pose_model(c, dtype=torch.float64, g9=G9, fault=None):
    """out [9], d_dec_pose [B][W], d_moments [B][16] for upstream gradient g9, from the formulas and their analytic derivatives.  In
    float64 (stable forms throughout) this is the reference; in float32 it is the host model of the kernel that carries the planted
    faults.  Also returns the intermediate values the acceptance rule is made from."""
    T = lambda t: t.to(dtype)
    dp, mo, pg, bg, fgt, prior = T(c["dec_pose"]), T(c["moments"]), T(c["pose_gt"]), T(c["bbox_gt"]), T(c["fill_gt"]), T(c["prior"])
    cls, pidx = c["class_gt"], c["prior_idx"].long()
    B, NC, gamma, alpha = c["B"], c["NC"], float(c["gamma"]), float(c["alpha"])
    g9 = torch.tensor(g9, dtype=dtype)
    mask = T(cls != c["bg_idx"])
    nb = mask.sum()
    inv_nb = (1.0 / nb if nb > 0 else nb * 0.0) if fault != "inv_nb_over_B" else torch.tensor(1.0 / B, dtype=dtype)
    gmask = torch.ones_like(mask) if fault == "mask_dropped" else mask
    v = {}
    # translation and yaw: t [B][4], its derivative gt [B][4]
    d = dp[:, :4] - pg
    if c["l2"]:
        t, dt = d * d, 2.0 * d
    else:
        t, dt = d.abs(), torch.sign(d)
    if c["yaw"]:
        a = dp[:, 3] * (1.0 + 1e-5) if fault == "yaw_phase" else dp[:, 3]
        sa, sb, ca = torch.sin(a), torch.sin(pg[:, 3]), torch.cos(a)
        dy_ = sa - sb
        ty = torch.where(dy_.abs() < 1.0, 0.5 * dy_ * dy_, dy_.abs() - 0.5)
        t = torch.cat([t[:, :3], ty[:, None]], 1)
        dt = torch.cat([dt[:, :3], (dy_.clamp(-1.0, 1.0) * ca)[:, None]], 1)
        v.update(sa=sa, sb=sb, ca=ca, dyaw=dy_)
    v.update(d=d, t=t)
    out = [(t.sum(1) * gmask).sum() * inv_nb]
    # focal class loss
    x = dp[:, 8:]
    tg = T(torch.arange(NC)[None, :] == cls[:, None])
    p, q = torch.sigmoid(x), torch.sigmoid(-x)                   # q = 1 - p without the cancellation
    pt, qt = q * tg + p * (1.0 - tg), p * tg + q * (1.0 - tg)    # pt and 1 - pt
    aw = alpha * tg + (1.0 - alpha) * (1.0 - tg)
    sp = torch.log1p(torch.exp(-x.abs()))
    bce = torch.clamp_min(x * (1.0 - 2.0 * tg), 0.0) + sp        # max(x, 0) - x t, t in {0, 1}
    w = _pow(pt, gamma)
    sgn = (1.0 - 2.0 * tg) * (-1.0 if fault == "focal_dpt_sign" else 1.0)
    inv_cls = 1.0 / (B * NC)
    la = aw * (1.0 - 2.0 * tg) * pt * w                           # p - t = (1 - 2t) pt, without the cancellation at t = 1
    lb = aw * bce * gamma * w * qt * sgn
    jcls = (la + lb) * inv_cls
    out.append((bce * aw * w).sum() * inv_cls)
    v.update(p=p, pt=pt, qt=qt, aw=aw, sp=sp, bce=bce, w=w, tg=tg, la=la, lb=lb)
    # box size and fill factor
    db = dp[:, 4:7] - bg
    df = dp[:, 7] - fgt
    out.append(((db * db).sum(1) * gmask).sum() * inv_nb)
    out.append((df * df * gmask).sum() * inv_nb)
    v.update(db=db, df=df)
    # KL of the box posterior against the label's prior: entry i sums the cross term over ALL prior dimensions j
    keep = T(pidx >= 0)
    pr = prior[pidx.clamp_min(0)]                                 # [B][3][8]
    pm, iv, ol = pr[:, 0], 1.0 / (pr[:, 1] + 1e-5), pr[:, 2]
    m, lv_raw = mo[:, :8], mo[:, 8:]
    lv = lv_raw.clamp(-30.0, 20.0)
    in_range = T((lv_raw > -30.0) & (lv_raw < 20.0)) if fault == "clamp_exclusive" else T((lv_raw >= -30.0) & (lv_raw <= 20.0))
    ev = torch.exp(lv)
    dm = m[:, :, None] - pm[:, None, :]                           # [B][i][j]
    l1, l2_ = dm * dm * iv[:, None, :], ev[:, :, None] * iv[:, None, :]
    kl = 0.5 * (l1 + l2_ - 1.0 - lv[:, :, None] + ol[:, None, :]).sum((1, 2))
    out.append((kl * keep).sum() * inv_nb)
    if fault == "cross_sum_over_i":
        dmean = (dm * iv[:, :, None]).sum(1)
        dlv = 0.5 * ((ev[:, None, :] * iv[:, :, None]).sum(2) - 8.0)
    else:
        dmean = (dm * iv[:, None, :]).sum(2)
        dlv = 0.5 * (l2_.sum(2) - 8.0)
    v.update(keep=keep, l1=l1, l2=l2_, lv=lv, ol=ol, dmiv=dm * iv[:, None, :], in_range=in_range, mask=mask, inv_nb=inv_nb)
    out += [t[:, i].sum() / B for i in range(4)]
    d_pose = torch.zeros(B, 8 + NC, dtype=dtype)
    d_pose[:, :4] = g9[0] * dt * gmask[:, None] * inv_nb
    d_pose[:, 4:7] = g9[2] * 2.0 * db * gmask[:, None] * inv_nb
    d_pose[:, 7] = g9[3] * 2.0 * df * gmask * inv_nb
    d_pose[:, 8:] = g9[1] * jcls
    d_mom = torch.cat([dmean, dlv * in_range], 1) * (keep * inv_nb * g9[4])[:, None]
    return torch.stack(out), d_pose, d_mom, v


def _spread(base, e, ex):
    """the most base ** ex can move when base moves by e (base, e >= 0; ex >= 0)"""
    if ex == 0.0:
        return torch.zeros_like(base)
    here, up, dn = _pow(base, ex), _pow(base + e, ex), _pow((base - e).clamp_min(0.0), ex)
    return torch.maximum(up - here, here - dn)


def pose_reference(c, g9=G9):
    """float64 out, d_dec_pose, d_moments and the bound of the acceptance rule for each of their elements (profiles/pose_head_exact.md):
    bound = errors of the leaves, first order and propagated through the formulas, + (n + r) 2^-24 sum|leaf| for the summation of n
    leaves and the r roundings behind it.  `sums` holds sum|leaf| per output, for the margins table."""
    out, d_pose, d_mom, v = pose_model(c, torch.float64, g9)
    B, NC, gamma = c["B"], c["NC"], float(c["gamma"])
    g9 = [abs(x) for x in g9]
    mask, keep, inv_nb = v["mask"], v["keep"], float(v["inv_nb"])
    nb = int(mask.sum().item())
    # --- translation / yaw leaves: value t, magnitude A, error e_t; derivative error e_dt
    d, t = v["d"], v["t"]
    if c["l2"]:
        A, e_t, e_dt = t.clone(), 3 * U * t, U * (2.0 * d).abs()
    else:
        A, e_t, e_dt = t.clone(), U * t, torch.zeros_like(t)
    if c["yaw"]:
        dy_, sa, sb, ca = v["dyaw"], v["sa"], v["sb"], v["ca"]
        e_d = _d("sin") * (sa.abs() + sb.abs()) + U * dy_.abs()
        lin = dy_.abs() >= 1.0
        A[:, 3] = torch.where(lin, dy_.abs() + 0.5, t[:, 3])
        # |dt/dd| <= min(|d|, 1); the two branches join with equal slope, so taking the other one costs 0.5 e_d^2 at the most
        e_t[:, 3] = (dy_.abs() + e_d).clamp_max(1.0) * e_d + 0.5 * e_d * e_d + 2 * U * A[:, 3]
        gy = dy_.clamp(-1.0, 1.0) * ca
        e_dt[:, 3] = e_d * ca.abs() * (1.0 + _d("cos")) + _d("cos") * gy.abs() + 2 * U * gy.abs()
    sums, bound = [], []
    sums.append((A.sum(1) * mask).sum().item() * inv_nb)
    bound.append((e_t.sum(1) * mask).sum().item() * inv_nb + (4 * nb + 2) * U * sums[-1])
    # --- focal leaves
    p, pt, qt, aw, sp, bce, w, tg = (v[k] for k in ("p", "pt", "qt", "aw", "sp", "bce", "w", "tg"))
    x_abs = c["dec_pose"][:, 8:].double().abs()
    rho_p = _d("exp") + 2 * U                                       # 1 / (1 + exp(-x)): exp, one addition, one division
    e_p = rho_p * p + ETA
    e_pt = torch.where(tg > 0, e_p + U * pt, e_p)                   # 1 - p rounds once more
    e_qt = torch.where(tg > 0, e_p, e_p + U * qt)
    # max(x, 0) - x t is exact and the log term log1p(exp(-|x|)) keeps its relative accuracy -- in that form.  The reference's torch
    # forms (1 - t) x - log_sigmoid(x), and log(1 + exp(-|x|)) is a third: a rounding at magnitude |x| + bce, or at 1, before a
    # cancellation.  The rule admits all three: two roundings at |x| + 1 + bce, absolute.
    e_bce = (_d("exp") + _d("log1p") + U) * sp + 2 * U * (x_abs + 1.0 + bce) + ETA
    d_w = U if gamma in (0.0, 1.0, 2.0) else _d("pow")
    E_w = _spread(pt, e_pt, gamma)
    E_w = E_w + d_w * (w + E_w)
    inv_cls = 1.0 / (B * NC)
    leaf = aw * bce * w
    e_leaf = aw * (e_bce * (w + E_w) + bce * E_w) + 3 * U * leaf + FLOOR
    sums.append(leaf.sum().item() * inv_cls)
    bound.append(e_leaf.sum().item() * inv_cls + (B * NC + 2) * U * sums[-1])
    # class Jacobian: La = aw (p - t) w, |p - t| = pt; Lb = aw bce d(pt^gamma)/dx in the two forms gamma w (1 - pt) and
    # gamma pt^(gamma - 1) p (1 - p): the rule admits both
    e_la = aw * (e_pt * (w + E_w) + pt * E_w) + 3 * U * v["la"].abs() + FLOOR
    if gamma == 0.0:
        e_lb = torch.zeros_like(w)
    else:
        form_a = e_bce * (w + E_w) * (qt + e_qt) + bce * E_w * (qt + e_qt) + bce * w * e_qt
        vv = _pow(pt, gamma - 1.0) if gamma >= 1.0 else None
        if vv is not None:
            E_v = _spread(pt, e_pt, gamma - 1.0)
            E_v = E_v + d_w * (vv + E_v)
            s, e_s = pt * qt, e_pt * (qt + e_qt) + pt * e_qt + U * pt * qt
            form_b = e_bce * (vv + E_v) * (s + e_s) + bce * E_v * (s + e_s) + bce * vv * e_s
            form_a = torch.maximum(form_a, form_b)
        e_lb = aw * gamma * form_a + 6 * U * v["lb"].abs() + FLOOR
    b_jcls = g9[1] * ((e_la + e_lb) * inv_cls + 4 * U * (v["la"].abs() + v["lb"].abs()) * inv_cls)
    # --- box size and fill factor
    db, df = v["db"], v["df"]
    for sq, n in ((db * db, 3), (df * df, 1)):
        s = ((sq.sum(1) if sq.dim() == 2 else sq) * mask).sum().item() * inv_nb
        sums.append(s)
        bound.append((3 + n * nb + 2) * U * s)
    # --- KL leaves
    l1, l2_, lv, ol = v["l1"], v["l2"], v["lv"], v["ol"]
    mag = 0.5 * (l1 + l2_ + 1.0 + lv.abs()[:, :, None] + ol.abs()[:, None, :]).sum((1, 2))
    e_kl = 0.5 * (7 * U * l1 + (_d("exp") + 4 * U) * l2_).sum((1, 2))
    nk = int(keep.sum().item())
    sums.append((mag * keep).sum().item() * inv_nb)
    bound.append((e_kl * keep).sum().item() * inv_nb + (40 * nk + 2) * U * sums[-1])
    for i in range(4):
        sums.append(A[:, i].sum().item() / B)
        bound.append(e_t[:, i].sum().item() / B + (B + 2) * U * sums[-1])
    # --- gradient elements
    b_pose = torch.zeros_like(d_pose)
    b_pose[:, :4] = g9[0] * mask[:, None] * inv_nb * e_dt + 4 * U * d_pose[:, :4].abs()
    b_pose[:, 4:8] = 5 * U * d_pose[:, 4:8].abs()
    b_pose[:, 8:] = b_jcls
    s_mean = v["dmiv"].abs().sum(2)
    s_lv = 0.5 * (l2_.sum(2) + 8.0)
    kin = (keep * inv_nb * g9[4])[:, None]
    b_mom = torch.cat([(8 + 6 + 3) * U * s_mean, (0.5 * (_d("exp") + 4 * U) * l2_.sum(2) + (16 + 3) * U * s_lv) * v["in_range"]], 1) * kin
    return {"out": out, "d_pose": d_pose, "d_mom": d_mom, "out_bound": torch.tensor(bound, dtype=torch.float64),
            "d_pose_bound": b_pose, "d_mom_bound": b_mom, "sums": torch.tensor(sums, dtype=torch.float64)}


OUT_NAMES = ("pose", "class", "bbox", "fill", "kl_bbox", "t1_mean", "t2_mean", "t3_mean", "v3_mean")


def rule_margins(ref, out, d_pose, d_mom):
    """worst |err| / bound per output and per group of gradient elements (yaw column, class columns, the other columns of d dec_pose;
    d moments).  0 / 0 counts as 0; any error over a zero bound, NaN and inf count as inf."""
    def ratio(got, want, bound):
        got = got.detach().cpu().double()
        err = (got - want).abs()
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
        r = torch.where(err == 0, torch.zeros_like(r), r)
        return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    m = {name: ratio(out, ref["out"], ref["out_bound"])[i].item() for i, name in enumerate(OUT_NAMES)}
    rp = ratio(d_pose, ref["d_pose"], ref["d_pose_bound"])
    m["d_pose_yaw"], m["d_pose_class"] = rp[:, 3].max().item(), rp[:, 8:].max().item()
    m["d_pose_rest"] = torch.cat([rp[:, :3], rp[:, 4:8]], 1).max().item()
    m["d_mom"] = ratio(d_mom, ref["d_mom"], ref["d_mom_bound"]).max().item()
    return m


def rule_failures(ref, out, d_pose, d_mom):
    return {k: r for k, r in rule_margins(ref, out, d_pose, d_mom).items() if not r <= 1.0}


def assert_rule(ref, out, d_pose, d_mom, what):
    bad = rule_failures(ref, out, d_pose, d_mom)
    assert not bad, "%s: |err| / bound over 1 for %s" % (what, bad)
