"""GroupNorm (+ swish, + dropout) in f32 and bf16, and the "norm" activation-checkpoint policy that re-makes its output."""
import collections
import weakref

import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .gn_link import _f32_gn_link, _gn_partials_of, _tag_gn_output


# ------------------------------------------------------------------------------------------------------
# GroupNorm (+ swish)
# ------------------------------------------------------------------------------------------------------
# Per-dtype description of the GroupNorm Functions: dtype, bytes per element, entry points (by name), the suffix of their error labels
# (the *_drop entry points: the ResnetBlock dropout forms, which take (p, seed) behind `swish`)
_GnKind = collections.namedtuple("_GnKind", "dtype esz fwd fwd_partials bwd bwd_partials workspace suffix fwd_drop fwd_partials_drop bwd_drop")
_GN_F32 = _GnKind(torch.float32, 4.0, "odvae_groupnorm_fwd_f32", "odvae_groupnorm_fwd_partials_f32", "odvae_groupnorm_bwd_f32",
                  "odvae_groupnorm_bwd_partials_f32", "odvae_groupnorm_workspace_bytes", "",
                  "odvae_groupnorm_fwd_drop_f32", "odvae_groupnorm_fwd_partials_drop_f32", "odvae_groupnorm_bwd_drop_f32")
# (statistics and arithmetic in f32, one rounding on the way out; no GroupNorm-backward link: bwd_partials is f32 only)
_GN_BF16 = _GnKind(BF16, 2.0, "odvae_groupnorm_fwd_bf16", "odvae_groupnorm_fwd_partials_bf16", "odvae_groupnorm_bwd_bf16",
                   None, "odvae_groupnorm_bf16_workspace_bytes", "_bf16",
                   "odvae_groupnorm_fwd_drop_bf16", "odvae_groupnorm_fwd_partials_drop_bf16", "odvae_groupnorm_bwd_drop_bf16")


def _gn_forward(kind, ctx, x, gamma, beta, groups, eps, swish, with_skip, partials, link=None, drop=None):
    """partials [N][chunks][groups][2]: the statistics of x as the conv that produced it left them (ops.conv3x3(gn_stats=True)):
    no statistics pass.  link (_GnBwdLink, f32 with swish only): filled here for the conv that reads the result (GN_FUSED_BWD).
    drop (p, seed) or None: the ResnetBlock dropout on the result (group_norm(drop_p=, drop_seed=)); the statistics are those of x
    either way, so `partials` stay usable."""
    L = _L()
    x = _cl(x, kind.dtype)
    n, c, h, w = x.shape
    g = gamma.detach().contiguous()
    b = beta.detach().contiguous()
    y = _new_cl(n, c, h, w, x, dtype=kind.dtype)
    mean = torch.empty(n, groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n, groups, dtype=torch.float32, device=x.device)
    tag = KERNEL_EVENTS.begin(secondary=True)
    have_partials = partials is not None and partials.shape[0] == n and partials.shape[2] == groups
    if drop is not None and have_partials:
        _lib.check(getattr(L, kind.fwd_partials_drop)(x.data_ptr(), n, h * w, c, groups, g.data_ptr(), b.data_ptr(), float(eps), int(swish),
                                                      drop[0], drop[1], y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), partials.data_ptr(),
                                                      int(partials.shape[1]), _lib.stream_ptr()), "groupnorm_fwd_partials_drop" + kind.suffix)
    elif drop is not None:
        wp, wn = _ws(getattr(L, kind.workspace)(n, h * w, c, groups), x)
        _lib.check(getattr(L, kind.fwd_drop)(x.data_ptr(), n, h * w, c, groups, g.data_ptr(), b.data_ptr(), float(eps), int(swish),
                                             drop[0], drop[1], y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), wp, wn, _lib.stream_ptr()),
                   "groupnorm_fwd_drop" + kind.suffix)
    elif have_partials:
        _lib.check(getattr(L, kind.fwd_partials)(x.data_ptr(), n, h * w, c, groups, g.data_ptr(), b.data_ptr(), float(eps), int(swish),
                                                 y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), partials.data_ptr(),
                                                 int(partials.shape[1]), _lib.stream_ptr()), "groupnorm_fwd_partials" + kind.suffix)
    else:
        wp, wn = _ws(getattr(L, kind.workspace)(n, h * w, c, groups), x)
        _lib.check(getattr(L, kind.fwd)(x.data_ptr(), n, h * w, c, groups, g.data_ptr(), b.data_ptr(), float(eps), int(swish),
                                        y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), wp, wn, _lib.stream_ptr()), "groupnorm_fwd" + kind.suffix)
    # algorithmic traffic: x read once, y written once
    KERNEL_EVENTS.end("groupnorm", 0.0, tag, kind.esz * 2 * n * h * w * c, issued=0.0)
    ctx.groups, ctx.swish = groups, int(swish)
    ctx.drop = drop      # two host scalars: the backward (and the "norm" policy's re-make) rebuild the mask from them
    ctx.save_for_backward(x, gamma, beta, mean, rstd)
    ctx.set_materialize_grads(False)   # an unused output's gradient stays None instead of a tensor of zeros
    ctx.link = None
    if link is not None and swish:
        link.node, link.groups = weakref.ref(ctx), groups
        ctx.link = link
    if with_skip:
        return y, x.view_as(x)   # the skip connection's handle on x: its gradient comes back into this node
    return y


def _gn_backward(kind, ctx, dy, dskip):
    """(dx, dgamma, dbeta)."""
    L = _L()
    x, gamma, beta, mean, rstd = ctx.saved_tensors
    if dy is None:               # only the skip branch carried a gradient
        return dskip, None, None
    dy = _cl(dy, kind.dtype)
    sums = ctx.link.take_sums(dy) if ctx.link is not None else None
    if dskip is not None:
        dskip = _cl(dskip, kind.dtype)
    n, c, h, w = x.shape
    dx = _new_cl(n, c, h, w, x, dtype=kind.dtype)
    dg = torch.empty(c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device)
    g = gamma.detach().contiguous()
    b = beta.detach().contiguous()
    wp, wn = _ws(getattr(L, kind.workspace)(n, h * w, c, ctx.groups), x)
    tag = KERNEL_EVENTS.begin(secondary=True)
    if ctx.drop is not None:     # dy_eff = dy * keep * scale inside the reduce and apply kernels (no link was made: sums is None)
        _lib.check(getattr(L, kind.bwd_drop)(x.data_ptr(), dy.data_ptr(), n, h * w, c, ctx.groups, g.data_ptr(),
                                             b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ctx.swish, ctx.drop[0], ctx.drop[1],
                                             dx.data_ptr(), dg.data_ptr(), db.data_ptr(), _lib.ptr(dskip), wp, wn, _lib.stream_ptr()),
                   "groupnorm_bwd_drop" + kind.suffix)
    elif sums is not None:       # the data-gradient launch that made dy left the first pass's sums: finalize + apply only
        _ops.GN_FUSED_BWD_HITS += 1
        _lib.check(getattr(L, kind.bwd_partials)(x.data_ptr(), dy.data_ptr(), n, h * w, c, ctx.groups, g.data_ptr(),
                                                 b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ctx.swish, dx.data_ptr(),
                                                 dg.data_ptr(), db.data_ptr(), _lib.ptr(dskip), sums.data_ptr(), int(sums.shape[1]),
                                                 wp, wn, _lib.stream_ptr()), "groupnorm_bwd_partials")
    else:
        _lib.check(getattr(L, kind.bwd)(x.data_ptr(), dy.data_ptr(), n, h * w, c, ctx.groups, g.data_ptr(),
                                        b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ctx.swish, dx.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), _lib.ptr(dskip), wp, wn, _lib.stream_ptr()),
                   "groupnorm_bwd" + kind.suffix)
    # algorithmic traffic: x, dy (and the folded skip gradient) read once, dx written once
    KERNEL_EVENTS.end("groupnorm", 0.0, tag, kind.esz * (3 + (dskip is not None)) * n * h * w * c, issued=0.0)
    return dx, dg, db


class _GroupNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, swish, with_skip=False, partials=None, link=None, drop=None):
        return _gn_forward(_GN_F32, ctx, x, gamma, beta, groups, eps, swish, with_skip, partials, link, drop)

    @staticmethod
    def backward(ctx, dy, dskip=None):
        return _gn_backward(_GN_F32, ctx, dy, dskip) + (None,) * 7


class _GroupNormB(Function):
    """GroupNorm(+swish) on bf16 activations: statistics and arithmetic in f32, one rounding on the way out."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, swish, with_skip=False, partials=None, drop=None):
        return _gn_forward(_GN_BF16, ctx, x, gamma, beta, groups, eps, swish, with_skip, partials, None, drop)

    @staticmethod
    def backward(ctx, dy, dskip=None):
        return _gn_backward(_GN_BF16, ctx, dy, dskip) + (None,) * 6


def _gn_drop(drop_p, drop_seed):
    """(p, seed) as the entry points take them, or None for no dropout."""
    p = float(drop_p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (drop_p,))
    if p == 0.0:
        return None
    if drop_seed is None:
        raise ValueError("group_norm(drop_p > 0) needs drop_seed: the mask is a function of (seed, element index, p)")
    return p, int(drop_seed) & 0xFFFFFFFFFFFFFFFF


def group_norm(x, gamma, beta, groups=32, eps=1e-6, swish=False, drop_p=0.0, drop_seed=None):
    """drop_p > 0: the ResnetBlock dropout on the result, y = keep * scale * act(GroupNorm(x)) with the mask of dropout_mask.py made from
    (drop_seed, element index, drop_p) inside the apply pass; the backward re-makes it.  Such a call leaves no GroupNorm-backward link for
    the conv that reads y (the sums of its data-gradient epilogue know nothing of the mask) and its backward is the two-kernel form."""
    drop = _gn_drop(drop_p, drop_seed)
    if drop is not None:
        if x.dtype == BF16:
            return _GroupNormB.apply(x, gamma, beta, groups, eps, swish, False, _gn_partials_of(x, groups), drop)
        return _GroupNorm.apply(x, gamma, beta, groups, eps, swish, False, _gn_partials_of(x, groups), None, drop)
    if x.dtype == BF16:
        return _GroupNormB.apply(x, gamma, beta, groups, eps, swish, False, _gn_partials_of(x, groups))
    link = _f32_gn_link(x, groups, swish)
    return _tag_gn_output(_GroupNorm.apply(x, gamma, beta, groups, eps, swish, False, _gn_partials_of(x, groups), link), link)


def group_norm_skip(x, gamma, beta, groups=32, eps=1e-6, swish=False):
    """(GroupNorm(x), x): the second output is x itself, to be used by the block's skip connection (`x + h`).  Its
    gradient returns into this node and is summed into dx inside the GroupNorm backward pass (one pass instead of
    autograd's separate 3-pass add)."""
    if x.dtype == BF16:
        return _GroupNormB.apply(x, gamma, beta, groups, eps, swish, True, _gn_partials_of(x, groups))
    link = _f32_gn_link(x, groups, swish)
    y, skip = _GroupNorm.apply(x, gamma, beta, groups, eps, swish, True, _gn_partials_of(x, groups), link)
    return _tag_gn_output(y, link), skip


# "norm" activation-checkpoint policy: the tensor a = act(GroupNorm(x)) is NOT kept for the backward of the conv that consumes it; that conv's
# saved input is replaced (saved-tensor hooks) by what it takes to re-make it -- x, mean, rstd, gamma, beta -- and one apply pass rebuilds it when
# the conv's backward asks for its saved tensors.  Against the unit policy (torch.utils.checkpoint around a whole ResnetBlock) nothing but the
# GroupNorm apply is recomputed: no conv, no attention forward runs twice.
def group_norm_apply(x, gamma, beta, mean, rstd, groups, swish, drop=None):
    """act(GroupNorm(x)) from a forward call's statistics (no autograd): the recompute of the "norm" policy.  drop: the forward call's
    (p, seed) -- the same mask again."""
    L = _L()
    x = _cl(x, x.dtype if x.dtype == BF16 else torch.float32)
    n, c, h, w = x.shape
    y = _new_cl(n, c, h, w, x, dtype=x.dtype)
    if drop is not None:
        fn = L.odvae_groupnorm_apply_drop_bf16 if x.dtype == BF16 else L.odvae_groupnorm_apply_drop_f32
        _lib.check(fn(x.data_ptr(), n, h * w, c, int(groups), gamma.detach().contiguous().data_ptr(), beta.detach().contiguous().data_ptr(),
                      mean.data_ptr(), rstd.data_ptr(), int(swish), drop[0], drop[1], y.data_ptr(), _lib.stream_ptr()), "groupnorm_apply_drop")
        return y
    fn = L.odvae_groupnorm_apply_bf16 if x.dtype == BF16 else L.odvae_groupnorm_apply_f32
    _lib.check(fn(x.data_ptr(), n, h * w, c, int(groups), gamma.detach().contiguous().data_ptr(), beta.detach().contiguous().data_ptr(),
                  mean.data_ptr(), rstd.data_ptr(), int(swish), y.data_ptr(), _lib.stream_ptr()), "groupnorm_apply")
    return y


class _RemakeFromNorm:
    __slots__ = ("x", "gamma", "beta", "mean", "rstd", "groups", "swish", "drop")

    def __init__(self, node):
        self.x, self.gamma, self.beta, self.mean, self.rstd = node.saved_tensors
        self.groups, self.swish, self.drop = node.groups, node.swish, getattr(node, "drop", None)

    def make(self):
        with torch.no_grad():
            return group_norm_apply(self.x, self.gamma, self.beta, self.mean, self.rstd, self.groups, self.swish, self.drop)


class remake_from_norm(torch.autograd.graph.saved_tensors_hooks):
    """with remake_from_norm(a): y = conv(a) -- `a` must be the output of ops.group_norm / group_norm_skip (its grad_fn holds x, mean, rstd)."""

    def __init__(self, a):
        node = a.grad_fn
        ok = node is not None and hasattr(node, "groups") and hasattr(node, "swish") and len(getattr(node, "saved_tensors", ())) == 5
        key = (a.data_ptr(), tuple(a.shape), a.dtype) if ok else None
        recipe = _RemakeFromNorm(node) if ok else None

        def pack(t):
            if key is not None and t.data_ptr() == key[0] and tuple(t.shape) == key[1] and t.dtype == key[2]:
                return recipe
            return t

        def unpack(obj):
            return obj.make() if isinstance(obj, _RemakeFromNorm) else obj

        super().__init__(pack, unpack)
