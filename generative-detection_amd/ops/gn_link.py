"""What travels between a conv and the GroupNorm beside it: statistics of a conv's output for the GroupNorm that reads it
(`_gn_partials`), and the link through which a conv's data gradient leaves the first pass of that GroupNorm's backward."""
import torch

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from ._base import BF16, _L, _stamp, _stamped


GN_GROUPS = 32      # Normalize() of the reference model: GroupNorm(32, C, eps 1e-6)


class _GnBwdLink:
    """What the consumer conv's data gradient needs of the GroupNorm in front of it, and where it leaves the sums.  `out` identifies the
    GroupNorm's output the way _gn_partials identifies a conv's (_stamp).  The GroupNorm's operands are NOT held here:
    `node` is a weak reference to its autograd context, whose saved tensors (x, gamma, beta, mean, rstd) the conv's backward reads -- through
    the saved-tensor hooks, so an activation-checkpointed unit recomputes them instead of this link keeping the first forward's alive."""
    __slots__ = ("node", "groups", "out", "sums")

    def __init__(self):
        self.node = self.out = self.sums = None
        self.groups = 0

    def operands(self):
        """(x, mean, rstd, gamma, beta) of the GroupNorm, or None if its node is gone."""
        ctx = self.node() if self.node is not None else None
        if ctx is None:
            return None
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        return x, mean, rstd, gamma.detach().contiguous(), beta.detach().contiguous()

    def take_sums(self, dy):
        """The sums, if they were made from exactly this gradient tensor (else None); single use."""
        sums, self.sums = self.sums, None
        if sums is None:
            return None
        p, stamp = sums
        return p if _stamped(dy, stamp) else None


def _gn_bwd_link_of(a, cin):
    """The link a swish-GroupNorm left on this very tensor (f32, 32 groups), if `a` still holds that GroupNorm's output."""
    link = getattr(a, "_gn_bwd_link", None)
    if link is None or not _ops.GN_FUSED_BWD or not _stamped(a, link.out) or a.shape[1] != cin:
        return None
    return link


def _gn_stats_ok(cout):
    cpg = cout // GN_GROUPS
    return _ops.GN_FUSED_STATS and cout % GN_GROUPS == 0 and 1 <= cpg <= 32 and (cpg & (cpg - 1)) == 0


def _tag_gn_partials(y, partial):
    """The statistics are valid for exactly these values of y: the stamp lets the consumer (_gn_partials_of) tell whether anything wrote
    to the tensor in between."""
    if partial is not None:
        y._gn_partials = (partial, _stamp(y))
    return y


def _gn_partials_of(x, groups):
    """Statistics the producing conv attached to this very tensor object (ops.conv3x3(gn_stats=True)), if they fit."""
    tagged = getattr(x, "_gn_partials", None)
    if tagged is None or not _ops.GN_FUSED_STATS or groups != GN_GROUPS:
        return None
    p, stamp = tagged
    if not _stamped(x, stamp) or p.device != x.device:
        return None      # the tensor was written to (or is not the conv's output any more): take the statistics pass
    n, _, h, w = x.shape
    chunks = _L().odvae_conv_bf16_stats_chunks(h, w) if x.dtype == BF16 else _L().odvae_conv3x3_wino4_stats_chunks(h, w)
    if p.shape[0] != n or p.shape[2] != groups or p.shape[1] != chunks:
        return None
    return p


def _f32_gn_link(x, groups, swish):
    ok = _ops.GN_FUSED_BWD and not _ops.GN_FUSED_BWD_SUSPENDED and swish and groups == GN_GROUPS and torch.is_grad_enabled() and x.requires_grad
    return _GnBwdLink() if ok else None


class gn_fused_bwd_suspended:
    """Context manager: no GroupNorm-backward links for the forward calls inside (activation-checkpointed units)."""

    def __enter__(self):
        _ops.GN_FUSED_BWD_SUSPENDED += 1

    def __exit__(self, *exc):
        _ops.GN_FUSED_BWD_SUSPENDED -= 1
        return False


def _tag_gn_output(y, link):
    if link is not None and link.node is not None:
        link.out = _stamp(y)
        y._gn_bwd_link = link
    return y
