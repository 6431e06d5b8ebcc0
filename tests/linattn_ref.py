"""Linear attention ([UPSTREAM] ldm/modules/attention.py LinearAttention as model.py's LinAttnBlock builds it: dim = C, heads = 1,
dim_head = C): the torch restatement, float64 / host-f32 references with gradients by autograd, input generators, a host model of the
kernels' formulation with faults that can be planted in it, and the acceptance rule (tests/gn_offset_inputs.py: `figure`, `check`):

    |q_hip - q_64|max  <=  max( 8 |q_torch_f32 - q_64|max ,  floor * max(1, |q_64|max) )

with FLOOR_FWD for outputs, ctx and the column statistics, FLOOR_DX for dqkv / dx, FLOOR_PARAM for weight and bias gradients.
Plain module: no fixtures, no device.  q, k, v are [N, C, T] on the host (channel d, token n), ctx is [N, C, C] (ctx[d][e]).
"""
import torch
import torch.nn as nn

from gn_offset_inputs import FLOOR_DX, FLOOR_FWD, FLOOR_PARAM, check, figure, inside   # noqa: F401  (re-exported: the rule)

OFFSETS = (0, 30, 90)


# ------------------------------------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------------------------------------
def core(q, k, v):
    """(out [N, C, T], ctx [N, C, C]): k softmaxed over the T tokens per (image, channel); ctx[d][e] = sum_n k[d][n] v[e][n];
    out[e][n] = sum_d ctx[d][e] q[d][n].  No scale, no softmax over q."""
    ks = k.softmax(dim=-1)
    ctx = torch.einsum("bdn,ben->bde", ks, v)
    return torch.einsum("bde,bdn->ben", ctx, q), ctx


class LinAttnBlock(nn.Module):
    """The reference module: to_qkv = Conv2d(C, 3C, 1, bias=False), to_out = Conv2d(C, C, 1); no norm, no residual."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.to_qkv = nn.Conv2d(in_channels, 3 * in_channels, 1, bias=False)
        self.to_out = nn.Conv2d(in_channels, in_channels, 1)

    def forward(self, x):
        b, c, h, w = x.shape
        q, k, v = self.to_qkv(x).reshape(b, 3, c, h * w).unbind(1)        # channels [0, C), [C, 2C), [2C, 3C)
        out, _ = core(q, k, v)
        return self.to_out(out.reshape(b, c, h, w))


def linearize(net):
    """Replaces every AttnBlock of an oracle Encoder / Decoder (oracle/ldm_model.py) by a reference LinAttnBlock of the same width: the
    torch counterpart of Encoder / Decoder(use_linear_attn=True).  Returns net."""
    def swap(holder, name):
        old = getattr(holder, name) if isinstance(name, str) else holder[name]
        new = LinAttnBlock(old.in_channels)
        if isinstance(name, str):
            setattr(holder, name, new)
        else:
            holder[name] = new
    swap(net.mid, "attn_1")
    for stage in (net.down if hasattr(net, "down") else net.up):
        for i in range(len(stage.attn)):
            swap(stage.attn, i)
    return net


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ------------------------------------------------------------------------------------------------------------------------------
def seed_of(n, c, t, a=0, salt=0):
    return (1000003 * salt + 7919 * int(a) + 31 * n + 17 * c + t) % (2 ** 31 - 1)


def channel_signs(c):
    return (1.0 - 2.0 * (torch.arange(c) % 2)).float()


def make_qkv(n, c, t, offset=0.0, seed=None):
    """(q, k, v, d_out) f32 [N, C, T]: randn; k = randn + offset * sign_d with the sign alternating from one channel to the next."""
    g = torch.Generator().manual_seed(seed_of(n, c, t, offset) if seed is None else seed)
    q, k, v, do = (torch.randn(n, c, t, generator=g) for _ in range(4))
    return q, (k + offset * channel_signs(c).view(1, c, 1)).float(), v, do


def hw_of(t):
    """(H, W) with H * W = t, as square as t allows"""
    h = max(d for d in range(1, int(t ** 0.5) + 1) if t % d == 0)
    return h, t // h


def pack(q, k, v):
    """[N, 3C, H, W]: the packed projection to_qkv would have produced"""
    n, c, t = q.shape
    h, w = hw_of(t)
    return torch.cat([q, k, v], dim=1).reshape(n, 3 * c, h, w)


def core_refs(q, k, v, do):
    """{64: dict, 32: dict} with out, ctx, m, rinv, dq, dk, dv: float64 and torch f32 on the host, gradients by autograd."""
    res = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        qr, kr, vr = (t.detach().to(dt).clone().requires_grad_(True) for t in (q, k, v))
        out, ctx = core(qr, kr, vr)
        out.backward(do.to(dt))
        m = kr.detach().max(dim=-1).values
        rinv = 1.0 / (kr.detach() - m.unsqueeze(-1)).exp().sum(-1)
        res[bits] = dict(out=out.detach(), ctx=ctx.detach(), m=m, rinv=rinv, dq=qr.grad, dk=kr.grad, dv=vr.grad)
    return res


def host_model(q, k, v, do, fault=None):
    """The kernels' formulation in f32 on the host: column maximum m and 1 / l, ctx = (exp(k - m)^T v) / l, out = q ctx; backward
    dctx = q^T dOut, dq = dOut ctx^T, g[d] = ctx[d] . dctx[d], s = exp(k - m) / l, dv = s dctx, dk = s (v dctx^T - g).
    fault: None, or one of FAULTS planted into it."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    c = q.shape[1]
    if fault == "permuted_thirds":
        q, k, v = k, v, q
    m = k.max(dim=-1, keepdim=True).values
    if fault == "no_max_subtraction":
        m = torch.zeros_like(m)
    e = (k - m).exp()
    rinv = 1.0 / e.sum(-1, keepdim=True)
    s = e * rinv
    if fault == "softmax_over_channels":
        s = k.softmax(dim=1)
    ctx = torch.einsum("bdn,ben->bde", s, v)
    if fault == "scaled":
        ctx = ctx * float(c) ** -0.5
    out = torch.einsum("bde,bdn->ben", ctx, q)
    dctx = torch.einsum("bdn,ben->bde", q, do)
    dq = torch.einsum("bde,ben->bdn", ctx, do)
    g = (ctx * dctx).sum(-1, keepdim=True)
    dv = torch.einsum("bdn,bde->ben", s, dctx)
    u = torch.einsum("ben,bde->bdn", v, dctx)
    dk = s * (u if fault == "g_dropped" else u - g)
    return dict(out=out, ctx=ctx, m=m.squeeze(-1), rinv=rinv.squeeze(-1), dq=dq, dk=dk, dv=dv)


FAULTS = ("softmax_over_channels", "permuted_thirds", "scaled", "no_max_subtraction", "g_dropped")


def core_figures(got, refs):
    """The rule's figures for a dict as host_model returns it (tensors on any device) against core_refs' references."""
    r64, r32 = refs[64], refs[32]
    figs = [figure(name, got[name], r64[name], r32[name], FLOOR_FWD) for name in ("out", "ctx", "m")]
    # 1 / l in units of the exact value, as the GroupNorm rule treats rstd
    figs.append(figure("rinv / rinv64", got["rinv"].detach().cpu().double() / r64["rinv"], torch.ones_like(r64["rinv"]),
                       r32["rinv"].double() / r64["rinv"], FLOOR_FWD))
    figs += [figure(name, got[name], r64[name], r32[name], FLOOR_DX) for name in ("dq", "dk", "dv")]
    return figs


def module_refs(block, x, dy):
    """{64: (y, dx, {param: grad}), 32: (...)} of a reference LinAttnBlock (its parameters as they are) by autograd."""
    import copy
    res = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        b = copy.deepcopy(block).to(dt)
        xr = x.detach().to(dt).clone().requires_grad_(True)
        y = b(xr)
        y.backward(dy.to(dt))
        res[bits] = (y.detach(), xr.grad, {k: p.grad for k, p in b.named_parameters()})
    return res
