"""BatchNorm inputs whose channel means lie far from zero: generators, references, host models.

The channel counterpart of `gn_offset_inputs` for the PatchGAN's BatchNorm2d + LeakyReLU(0.2) (csrc/gan_norm.hip).  The PatchGAN
convolutions in front of BatchNorm have no bias and read LeakyReLU outputs, so nothing centres their channel means.  `make_input`
gives x = s (randn + r sign_c) with the sign alternating from one channel to the next; `ref64` / `ref32` are `F.batch_norm` in
training mode (momentum 0.1, unbiased running variance) followed by `F.leaky_relu(., 0.2)` in float64 and in torch f32 on the host;
`two_pass_f32` is a centred f32 evaluation and `one_pass_model` the uncentred design the statistics kernel had: per thread a
sequential f32 sum of x and of fl(x x), an f64 combine, var = E[x^2] - E[x]^2.  The acceptance rule, its factor and its floors are
those of `gn_offset_inputs` and are used from there.
Plain module: no fixtures, no device.  All tensors are NCHW on the host.
"""
import numpy as np
import torch
import torch.nn.functional as F

import gn_offset_inputs as G

EPS = 1e-5                # torch.nn.BatchNorm2d's default, what the discriminator uses
MOMENTUM = 0.1
SLOPE = 0.2
RUNGS = G.RUNGS

# (n, c, h, w) and what each reaches in bn_colstats_kernel
SHAPES = [(3, 128, 6, 5),       # the shape of test_batchnorm_lrelu
          (2, 64, 16, 16),      # 4 row lanes, 4 statistics blocks
          (4, 512, 3, 3),       # the loop over 256 channels runs twice, 36 rows
          (2, 96, 9, 7),        # 64 idle threads
          (1, 320, 5, 5),       # ragged second pass of 64 channels
          (1, 64, 2, 1),        # two rows
          (1, 32, 401, 1)]      # 401 rows in 3 blocks of 134, last ragged
MODEL_SHAPES = SHAPES[:4]       # where the one-pass model has to be rejected from r = 64 on


def shape_id(s):
    return "x".join(map(str, s))


def channel_signs(c):
    """[c]: +1 for even channels, -1 for odd ones"""
    return (1.0 - 2.0 * (torch.arange(c) % 2)).float()


def make_input(shape, r, s, seed=None):
    """x = s (randn + r sign_c), f32 [n, c, h, w]; seeded per case"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(G.seed_of(shape, r, s, 17) if seed is None else seed)
    return (s * (torch.randn(n, c, h, w, generator=g) + r * channel_signs(c).view(1, c, 1, 1))).float()


def affine(c, seed=11):
    g = torch.Generator().manual_seed(seed + c)
    return torch.randn(c, generator=g), torch.randn(c, generator=g)


def running_start(c, seed=13):
    g = torch.Generator().manual_seed(seed + c)
    return 0.1 * torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5


def rows_of(x):
    """[n h w, c]: the matrix the kernels walk (NHWC flattened)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def stats64(x, eps=EPS):
    """(mean, var, rstd) [c] in float64 of the values x holds; var is the biased one"""
    v = rows_of(x.double())
    var = v.var(0, unbiased=False)
    return v.mean(0), var, 1.0 / torch.sqrt(var + eps)


def realised_ratio(x):
    v = rows_of(x.double())
    return v.mean(0).abs() / v.std(0, unbiased=False)


def _reference(x, gamma, beta, running_mean, running_var, dt, eps):
    rm = None if running_mean is None else running_mean.to(dt).clone()
    rv = None if running_var is None else running_var.to(dt).clone()
    y = F.batch_norm(x.to(dt), rm, rv, None if gamma is None else gamma.to(dt), None if beta is None else beta.to(dt), True, MOMENTUM, eps)
    return F.leaky_relu(y, SLOPE), rm, rv


def ref64(x, gamma=None, beta=None, running_mean=None, running_var=None, eps=EPS):
    """(y, running_mean, running_var) in float64, the running estimates after one training step"""
    return _reference(x, gamma, beta, running_mean, running_var, torch.float64, eps)


def ref32(x, gamma=None, beta=None, running_mean=None, running_var=None, eps=EPS):
    """torch f32 on the host: (y, running_mean, running_var, mean, rstd), the statistics as torch.native_batch_norm saves them"""
    y, rm, rv = _reference(x, gamma, beta, running_mean, running_var, torch.float32, eps)
    _, mean, rstd = torch.native_batch_norm(x.float().contiguous(), None, None, None, None, True, MOMENTUM, eps)
    return y, rm, rv, mean, rstd


def eval_refs(x, gamma, beta, mean, var, eps=EPS):
    """{64: y, 32: y}: eval-mode BatchNorm + LeakyReLU with the given running estimates (f32 tensors)"""
    out = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        y = F.batch_norm(x.to(dt), mean.to(dt), var.to(dt), gamma.to(dt), beta.to(dt), False, MOMENTUM, eps)
        out[bits] = F.leaky_relu(y, SLOPE)
    return out


def preact64(x, gamma, beta, running=None, eps=EPS):
    """u = BatchNorm(x) before the activation, float64; running = (mean, var) selects eval mode"""
    rm, rv = (None, None) if running is None else (running[0].double(), running[1].double())
    return F.batch_norm(x.double(), rm, rv, gamma.double(), beta.double(), running is None, MOMENTUM, eps)


KINK = 2e-3     # ten times the project's forward tolerance


def kink_free_dy(u64, seed):
    """randn, but 0 where |u_64| < KINK: LeakyReLU's derivative jumps from 0.2 to 1 at u = 0, so where u lies within the forward's own
    tolerance of 0 neither slope is wrong, and a gradient passing there would test the sign of a rounding error"""
    dy = torch.randn(u64.shape, generator=torch.Generator().manual_seed(seed))
    return dy * (u64.abs() >= KINK).float()


def backward_refs(x, gamma, beta, dy, running=None, eps=EPS):
    """{64: (dx, dgamma, dbeta), 32: (...)} by autograd in float64 and in f32 on the host; training mode, or eval mode with
    running = (mean, var)"""
    out = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        xr, gr, br = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        rm, rv = (None, None) if running is None else (running[0].to(dt), running[1].to(dt))
        F.leaky_relu(F.batch_norm(xr, rm, rv, gr, br, running is None, MOMENTUM, eps), SLOPE).backward(dy.to(dt))
        out[bits] = (xr.grad, gr.grad, br.grad)
    return out


def normalise(x, mean, rstd):
    """(x - mean) rstd in float64 with the given statistics [c]: what an exact apply pass makes of them"""
    c = x.shape[1]
    return (x.double() - mean.double().view(1, c, 1, 1)) * rstd.double().view(1, c, 1, 1)


def two_pass_f32(x, eps=EPS):
    """(mean, rstd) by a centred evaluation in f32 throughout"""
    v = rows_of(x.float())
    mean = v.mean(0, keepdim=True)
    var = ((v - mean) ** 2).mean(0)
    return mean.squeeze(0), 1.0 / torch.sqrt(var + np.float32(eps))


def launch_geometry(rows, c):
    """(rows per block, row lanes) of bn_colstats_kernel: clamp(rows / 128, 1, 1024) blocks, 256 / min(c, 256) row lanes per block"""
    nblk = min(max(rows // 128, 1), 1024)
    return -(-rows // nblk), 256 // min(c, 256)


def one_pass_model(x, eps=EPS):
    """(mean, rstd) the way the uncentred statistics kernel formed them: thread (row lane, channel) of a block adds its rows -- every
    `lanes`-th of the block's -- SEQUENTIALLY in f32, x and fl(x x) (numpy's cumulative sum adds in order, in the array's own type);
    all partials are combined in float64; var = max(b / m - mu mu, 0)."""
    v = rows_of(x.float()).contiguous().numpy()
    rows, c = v.shape
    rpb, lanes = launch_geometry(rows, c)
    a, b = np.zeros(c), np.zeros(c)
    for r0 in range(0, rows, rpb):
        blk = v[r0:r0 + rpb]
        for rl in range(lanes):
            t = blk[rl::lanes]
            if len(t):
                a += np.cumsum(t, axis=0, dtype=np.float32)[-1].astype(np.float64)
                b += np.cumsum(t * t, axis=0, dtype=np.float32)[-1].astype(np.float64)
    mu = a / rows
    var = np.maximum(b / rows - mu * mu, 0.0)
    return torch.from_numpy(mu.astype(np.float32)), torch.from_numpy((1.0 / np.sqrt(var + eps)).astype(np.float32))
