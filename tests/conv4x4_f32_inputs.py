"""Cases and host mirrors for the f32 implicit-GEMM PatchGAN convolutions (odvae_conv4x4_f32, odvae_conv4x4_wgrad_f32).

* the cases beyond gan_lpips_inputs.CONV_CASES, each chosen for one mechanism of the kernels, and one weight-gradient case per stride
  that the library must plan as several splits with a short last one over more than one channel tile on both axes;
* host mirrors of what the library decides on the host: the pack sizes and the weight-gradient plan;
* float64 mirrors of the kernels' INDEX arithmetic -- the pack orders of odvae_conv4x4_pack_f32 and the halo walks of the four
  geometries (forward at stride 1 and 2, the stride-1 data gradient as a pad-2 conv on flipped taps, the stride-2 data gradient by
  output parity class on the grid ceil(Hi/2) x ceil(Wi/2), the weight gradient in two halves of eight taps), which
  tests/test_conv4x4_f32_inputs.py holds to the host models of tests/conv4x4_bf16_inputs.py.
Plain module: no fixtures, no device.  All tensors are float64 NCHW on the host.
"""
import torch
import torch.nn.functional as F

import gan_lpips_inputs as G

# (stride, (Hi, Wi), Cin, Cout, bias, N), as gan_lpips_inputs.CONV_CASES
EXTRA_CASES = [
    (2, (36, 44), 64, 130, True, 3),       # 18 x 22 outputs = 3 x 2 ragged tiles; Cout past one 128-block with 2 live channels
    (2, (35, 41), 3, 64, True, 2),         # odd Hi and Wi at stride 2; the 3-channel image layer
    (2, (9, 7), 72, 4, False, 3),          # ragged reduction chunk; narrow output
    (2, (66, 68), 8, 64, True, 2),         # one 8-channel chunk; 33 x 34 outputs
    (1, (10, 19), 256, 130, False, 2),     # stride 1; 2 x 2 ragged tiles; eight chunks
    (1, (9, 7), 130, 1, True, 3),          # the head; Cin % 4 != 0
    (1, (33, 34), 64, 64, True, 2),        # 4 x 3 tiles
    (1, (12, 20), 512, 4, True, 1),        # reduction of 8 192
    (1, (2, 2), 3, 1, True, 1),            # one output pixel
    (2, (2, 2), 3, 1, True, 1),
]
ALL_CASES = list(G.CONV_CASES) + EXTRA_CASES

# the weight gradient past one tile per block: 88 tiles (4 per image) in 30 splits of 3 with a last split of 1, so splits cross image
# boundaries; 2 ci tiles (72 channels: a ragged second one), 3 co tiles (130).  N Ho Wo = 3 762 / 2 376 pixels.
WGRAD_SPLIT_CASES = {1: (1, (10, 20), 72, 130, True, 22), 2: (2, (13, 37), 72, 130, True, 22)}
WGRAD_SPLIT_PLAN = {"kind": 1, "ntiles": 88, "nsplit": 30, "tiles_per_split": 3, "ci_tiles": 2, "co_tiles": 3}
PLAN_FIELDS = ("kind", "ntiles", "nsplit", "tiles_per_split", "ci_tiles", "co_tiles", "tile_rows", "stride")


def case_id(c):
    s, (h, w), cin, cout, bias, n = c
    return "s%d-%dx%d-%d-%d-%s-n%d" % (s, h, w, cin, cout, "b" if bias else "nb", n)


def ceil_div(a, b):
    return -(-a // b)


def reduce_pad(c):
    return ceil_div(c, 32) * 32


def out_pad(c):
    return 32 if c <= 32 else ceil_div(c, 128) * 128


def pack_floats(c_reduce, c_out):
    """[16][reduce_pad / 4][out_pad][4]"""
    return 16 * reduce_pad(c_reduce) * out_pad(c_out)


def wgrad_plan_model(stride, n, hi, wi, cin, cout):
    """the rule of odvae_conv4x4_wgrad_plan: tiles of 8 x 16 (stride 1) / 4 x 16 (stride 2) output pixels, 64-channel tiles on both axes,
    about 256 (split, ci tile, co tile) triples, each run as two blocks (tap halves)"""
    ho, wo = G.out4x4(hi, stride), G.out4x4(wi, stride)
    th = 8 if stride == 1 else 4
    ntiles = ceil_div(wo, 16) * ceil_div(ho, th) * n
    ci_tiles, co_tiles = ceil_div(cin, 64), ceil_div(cout, 64)
    nsplit = max(1, min(ceil_div(256, ci_tiles * co_tiles), ntiles))
    tps = ceil_div(ntiles, nsplit)
    return dict(zip(PLAN_FIELDS, (1, ntiles, ceil_div(ntiles, tps), tps, ci_tiles, co_tiles, th, stride)))


def wgrad_workspace_bytes(stride, n, hi, wi, cin, cout):
    p = wgrad_plan_model(stride, n, hi, wi, cin, cout)
    cinp, coutp = p["ci_tiles"] * 64, p["co_tiles"] * 64
    return 4 * (p["nsplit"] * 16 * cinp * coutp + p["nsplit"] * coutp)


# ------------------------------------------------------------------------------------------------------------------------------
# the kernels' index arithmetic in float64
# ------------------------------------------------------------------------------------------------------------------------------
def pack_fwd_model(w):
    """[16][Cin][Cout]: entry kh * 4 + kw holds w[co][ci][kh][kw]"""
    cout, cin = w.shape[:2]
    return w.reshape(cout, cin, 16).permute(2, 1, 0).contiguous()


def pack_dgrad_model(w, stride):
    """[16][Cout][Cin].  Stride 1: entry t holds tap 15 - t.  Stride 2: entry cls * 4 + a * 2 + b, cls = 2 py + px, holds tap
    (3 - py - 2a, 3 - px - 2b)."""
    cout, cin = w.shape[:2]
    flat = w.reshape(cout, cin, 16)
    src = []
    for t in range(16):
        if stride == 1:
            src.append(15 - t)
        else:
            cls, a, b = t >> 2, (t >> 1) & 1, t & 1
            src.append((3 - (cls >> 1) - 2 * a) * 4 + (3 - (cls & 1) - 2 * b))
    return flat[:, :, src].permute(2, 0, 1).contiguous()


_P = 4


def _at(xp, r0, c0, step, nr, nc):
    """xp[:, :, r0 + _P :: step, c0 + _P :: step] with nr x nc elements (xp is x zero-padded by _P before and generously after)"""
    return xp[:, :, r0 + _P:r0 + _P + step * (nr - 1) + 1:step, c0 + _P:c0 + _P + step * (nc - 1) + 1:step]


def walk16(x, pack, step, origin, ho, wo):
    """the 16-tap halo walk: y[oy][ox] = sum_t x[step oy + origin + t // 4][step ox + origin + t % 4] pack[t], zero outside x"""
    xp = F.pad(x, (_P, _P + 8, _P, _P + 8))
    y = torch.zeros(x.shape[0], pack.shape[2], ho, wo, dtype=x.dtype)
    for t in range(16):
        y = y + torch.einsum("nchw,co->nohw", _at(xp, origin + t // 4, origin + t % 4, step, ho, wo), pack[t])
    return y


def forward_by_pack(x, w, b, stride):
    """MODE 6 (stride 2) / MODE 7 (stride 1): origin -1"""
    ho, wo = G.out4x4(x.shape[2], stride), G.out4x4(x.shape[3], stride)
    y = walk16(x, pack_fwd_model(w), stride, -1, ho, wo)
    return y if b is None else y + b.reshape(1, -1, 1, 1)


def dgrad_by_pack(dy, w, x_shape, stride):
    """stride 1: MODE 9, the walk with origin -2 on the flipped pack.  stride 2: MODE 8 -- low-res pixel (y, x) of the grid
    ceil(Hi/2) x ceil(Wi/2), class (py, px): dx[2y + py][2x + px] = sum_{a, b} dy[y + py - 1 + a][x + px - 1 + b] pack[cls * 4 + 2a + b];
    stores at rows >= Hi / columns >= Wi are dropped"""
    n, cin, hi, wi = x_shape
    pack = pack_dgrad_model(w, stride)
    if stride == 1:
        return walk16(dy, pack, 1, -2, hi, wi)
    gh, gw = ceil_div(hi, 2), ceil_div(wi, 2)
    dyp = F.pad(dy, (_P, _P + 8, _P, _P + 8))
    dx = torch.zeros(n, cin, 2 * gh, 2 * gw, dtype=dy.dtype)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        acc = torch.zeros(n, cin, gh, gw, dtype=dy.dtype)
        for a in range(2):
            for b in range(2):
                acc = acc + torch.einsum("nohw,oc->nchw", _at(dyp, py - 1 + a, px - 1 + b, 1, gh, gw), pack[cls * 4 + 2 * a + b])
        dx[:, :, py::2, px::2] = acc
    return dx[:, :, :hi, :wi].contiguous()


def wgrad_by_halves(x, dy, stride):
    """the weight-gradient kernel's walk: half z stages the halo from row S oy0 - 1 + 2z and its eight taps are local row khl in {0, 1},
    column kw: dw[..][2z + khl][kw] = sum dy[oy][ox] x[S oy - 1 + 2z + khl][S ox - 1 + kw]"""
    ho, wo = dy.shape[2:]
    xp = F.pad(x, (_P, _P + 8, _P, _P + 8))
    dw = torch.zeros(dy.shape[1], x.shape[1], 4, 4, dtype=x.dtype)
    for z in range(2):
        for t8 in range(8):
            khl, kw = t8 // 4, t8 % 4
            dw[:, :, 2 * z + khl, kw] = torch.einsum("nohw,nchw->oc", dy, _at(xp, -1 + 2 * z + khl, -1 + kw, stride, ho, wo))
    return dw
