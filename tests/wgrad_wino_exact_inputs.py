"""Inputs, plans and a host model for tests/test_wgrad_wino_exact_gpu.py, which pins the Winograd-domain weight gradient
(csrc/conv3x3_wgrad_wino_f32.hip) bit for bit at the edges of its plan.  Plain module: no fixtures, no device; tests/wgrad_wino_math.py has
the transforms and the sparse recipes of the split loop.

    plan()         a mirror of the library's plan(): tiles, chunks of 16, splits, which kernel runs, whether the XCD block mapping is on.
                   The GPU tests assert it against the library (nsplit is readable from odvae_conv3x3_wgrad_wino_workspace_bytes).
    make_dense()   whole numbers in [-3, 3] (x) and [-2, 2] (dy) at every pixel, with sbar < 2^21 asserted: every partial sum of the domain
                   is then a whole number below 2^24 in any order, the halves and quarters G^T . G makes of them are exact, and the float64
                   gradient is an f32 number in every entry -- the f32 loop must return it bit for bit.
    model()        the f32 loop in float64: the kernel's tile walk (one staging slot per tile of a chunk, advanced by 16 tiles per fetch, by
                   division on narrow maps and by adds on wide ones), its border masks, its validity mask, the loop over a split's chunks,
                   the per-split slabs as the blocks write them, the reduction in its slab order, G^T . G, and dbias from the xi = (1, 1)
                   row.  fault= plants one of FAULTS; tests/test_wgrad_wino_exact_inputs.py shows that each is rejected by the shape named
                   for it in GUARDS.
"""
import collections
import functools

import torch

import wgrad_wino_math as wm

CT = wm.CHUNK
OOB = 0xFFFFFFF0                    # the f32 loop's byte-offset limit (tensors below 4 GiB)
SP_MAX_BYTES = 0x7F000000           # the split loop's (tensors below 2 GiB)

Plan = collections.namedtuple("Plan", "TX TY tiles chunks chunks_per_split nsplit last_split wide split_eligible xcd_map workspace_bytes")


def ceil_div(a, b):
    return -(-a // b)


def supported(n, h, w, cin, cout):
    if min(n, h, w, cin, cout) <= 0 or h % 2 or w % 2 or cin % 128 or cout % 128:
        return 0
    px = n * h * w
    return 0 if px * cin * 4 >= OOB or px * cout * 4 >= OOB or px // 4 >= 1 << 30 else 1


def plan(n, cin, cout, h, w):
    """the library's plan for a supported shape"""
    ty, tx = h // 2, w // 2
    tiles = n * ty * tx
    chunks = ceil_div(tiles, CT)
    base = 4 * (cin // 128) * (cout // 128)
    ns = max(1, min(256 // base, chunks))               # one 8-wave block per CU, one round
    cps = ceil_div(chunks, ns)
    nsplit = ceil_div(chunks, cps)
    px = n * h * w
    return Plan(TX=tx, TY=ty, tiles=tiles, chunks=chunks, chunks_per_split=cps, nsplit=nsplit, last_split=chunks - (nsplit - 1) * cps,
                wide=tx >= CT, split_eligible=tx % CT == 0 and px * cin * 4 < SP_MAX_BYTES and px * cout * 4 < SP_MAX_BYTES,
                xcd_map=nsplit % 8 == 0, workspace_bytes=nsplit * (16 * cin * cout + cout) * 4)


def workspace_bytes(n, cin, cout, h, w):
    return plan(n, cin, cout, h, w).workspace_bytes if supported(n, h, w, cin, cout) else 0


def nsplit_from_workspace(nbytes, cin, cout):
    per = (16 * cin * cout + cout) * 4
    assert nbytes % per == 0
    return nbytes // per


# ---- the cases: (N, Cin, Cout, H, W) -> (TX, TY, tiles, chunks, chunks per split, nsplit, chunks of the last split) --------------------------
F32_CASES = {
    # one tile per image, all four borders on every tile, nsplit 1 in the reduction
    (2, 128, 128, 2, 2): (1, 1, 2, 1, 1, 1, 1),
    # widest narrow map, one ragged chunk
    (1, 128, 128, 2, 30): (15, 1, 15, 1, 1, 1, 1),
    # chunks span tile rows and images, ragged end, nsplit 3
    (3, 128, 128, 6, 10): (5, 3, 45, 3, 1, 3, 1),
    # cib / cob indexing; dbias only from cib == 0
    (1, 128, 384, 6, 10): (5, 3, 15, 1, 1, 1, 1),
    (1, 384, 128, 6, 10): (5, 3, 15, 1, 1, 1, 1),
    # reduction: wavefronts with no slab, with one, wavefront 0 with two
    (2, 128, 128, 4, 16): (8, 2, 32, 2, 1, 2, 1),
    (3, 128, 128, 4, 16): (8, 2, 48, 3, 1, 3, 1),
    (5, 128, 128, 4, 16): (8, 2, 80, 5, 1, 5, 1),
    # the workload's narrow layer, XCD mapping on
    (2, 128, 128, 16, 16): (8, 8, 128, 8, 1, 8, 1),
    # XCD mapping with bx >> 5 up to 7, 16 slabs per reduction wavefront
    (64, 128, 128, 4, 16): (8, 2, 1024, 64, 1, 64, 1),
    # first shape past one chunk per split, short last split
    (65, 128, 128, 4, 16): (8, 2, 1040, 65, 2, 33, 1),
    # the same on 2 x 2 channel blocks
    (17, 256, 256, 4, 16): (8, 2, 272, 17, 2, 9, 1),
    # three chunks per split: both LDS stages reused
    (9, 512, 512, 4, 16): (8, 2, 144, 9, 3, 3, 3),
    # four chunks per split, short last split
    (13, 512, 512, 4, 16): (8, 2, 208, 13, 4, 4, 1),
    # wide walk, wrap inside a chunk, TX % 16 = 1
    (1, 128, 128, 4, 34): (17, 2, 34, 3, 1, 3, 1),
    # wide, TX % 16 = 15, single tile row
    (1, 128, 128, 2, 62): (31, 1, 31, 2, 1, 2, 1),
    # wide, every wrap is also an image boundary, ragged end
    (3, 128, 128, 2, 48): (24, 1, 72, 5, 1, 5, 1),
    # wide walk over several chunks of one split; split-eligible shapes on which the f32 loop is forced
    (1, 512, 512, 18, 32): (16, 9, 144, 9, 3, 3, 3),
    (3, 512, 512, 2, 96): (48, 1, 144, 9, 3, 3, 3),
    # At one chunk per split every tile is placed by the division at the start and the wide walk's advance is never consumed, so two
    # shapes more: several chunks per split on a wide map with TX % 16 != 0 -- a wrap inside every chunk; and one where every wrap is
    # also an image boundary, with a ragged end
    (1, 512, 512, 10, 34): (17, 5, 85, 6, 2, 3, 2),
    (3, 512, 512, 2, 48): (24, 1, 72, 5, 2, 3, 1),
}
SPLIT_CASES = {
    (1, 128, 128, 2, 32): (16, 1, 16, 1, 1, 1, 1),            # smallest admitted shape
    (2, 128, 128, 8, 32): (16, 4, 128, 8, 1, 8, 1),           # XCD mapping on
    (4, 128, 128, 4, 64): (32, 2, 256, 16, 1, 16, 1),         # XCD mapping, second group of eight
    (1, 512, 256, 18, 32): (16, 9, 144, 9, 2, 5, 1),          # steady state of half_phase, short last split
    (1, 512, 512, 10, 32): (16, 5, 80, 5, 2, 3, 1),
    (1, 512, 512, 18, 32): (16, 9, 144, 9, 3, 3, 3),
    (1, 512, 512, 26, 32): (16, 13, 208, 13, 4, 4, 1),
    (3, 512, 512, 2, 96): (48, 1, 144, 9, 3, 3, 3),           # TY = 1, tile rows of three chunks; every split is one whole image
    (5, 512, 512, 2, 32): (16, 1, 80, 5, 2, 3, 1),            # so one more: a split's two chunks are two images, TY = 1
}
RECIPES = ("x3", "dy3", "22")
# planted NaN: shapes with a split 1 (and, where the plan has one, a ragged last chunk), both narrow and wide f32 variants
NAN_CASES = [(0, (3, 128, 128, 6, 10)), (0, (65, 128, 128, 4, 16)), (0, (3, 128, 128, 2, 48)), (0, (1, 512, 512, 10, 32)),
             (1, (2, 128, 128, 8, 32)), (1, (1, 512, 256, 18, 32)), (1, (3, 512, 512, 2, 96))]


def table_row(shape):
    p = plan(*shape)
    return (p.TX, p.TY, p.tiles, p.chunks, p.chunks_per_split, p.nsplit, p.last_split)


def case_id(shape):
    return "%d-%dto%d-%dx%d" % shape


def nan_pixels(shape):
    """(image, row, column) of the three planted pixels: pixel (0, 0) of image 0, the last pixel of the last image (inside the ragged
    chunk where the plan has one), the first pixel of the first tile of split 1"""
    n, _, _, h, w = shape
    p = plan(*shape)
    assert p.nsplit >= 2
    tl = p.chunks_per_split * CT
    tn, rem = divmod(tl, p.TY * p.TX)
    return [(0, 0, 0), (n - 1, h - 1, w - 1), (tn, 2 * (rem // p.TX), 2 * (rem % p.TX))]


# ---- the dense exact recipe ------------------------------------------------------------------------------------------------------------------
def make_dense(n, cin, cout, h, w, seed=0):
    """x in [-3, 3], dy in [-2, 2], whole numbers at every pixel (float64); asserts sbar < 2^21"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n, cin, h, w), generator=g).double()
    dy = torch.randint(-2, 3, (n, cout, h, w), generator=g).double()
    s = wm.sbar(x, dy)
    assert s < 2.0 ** 21, "sbar = %g is not below 2^21" % s
    return x, dy


@functools.lru_cache(maxsize=None)
def dense_case(shape):
    """(x, dy, dw64, db64, sbar) of the dense recipe, built once per shape and shared: do not modify"""
    x, dy = make_dense(*shape, seed=sum(shape))
    dw, db = wm.wgrad_f64(x, dy)
    assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db), "the float64 gradient is an f32 number"
    return x, dy, dw, db, wm.sbar(x, dy)


@functools.lru_cache(maxsize=None)
def sparse_case(recipe, shape):
    """(x, dy, dw64, db64) of a sparse recipe of wgrad_wino_math.make_exact, built once and shared: do not modify"""
    x, dy = wm.make_exact(recipe, *shape, seed=3)
    dw, db = wm.wgrad_f64(x, dy)
    assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db), "the float64 gradient is an f32 number"
    return x, dy, dw, db


# ---- the host model of the f32 loop ----------------------------------------------------------------------------------------------------------
FAULTS = (
    "ragged_chunk_dropped",      # 1  total_chunks rounds down
    "past_end_taken",            # 2  tiles past end_tile are fetched where they are below total_tiles: the chunk staged past the split's end is
                                 #    the next split's first, and its dy is counted twice in dbias (dw never multiplies that stage)
    "no_left_mask",              # 3  column 0 of the patch is read at ttx == 0: the pixel to the left in memory
    "no_bottom_mask",            # 4  row 3 of the patch is read at tty == TY - 1: the first row of the next image
    "wide_wrap_on_equal",        # 5  the wide walk wraps only when ttx + 16 == TX
    "tty_not_reset",             # 6  the tile row is not reset at an image boundary
    "xcd_plain_split",           # 7  with the XCD mapping on, the split index is still bx >> 2
    "reduce_skips_3_mod_4",      # 8  the reduction's fourth wavefront sums nothing
    "dbias_misses_last_split",   # 9
    "stale_stage",               # 10 the last iteration adds the chunk of the other LDS stage once more
    "reduce_starts_at_k_plus_4",     # wavefront k begins at slab k + 4
    "no_top_mask",
    "no_right_mask",
)
# the shape named to guard against each fault (every one is in F32_CASES)
GUARDS = {
    "ragged_chunk_dropped": [(1, 128, 128, 2, 30), (3, 128, 128, 6, 10), (3, 128, 128, 2, 48)],
    "past_end_taken": [(3, 128, 128, 6, 10), (65, 128, 128, 4, 16)],
    "no_left_mask": [(2, 128, 128, 2, 2), (1, 128, 128, 4, 34)],
    "no_bottom_mask": [(2, 128, 128, 2, 2), (3, 128, 128, 2, 48)],
    "wide_wrap_on_equal": [(1, 512, 512, 10, 34), (3, 512, 512, 2, 48)],
    "tty_not_reset": [(3, 512, 512, 2, 48), (65, 128, 128, 4, 16)],
    "xcd_plain_split": [(2, 128, 128, 16, 16), (64, 128, 128, 4, 16)],
    "reduce_skips_3_mod_4": [(5, 128, 128, 4, 16), (64, 128, 128, 4, 16)],
    "dbias_misses_last_split": [(2, 128, 128, 4, 16), (13, 512, 512, 4, 16)],
    "stale_stage": [(9, 512, 512, 4, 16), (65, 128, 128, 4, 16), (1, 512, 512, 18, 32)],
    "reduce_starts_at_k_plus_4": [(3, 128, 128, 4, 16), (5, 128, 128, 4, 16)],
    "no_top_mask": [(2, 128, 128, 2, 2)],
    "no_right_mask": [(2, 128, 128, 2, 2), (1, 128, 128, 2, 30)],
}


def _walk(p, n, h, w, split, fault):
    """The staging slots' tile walk over one split: a list, one entry per chunk the loop stages -- the split's own, which it multiplies, and
    the one after them, which it stages in its last iteration, all zeros, and never multiplies (its dy still runs through the bias sum) --
    of int64 tensors [16] (tl, valid, tty, ttx, xo, yo): the tile, whether it is fetched, its tile row and column as the masks see them,
    and the pixel index (row-major over image, row, column) of the patch origin (row 2 tty - 1, column 2 ttx - 1) and of the dy tile."""
    chunks = p.tiles // CT if fault == "ragged_chunk_dropped" else p.chunks
    chunk0 = split * p.chunks_per_split
    nch = min(p.chunks_per_split, chunks - chunk0)
    end_tile = min(p.tiles, (chunk0 + nch) * CT)
    if fault == "past_end_taken":
        end_tile = p.tiles
    per_img = p.TY * p.TX
    tl = chunk0 * CT + torch.arange(CT)

    def by_division(tl):
        tn, rem = tl // per_img, tl % per_img
        if fault == "tty_not_reset" and (tl >= CT * chunk0 + CT).all():      # every fetch after the first
            tn, rem = torch.zeros_like(tl), tl
        tty, ttx = rem // p.TX, rem % p.TX
        return tty, ttx, (tn * h + 2 * tty - 1) * w + 2 * ttx - 1, (tn * h + 2 * tty) * w + 2 * ttx
    tty, ttx, xo, yo = by_division(tl)
    out = []
    for _ in range(max(nch, 0) + 1):
        out.append((tl, tl < end_tile, tty, ttx, xo, yo))
        tl = tl + CT
        if p.wide:      # W = 2 TX, H = 2 TY: 16 tiles on are 32 pixels on, plus one pixel row where the tile row wraps
            nx = ttx + CT
            wrap = (nx == p.TX) if fault == "wide_wrap_on_equal" else (nx >= p.TX)
            xo = xo + 2 * CT + wrap * w
            yo = yo + 2 * CT + wrap * w
            ttx = torch.where(wrap, nx - p.TX, nx)
            ny = tty + wrap
            tty = ny if fault == "tty_not_reset" else torch.where(ny >= p.TY, torch.zeros_like(ny), ny)
        else:
            tty, ttx, xo, yo = by_division(tl)
    return out


def _gather(flat, pix, ok):
    """flat [pixels][C], pix / ok [...] -> [...][C]: the pixel where ok and inside the tensor, else 0 (a buffer load out of range)"""
    ok = ok & (pix >= 0) & (pix < flat.shape[0])
    return flat[torch.where(ok, pix, torch.zeros_like(pix))] * ok.unsqueeze(-1)


def model(x, dy, fault=None):
    """x [N][Cin][H][W], dy [N][Cout][H][W] float64 -> (dw [Cout][Cin][3][3], db [Cout]) as the f32 loop and the reduction make them, every
    sum in float64.  A slab row no block writes stays NaN."""
    assert fault is None or fault in FAULTS
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    p = plan(n, cin, cout, h, w)
    xf = x.permute(0, 2, 3, 1).reshape(-1, cin)
    yf = dy.permute(0, 2, 3, 1).reshape(-1, cout)
    i4, i2 = torch.arange(4), torch.arange(2)

    def split_sums(split):
        """dU [16][Cin][Cout] and the bias partial [Cout] of one split's blocks"""
        du = torch.zeros(16, cin, cout, dtype=torch.float64)
        bias = torch.zeros(cout, dtype=torch.float64)
        staged = _walk(p, n, h, w, split, fault)
        nch = len(staged) - 1
        for k, (tl, valid, tty, ttx, xo, yo) in enumerate(staged):
            rok = torch.ones(CT, 4, dtype=torch.bool)
            cok = torch.ones(CT, 4, dtype=torch.bool)
            if fault != "no_top_mask":
                rok[:, 0] = tty > 0
            if fault != "no_bottom_mask":
                rok[:, 3] = tty < p.TY - 1
            if fault != "no_left_mask":
                cok[:, 0] = ttx > 0
            if fault != "no_right_mask":
                cok[:, 3] = ttx < p.TX - 1
            ok = valid[:, None, None] & rok[:, :, None] & cok[:, None, :]
            d = _gather(xf, xo[:, None, None] + i4[None, :, None] * w + i4[None, None, :], ok)                  # [16][4][4][Cin]
            t = _gather(yf, yo[:, None, None] + i2[None, :, None] * w + i2[None, None, :], valid[:, None, None].expand(CT, 2, 2))
            v = torch.einsum("ri,tijc,sj->rstc", wm.BT, d, wm.BT).reshape(16, CT, cin)
            m = torch.einsum("ri,tijc,sj->rstc", wm.A, t, wm.A).reshape(16, CT, cout)
            bias += m[5].sum(0)          # xi = (1, 1): dy00 + dy01 + dy10 + dy11, of every chunk staged
            if k < nch:
                weight = 2.0 if fault == "stale_stage" and nch >= 2 and k == nch - 2 else 1.0
                du += weight * torch.einsum("xti,xto->xio", v, m)
        return du, bias

    slabs = torch.full((p.nsplit, 16, cin, cout), float("nan"), dtype=torch.float64)
    bias_part = torch.full((p.nsplit, cout), float("nan"), dtype=torch.float64)
    rows_of = collections.defaultdict(list)          # split -> the domain rows r whose blocks take it
    for bx in range(4 * p.nsplit):
        if p.xcd_map:
            r, split = (bx >> 3) & 3, (bx >> 2 if fault == "xcd_plain_split" else (bx & 7) + 8 * (bx >> 5))
        else:
            r, split = bx & 3, bx >> 2
        rows_of[split].append(r)
    for split, rows in rows_of.items():
        du, bias = split_sums(split)
        for r in rows:
            slabs[split, 4 * r:4 * r + 4] = du[4 * r:4 * r + 4]
            if r == 1:                                # and cib == 0: every channel block of dy is summed by exactly one block
                bias_part[split] = bias

    # the reduction: wavefront k sums the slabs k, k + 4, ..., the four partial sums meet as (0 + 1) + (2 + 3)
    part = torch.zeros(4, 16, cin, cout, dtype=torch.float64)
    for k in range(4):
        if fault == "reduce_skips_3_mod_4" and k == 3:
            continue
        for s in range(k + 4 if fault == "reduce_starts_at_k_plus_4" else k, p.nsplit, 4):
            part[k] += slabs[s]
    dw = wm.to_weights((part[0] + part[1]) + (part[2] + part[3]))
    db = torch.zeros(cout, dtype=torch.float64)
    for q in range(p.nsplit - 1 if fault == "dbias_misses_last_split" else p.nsplit):
        db += bias_part[q]
    return dw, db
