"""Inputs, a float64 reference and a host model for the segmented gradient norms (odvae_grad_seg_norms_f32) and the clamped Adam step
(odvae_adam_step_clamp_f32); shared by tests/test_grad_norms_inputs.py (CPU) and tests/test_grad_norms_gpu.py.

The contract (include/odvae_hip.h): out[i] = the p-norm of segment i of one flat f32 arena, summed in float64 and rounded to f32 once;
out[n_seg] = the same norm of those F32 values over the segments that count, summed in float64 again.  `reference` is that contract in
numpy.  `host_model` walks the kernel's index space -- 4096-float chunks, the last partial chunk with its float4 body and scalar tail, the
segment of a chunk found by a search in the chunk prefix, at most K segments per launch -- and takes planted faults, so the CPU tests show
that the cases the GPU tests run tell a wrong kernel from a right one."""
import numpy as np
import torch
import torch.nn as nn

CHUNK = 4096
SEGS_PER_LAUNCH = 160
MAX, L1, L2, P = 0, 1, 2, 3      # ODVAE_NORM_*
EDGE_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193]
FAULTS = ("f32_accumulate", "read_padding", "max_drops_nan", "one_short", "total_unrounded", "noncounting_in_total")


def kind_of(p):
    if p == "inf" or p == float("inf"):
        return MAX, 0.0
    return (L1 if p == 1 else L2 if p == 2 else P), float(p)


def layout(lengths, lead=0, gap=1):
    """Offsets of segments `lengths` on the optimizer arena's 64-float grid with `gap` extra empty 64-float rows between them (the
    round-up padding comes on top), `lead` floats in front and 128 behind.  Returns (offsets, arena length)."""
    offs, off = [], lead
    for n in lengths:
        offs.append(off)
        off += (n + 63) // 64 * 64 + 64 * gap
    return offs, off + 128


def fill(lengths, offs, total, values, outside=float("nan")):
    """f32 arena of `total` floats: `outside` (NaN canaries) everywhere but the segments, which take values(i, n) -> array of n."""
    arena = np.full(total, outside, dtype=np.float32)
    for i, (o, n) in enumerate(zip(offs, lengths)):
        arena[o:o + n] = values(i, n)
    return arena


def whole_numbers(seed):
    """values(i, n): whole numbers in [-8, 8]: every sum of |g|, g^2, g^3 over any segment here is exact in float64 in any order."""
    rng = np.random.RandomState(seed)
    return lambda i, n: rng.randint(-8, 9, size=n).astype(np.float32)


def perfect_square_segment(n, k):
    """n floats whose sum of squares is a perfect square: {3, 4, 0, ...} scaled by k where it fits, else k * k ones need n >= k * k."""
    v = np.zeros(n, dtype=np.float32)
    if n >= 2:
        v[0], v[-1] = 3.0 * k, -4.0 * k      # sum of squares (5k)^2
    else:
        v[0] = float(k)
    return v


def _seg_norm(x, kind, p):
    a = np.abs(x.astype(np.float64))
    if kind == MAX:
        return np.float32(np.nan) if np.isnan(a).any() else np.float32(a.max())
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == L1:
            return np.float32(a.sum())
        if kind == L2:
            return np.float32(np.sqrt((a * a).sum()))
        return np.float32(np.power(np.power(a, p).sum(), 1.0 / p))


def reference(arena, offs, lengths, counts, norm_type):
    """float32 [n_seg + 1]: the contract in float64 (numpy's pairwise float64 sums: exact on the whole-number inputs, ~1e-16 relative
    otherwise -- far below the f32 rounding that follows)."""
    kind, p = kind_of(norm_type)
    out = np.array([_seg_norm(arena[o:o + n], kind, p) for o, n in zip(offs, lengths)], dtype=np.float32)
    sel = out[np.asarray(counts, dtype=bool)] if counts is not None else out
    total = _seg_norm(sel, kind, p) if sel.size else np.float32(0.0)
    return np.concatenate([out, np.array([total], dtype=np.float32)])


def host_model(arena, offs, lengths, counts, norm_type, fault=None, chunk=CHUNK, segs_per_launch=SEGS_PER_LAUNCH):
    """The kernel's walk on the host.  Stage 1 per launch of <= K segments: chunk c of the launch -> its segment by the prefix search ->
    [base, base + n) of that segment, n4 = n // 4 float4 and n - 4 * n4 scalars -> one float64 partial.  Stage 2: a segment's partials
    -> one f32.  Stage 3: the counting segments' f32 values -> the total.  `fault` plants one of FAULTS."""
    assert fault is None or fault in FAULTS
    kind, p = kind_of(norm_type)
    n_seg = len(offs)

    def take(x):
        a = np.abs(x.astype(np.float64))
        if kind == MAX:
            if fault == "max_drops_nan":
                return np.fmax.reduce(a) if a.size else 0.0
            return np.nan if np.isnan(a).any() else (a.max() if a.size else 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            v = a if kind == L1 else a * a if kind == L2 else np.power(a, p)
            if fault == "f32_accumulate":
                return float(np.cumsum(v.astype(np.float32), dtype=np.float32)[-1]) if v.size else 0.0      # one running f32 sum
            return v.sum()

    def fold(parts):
        parts = np.asarray(parts, dtype=np.float64)
        if kind == MAX:
            if fault == "max_drops_nan":
                return np.fmax.reduce(parts)
            return np.nan if np.isnan(parts).any() else parts.max()
        if fault == "f32_accumulate":
            return float(np.cumsum(parts.astype(np.float32), dtype=np.float32)[-1])
        return parts.sum()

    def finish(s):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.float32(s) if kind in (MAX, L1) else np.float32(np.sqrt(s)) if kind == L2 else np.float32(np.power(s, 1.0 / p))

    partials, records = [], []
    for first in range(0, n_seg, segs_per_launch):
        idx = list(range(first, min(first + segs_per_launch, n_seg)))
        prefix = np.cumsum([0] + [-(-lengths[i] // chunk) for i in idx])
        base_part = len(partials)
        for c in range(int(prefix[-1])):
            lo = int(np.searchsorted(prefix, c, side="right")) - 1      # last segment of the launch whose prefix <= c
            seg = idx[lo]
            base = (c - int(prefix[lo])) * chunk
            n = min(lengths[seg] - base, chunk)
            if fault == "one_short" and base + n == lengths[seg]:
                n -= 1
            if fault == "read_padding":
                n = -(-n // 4) * 4                                       # whole float4 past the segment's end
            if fault == "f32_accumulate" and base > 0:
                continue                                                 # (the running sum took the whole segment at its first chunk)
            span = lengths[seg] if fault == "f32_accumulate" else n
            partials.append(take(arena[offs[seg] + base:offs[seg] + base + span]))
            if c == int(prefix[lo]):
                records.append((len(partials) - 1, seg))
        assert len(partials) >= base_part
    out = np.zeros(n_seg + 1, dtype=np.float32)
    sums = np.zeros(n_seg, dtype=np.float64)
    bounds = [r[0] for r in records] + [len(partials)]
    for j, (_, seg) in enumerate(records):
        sums[seg] = fold(partials[bounds[j]:bounds[j + 1]])
        out[seg] = finish(sums[seg])
    flags = np.ones(n_seg, dtype=bool) if (counts is None or fault == "noncounting_in_total") else np.asarray(counts, dtype=bool)
    if not flags.any():
        return out
    if fault == "total_unrounded":
        out[n_seg] = finish(fold(sums[flags]))
    else:
        sel = out[:n_seg][flags]
        if kind == MAX:
            out[n_seg] = finish(fold(np.abs(sel.astype(np.float64))))
        else:
            a = np.abs(sel.astype(np.float64))
            with np.errstate(over="ignore", invalid="ignore"):
                out[n_seg] = finish(fold(a if kind == L1 else a * a if kind == L2 else np.power(a, p)))
    return out


def ulps(a, b):
    """Distance in f32 units in the last place between two f32 arrays (0 where both are NaN or bit-equal; huge where one is NaN)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN (payloads are not under test)."""
    return bool((ulps(a, b) == 0).all())


# ---- clamp ---------------------------------------------------------------------------------------------------------------------------
def clamp_inputs(n, seed, c):
    """n gradients around the bound c with NaN, +-inf, -0.0, +0.0 and subnormals planted (cyclically, so n = 1 ... 5 get some too)."""
    rng = np.random.RandomState(seed)
    g = (rng.standard_normal(n) * 2.0 * c).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, c, -c, np.nextafter(np.float32(c), np.float32(np.inf))], dtype=np.float32)
    pos = (np.arange(len(special)) * 7 + seed) % n
    g[pos] = special[:len(pos)]
    return g


def clamp_model(g, c, fault=None):
    """torch.clamp(g, -c, c) on the host: NaN stays NaN, +-inf -> +-c, -0.0 stays -0.0.  fault 'nan_to_c': fmin / fmax, which drop NaN."""
    g = np.asarray(g, dtype=np.float32)
    if fault == "nan_to_c":
        return np.fmin(np.fmax(g, np.float32(-c)), np.float32(c))
    return np.where(g < -c, np.float32(-c), np.where(g > c, np.float32(c), g)).astype(np.float32)


# ---- a two-optimizer module with the surface Trainer uses (CPU: torch.optim.Adam, the fallback path) -------------------------------------
class TinyLightning(nn.Module):
    """`side` belongs to optimizer 0 but joins the loss only on the batch indices in `side_batches`; `idle` belongs to it too and never
    gets a gradient.  `logs` keeps every log_dict call."""

    def __init__(self, side_batches=()):
        super().__init__()
        self.gen = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 4))
        self.disc = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 4))
        self.side = nn.Linear(8, 4)
        self.idle = nn.Linear(2, 2)
        self.side_batches = tuple(side_batches)
        self._global_step = 0
        self.learning_rate = 1e-2
        self.logs = []

    @property
    def global_step(self):
        return self._global_step

    def log_dict(self, d, *args, **kwargs):
        self.logs.append({k: v.detach().clone() for k, v in d.items()})

    def training_step(self, batch, batch_idx, optimizer_idx):
        x, y = batch
        if optimizer_idx == 0:
            out = self.gen(x)
            if batch_idx in self.side_batches:
                out = out + self.side(x)
            return ((out - y) ** 2).mean()
        return (self.disc(x) ** 2).mean()

    def configure_optimizers(self):
        gen = list(self.gen.parameters()) + list(self.side.parameters()) + list(self.idle.parameters())
        return [torch.optim.Adam(gen, lr=self.learning_rate, betas=(0.5, 0.9)),
                torch.optim.Adam(self.disc.parameters(), lr=self.learning_rate, betas=(0.5, 0.9))], []


def tiny_batches(n, seed=5, rows=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 8, generator=g), torch.randn(rows, 4, generator=g)) for _ in range(n)]

