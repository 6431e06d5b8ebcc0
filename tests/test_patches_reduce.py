"""CPU checks for Pillow's box pre-reduction in the patch path (`Image.resize(BILINEAR, reducing_gap=1.0)` on a crop of side
>= 2 S, src/data/datasets/nuscenes.py:176): a numpy model of the kernel's arithmetic (csrc/patch_u8.hip,
patch_reduce_resize_kernel) driven by the product's own host tables -- `reduce_multipliers`, `reduced_resample_table` -- is
held to Pillow itself, bit for bit; two planted mistakes must be caught; `crop_is_background` is held to a direct IoU formula."""
import numpy as np
import pytest

PIL_Image = pytest.importorskip("PIL.Image")

CASES = ([(16, s) for s in (32, 33, 47, 48, 50, 63, 64, 79, 100, 113)] + [(24, s) for s in (50, 100, 200)]
         + [(32, 200), (32, 400), (64, 200), (64, 400), (128, 256), (128, 257), (128, 400)]
         + [(256, s) for s in (512, 513, 767, 800, 900)])


def _image(S, size):
    return np.random.default_rng(1000 * S + size).integers(0, 256, (size, size, 3), dtype=np.uint8)


def reduce_model(img, f, mults, full_divisor_on_partial=False):
    """The kernel's stage 1: every reduced pixel from its box of the crop; u32 arithmetic ((ss + n/2) * mult(n)) >> 24 with the
    three multipliers of `reduce_multipliers` (full boxes, last column / row, corner)."""
    size = img.shape[0]
    r = -(-size // f)
    padded = np.zeros((r * f, r * f, 3), np.uint64)
    padded[:size, :size] = img
    ss = padded.reshape(r, f, r, f, 3).sum(axis=(1, 3))
    side = np.minimum(f, size - np.arange(r) * f)                                  # box width / height per reduced column / row
    partial = (side != f).astype(int)
    n = (side[:, None] * side[None, :]).astype(np.uint64)
    m = np.asarray(mults[:3], np.uint64)[partial[:, None] + partial[None, :]]      # full, one partial side, corner
    if full_divisor_on_partial:
        n, m = np.full_like(n, f * f), np.full_like(m, mults[0])
    v = (ss + (n // np.uint64(2))[:, :, None]) * m[:, :, None]
    assert int(v.max()) < 2 ** 32                                                  # the kernel's u32 product does not wrap
    return (v >> np.uint64(24)).astype(np.uint8)


def two_pass_model(red, tab, S):
    """The kernel's stages 2 and 3 from a table whose windows index the reduced image."""
    half = 1 << 21
    r = red.shape[0]
    src = np.minimum(tab[:, 5, None] + np.arange(5)[None], r - 1)          # taps beyond the window carry a zero coefficient
    k = np.where(np.arange(5)[None] < tab[:, 6, None], tab[:, :5], 0).astype(np.int64)
    hor = half + (red.astype(np.int64)[:, src, :] * k[None, :, :, None]).sum(2)          # [r, S, 3]
    hor = np.clip(hor >> 22, 0, 255)
    out = half + (hor[src] * k[:, :, None, None]).sum(1)                                   # [S, S, 3]
    return np.clip(out >> 22, 0, 255).astype(np.uint8)


def chain_model(img, S, table=None, **kw):
    from odvae_amd.patches import reduce_multipliers, reduced_resample_table
    f, tab = reduced_resample_table(img.shape[0], S)
    return two_pass_model(reduce_model(img, f, reduce_multipliers(img.shape[0], f), **kw), tab if table is None else table, S)


def _pil_resize(img, S):
    return np.asarray(PIL_Image.fromarray(img).resize((S, S), resample=PIL_Image.Resampling.BILINEAR, reducing_gap=1.0))


@pytest.mark.parametrize("S,size", CASES)
def test_reduce_rule_matches_pillow_reduce(S, size):
    from odvae_amd.patches import reduce_multipliers, reduced_resample_table
    f, tab = reduced_resample_table(size, S)
    assert f == size // S >= 2 and tab.shape == (S, 8) and tab.dtype == np.int32
    img = _image(S, size)
    ref = np.asarray(PIL_Image.fromarray(img).reduce(f))
    assert np.array_equal(reduce_model(img, f, reduce_multipliers(size, f)), ref)
    ramp = np.broadcast_to((np.arange(size * size) % 256).astype(np.uint8).reshape(size, size, 1), (size, size, 3)).copy()
    assert np.array_equal(reduce_model(ramp, f, reduce_multipliers(size, f)), np.asarray(PIL_Image.fromarray(ramp).reduce(f)))


@pytest.mark.parametrize("S,size", CASES)
def test_reduce_then_resize_matches_pillow(S, size):
    img = _image(S, size)
    assert np.array_equal(chain_model(img, S), _pil_resize(img, S))
    flat = np.full((size, size, 3), 255, np.uint8)                           # the largest sums: nothing wraps, nothing clips early
    assert np.array_equal(chain_model(flat, S), _pil_resize(flat, S))


@pytest.mark.parametrize("S,size", CASES + [(16, 31), (96, 191), (96, 287), (256, 511), (80, 150), (80, 333)])
def test_tables_fit_the_kernel(S, size):
    """At most 5 taps per window, windows inside the reduced image, the mask's NEAREST index from the unreduced walk, and the
    window of reduced pixels behind a 64 x 4 output block inside the kernel's LDS tile (RED_W = 136 columns, RED_H = 13 rows)."""
    from odvae_amd.patches import reduced_resample_table
    from oracle import patches as oracle
    f, tab = reduced_resample_table(size, S)
    r = -(-size // f)
    first, taps = tab[:, 5].astype(int), tab[:, 6].astype(int)
    assert taps.min() >= 1 and taps.max() <= 5 and first.min() >= 0 and (first + taps).max() <= r
    assert np.all(np.diff(first) >= 0) and np.all(np.diff(first + taps) >= 0)
    assert not np.where(np.arange(5)[None] >= taps[:, None], tab[:, :5], 0).any()
    assert np.array_equal(tab[:, 7], oracle.pillow_nearest_index(size, S))
    for o0 in range(0, S, 64):
        o1 = min(o0 + 63, S - 1)
        assert first[o1] + taps[o1] - first[o0] <= 131
    for o0 in range(0, S, 4):
        o1 = min(o0 + 3, S - 1)
        assert first[o1] + taps[o1] - first[o0] <= 11


def test_small_crops_keep_the_plain_table_and_the_refusal_stays():
    from odvae_amd.patches import reduce_multipliers, reduced_resample_table, resample_table
    for S, size in [(96, 50), (96, 96), (96, 191), (256, 400), (16, 31)]:
        f, tab = reduced_resample_table(size, S)
        assert f == 1 and np.array_equal(tab, resample_table(size, S))
    assert int(reduce_multipliers(50, 1)[0]) == 1 << 24          # f = 1: (ss * 2^24) >> 24 = ss, the "reduce" is a copy
    with pytest.raises(ValueError):
        resample_table(192, 96)


def _table_with_box_edge(size, S, in1):
    """`reduced_resample_table` with a planted source-box edge (Resample.c precompute_coeffs in scalar f64)."""
    from oracle.patches import PRECISION_BITS
    f = size // S
    r = -(-size // f)
    scale = in1 / S
    filterscale = max(scale, 1.0)
    support, ss = filterscale, 1.0 / filterscale
    tab = np.zeros((S, 8), np.int32)
    for xx in range(S):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), r) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        tot = 0.0
        for v in w:
            tot += v
        tab[xx, :n] = [int(0.5 + v / tot * (1 << PRECISION_BITS)) for v in w]
        tab[xx, 5:7] = (xmin, n)
    return tab


def test_a_float64_box_edge_is_caught():
    """Pillow's C entry takes the source box as float32: the f64 quotient size / f gives other coefficients and other bytes."""
    from odvae_amd.patches import reduced_resample_table
    S, size = 64, 200
    img = _image(S, size)
    f, tab = reduced_resample_table(size, S)
    good = _table_with_box_edge(size, S, float(np.float32(size / f)))
    assert np.array_equal(good[:, :7], tab[:, :7])                       # the scalar restatement is the product's table
    bad = _table_with_box_edge(size, S, size / f)
    assert not np.array_equal(bad, good)
    ref = _pil_resize(img, S)
    assert np.array_equal(chain_model(img, S, table=good), ref)
    differing = int((chain_model(img, S, table=bad) != ref).sum())
    print("float64 box edge: %d of %d bytes differ" % (differing, ref.size))
    assert differing > 0


@pytest.mark.parametrize("S,size", [(16, 50), (16, 79), (32, 200), (128, 257), (256, 767)])
def test_a_full_divisor_on_partial_boxes_is_caught(S, size):
    """The last column / row (size % f != 0) averages over the pixels it has, not over f * f."""
    assert size % (size // S) != 0
    img = _image(S, size)
    ref = _pil_resize(img, S)
    assert np.array_equal(chain_model(img, S), ref)
    assert not np.array_equal(chain_model(img, S, full_divisor_on_partial=True), ref)


def _iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def test_crop_is_background_is_the_iou_rule():
    """nuscenes.py:585-595: accepted iff every IoU < 0.5, or there is no box.  Integer and half-integer coordinates: the IoU is
    then at least 1 / (2 * union) > 1e-6 away from 0.5 unless it IS 0.5, so float32 and float64 agree on the comparison."""
    from odvae_amd.patches import crop_is_background
    assert crop_is_background((10, 20, 100), []) and crop_is_background((10, 20, 100), np.zeros((0, 4)))
    assert not crop_is_background((0, 0, 100), [[0, 0, 100, 50]])                         # IoU == 0.5 exactly: not < 0.5
    assert crop_is_background((0, 0, 100), [[0, 0, 100, 49.5]])
    assert not crop_is_background((0, 0, 100), [[300, 300, 310, 310], [0, 0, 100, 51]])    # one overlapping box is enough
    assert crop_is_background((0, 0, 50), [[0, 0, 400, 400]])                              # a small crop inside a big box: IoU 1/64
    rng = np.random.default_rng(5)
    accepted = 0
    for _ in range(400):
        size = int(rng.choice([50, 100, 200, 400]))
        x, y = int(rng.integers(0, 1600 - size + 1)), int(rng.integers(0, 900 - size + 1))
        boxes = []
        for _ in range(int(rng.integers(1, 5))):
            bx, by = x + int(rng.integers(-size // 3, size // 3)), y + int(rng.integers(-size // 3, size // 3))
            boxes.append([bx, by, bx + int(rng.integers(size, 3 * size)) / 2, by + int(rng.integers(size, 3 * size)) / 2])
        want = all(_iou([x, y, x + size, y + size], b) < 0.5 for b in boxes)
        assert crop_is_background((x, y, size), boxes) == want, (x, y, size, boxes)
        accepted += want
    assert 40 < accepted < 360
