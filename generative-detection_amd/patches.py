"""Object-patch extraction on the GPU: the step right before the hot path.

The reference cuts one square patch per annotated object out of a decoded camera image with PIL, resizes it to the
network resolution and rasterises the object's 2-d box into a mask (src/data/datasets/nuscenes.py:90-194, one Python call
per instance inside DataLoader workers).  Here the decoded u8 camera images live in HBM and one kernel launch produces the
whole batch: `patch` [B,3,S,S] f32 in [0,1] (channels_last) and `mask_2d_bbox` [B,1,S,S], bit-identical to the PIL path
(csrc/patch_u8.hip).  JPEG decoding, annotation parsing and the pose targets stay where they are (out of scope).

Host side, per instance (plain integer arithmetic, no device sync):
  * `plan_patch`   -- which square to cut: nuscenes.py:97-158 (centre rejection, square box around the floored projected
                      centre, snapping to PATCH_SIZES under `perturb_scale`, the four border clamps, padding pixels)
  * `mask_slice`   -- numpy's slice rule for `mask_bool[y1:y2, x1:x2] = True` (:178-187; negative starts wrap, as there)
  * `resample_table` -- Pillow's coefficient windows for (crop size -> S), cached per crop size
  * `reduced_resample_table` -- the same behind Pillow's box pre-reduction (`reducing_gap=1.0`, crop size >= 2 S), with
                      `reduce_multipliers` for the reduce itself (GpuPatcher(box_reduce=True))
  * `crop_is_background` -- the acceptance rule for a background square (nuscenes.py:585-595); `backgrounds=` cuts them
"""
import math

import numpy as np
import torch

from . import lib as _lib

PATCH_SIZES = (50, 100, 200, 400)   # nuscenes.py:55
PRECISION_BITS = 32 - 8 - 2         # Pillow Resample.c (8 bits per channel)


def snap_to_patch_size(extent):
    """Closest entry of PATCH_SIZES, the first one on ties (`list.index(min(...))`, nuscenes.py:129-130,140-141)."""
    best = PATCH_SIZES[0]
    for s in PATCH_SIZES[1:]:
        if abs(extent - s) < abs(extent - best):
            best = s
    return best


class PatchPlan:
    """Crop square [x1, x1+size) x [y1, y1+size) in camera-image pixels + what the caller derives from it."""
    __slots__ = ("x1", "y1", "size", "padding_pixels", "mask_x", "mask_y")

    def __init__(self, x1, y1, size, padding_pixels, mask_x, mask_y):
        self.x1, self.y1, self.size, self.padding_pixels, self.mask_x, self.mask_y = x1, y1, size, padding_pixels, mask_x, mask_y


def mask_slice(lo, hi, n):
    """(start, stop) that `array[lo:hi]` addresses on an axis of length n (Python slice semantics, step 1)."""
    start, stop, _ = slice(lo, hi).indices(n)
    return start, max(stop, start)


def plan_patch(bbox, center_2d, img_w, img_h, perturb_scale):
    """The crop the reference takes for one object, or None where it drops the instance (nuscenes.py:97-166).
    bbox = [x1, y1, x2, y2] floats (exterior rectangle of the projected 3-d box), center_2d = projected centre."""
    cx, cy = float(center_2d[0]), float(center_2d[1])
    if cx < 0 or cy < 0 or cx >= img_w or cy >= img_h:          # :102-103  less than half of the object visible
        return None
    bx1, by1, bx2, by2 = (int(v) for v in bbox)                   # :109  truncation toward zero
    width, height = bx2 - bx1, by2 - by1
    size = max(width, height)
    ccx, ccy = int(math.floor(cx)), int(math.floor(cy))
    outside = bx1 >= img_w or by1 >= img_h or bx2 <= 0 or by2 <= 0
    if outside:                                                   # :117-136  only width/height survive this branch
        width = min(img_w, bx2) - max(0, bx1)
        height = min(img_h, by2) - max(0, by1)
    elif perturb_scale:                                           # :138-150
        size = snap_to_patch_size(size)
        half = size // 2
        if ccx - half < 0:
            ccx = half
        if ccy - half < 0:
            ccy = half
        if ccx + half > img_w:
            ccx = img_w - half
        if ccy + half > img_h:
            ccy = img_h - half
    half = size // 2
    side = 2 * half                                               # :157-160  (c - half, c + half)
    if side <= 0:                                                 # PIL raises / divides by zero -> instance dropped (:164-174)
        return None
    x1, y1 = ccx - half, ccy - half
    pad = width - height if width > height else 0                 # :152-155
    # :181-187  bbox corners relative to the crop, truncated, then numpy slice assignment on a (side, side) array
    mx = mask_slice(int(float(bbox[0]) - x1), int(float(bbox[2]) - x1), side)
    my = mask_slice(int(float(bbox[1]) - y1), int(float(bbox[3]) - y1), side)
    return PatchPlan(x1, y1, side, pad, mx, my)


def resample_table(in_size, out_size):
    """int32 [out_size][8] = {k0..k4, first source index, taps, nearest source index}: Pillow's BILINEAR windows for
    in_size -> out_size (Resample.c precompute_coeffs + normalize_coeffs_8bpc, evaluated in f64 in the same operation
    order) and the NEAREST source index (Geometry.c ImagingScaleAffine: xo = scale/2, then xo += scale per step)."""
    if in_size >= 2 * out_size:
        raise ValueError("crop %d -> %d: Image.resize(reducing_gap=1.0) would box-reduce first; not supported" % (in_size, out_size))
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                    # bilinear support 1.0
    inv = 1.0 / filterscale
    idx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (idx + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    taps = last - first
    assert taps.max() <= 5
    w = np.zeros((out_size, 5), np.float64)
    total = np.zeros(out_size, np.float64)
    for t in range(5):
        a = np.abs(((t + first).astype(np.float64) - center + 0.5) * inv)
        wt = np.where((a < 1.0) & (t < taps), 1.0 - a, 0.0)
        w[:, t] = wt
        total = total + wt                                        # left-to-right accumulation, as the C loop
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    tab = np.zeros((out_size, 8), np.int32)
    tab[:, :5] = k
    tab[:, 5] = first
    tab[:, 6] = taps
    xo = 0.0 + scale * 0.5
    for i in range(out_size):
        tab[i, 7] = int(xo)
        xo += scale
    return tab


def reduced_resample_table(in_size, out_size):
    """(f, table) for `Image.resize((out_size, out_size), BILINEAR, reducing_gap=1.0)` on a square of side in_size: Pillow
    first box-reduces by f = int(in_size / out_size) or 1 (Image.py resize) to side r = ceil(in_size / f), then resamples
    from the reduced image with the source box [0, in_size / f) -- handed to C as float32 -- clipped to [0, r).  The table
    has the layout of `resample_table`, windows over the REDUCED image; column 7 (the NEAREST index of the box mask, which
    is never pre-reduced) stays the in_size -> out_size walk.  f == 1: `resample_table` itself."""
    f = int(in_size / out_size) or 1
    if f == 1:
        return 1, resample_table(in_size, out_size)
    r = -(-in_size // f)
    in1 = float(np.float32(in_size / f))
    scale = in1 / out_size                                         # < 2: at most 5 taps, as resample_table
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    inv = 1.0 / filterscale
    idx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (idx + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), r)
    taps = last - first
    assert 1 <= taps.min() and taps.max() <= 5
    w = np.zeros((out_size, 5), np.float64)
    total = np.zeros(out_size, np.float64)
    for t in range(5):
        a = np.abs(((t + first).astype(np.float64) - center + 0.5) * inv)
        wt = np.where((a < 1.0) & (t < taps), 1.0 - a, 0.0)
        w[:, t] = wt
        total = total + wt
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    tab = np.zeros((out_size, 8), np.int32)
    tab[:, :5] = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    tab[:, 5] = first
    tab[:, 6] = taps
    step = float(in_size) / out_size
    xo = 0.0 + step * 0.5
    for i in range(out_size):
        tab[i, 7] = int(xo)
        xo += step
    return f, tab


def reduce_multiplier(n):
    """Pillow Reduce.c division_UINT32(n, 8): (ss + n/2) * this >> 24 is the rounded mean of n bytes in u32 arithmetic."""
    return int(np.float32(4294967296.0) / np.float32(256 * n))


def reduce_multipliers(in_size, f):
    """uint32 [4] = {mult(f*f), mult(f*rem), mult(rem*rem), 0}: full boxes, the narrower last column / row (rem = its width,
    == f where f divides in_size) and their corner.  A partial box averages over the pixels it has (ImagingReduceCorners)."""
    rem = in_size - (-(-in_size // f) - 1) * f
    return np.asarray([reduce_multiplier(f * f), reduce_multiplier(f * rem), reduce_multiplier(rem * rem), 0], np.uint32)


def crop_is_background(square, bboxes):
    """Whether `get_random_crop_without_overlap` (nuscenes.py:585-595) accepts the square (x, y, size) as a background crop:
    its IoU with every [x1, y1, x2, y2] box is < 0.5, or there are no boxes.  float32 like torchvision's box_iou on the
    reference's float tensors.  The random draw of the square stays with the caller."""
    x, y, size = square
    if len(bboxes) == 0:
        return True
    c = np.asarray([x, y, x + size, y + size], np.float32)
    bb = np.asarray(bboxes, np.float32).reshape(-1, 4)
    wh = np.maximum(np.minimum(c[2:], bb[:, 2:]) - np.maximum(c[:2], bb[:, :2]), np.float32(0))
    inter = wh[:, 0] * wh[:, 1]
    area_c = (c[2] - c[0]) * (c[3] - c[1])
    area_b = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area_c + area_b - inter)
    return bool(np.all(iou < np.float32(0.5)))


class PatchBatch:
    """What `_generate_patch` returns, batched: patch [n,3,S,S], mask [n,1,S,S] (device), patch_size [n,2] f32 (w, h) of
    the crop, resampling_factor [(fx, fy)], padding_pixels_resampled [n] and `kept` = indices of the instances that
    were not dropped.  Background rows follow the object rows: `background` [n] bools says which rows they are; theirs are
    patch_size (S, S) (the reference stores the network size there, nuscenes.py:549), an all-zero mask and no padding."""
    __slots__ = ("patch", "mask", "patch_size", "resampling_factor", "padding_pixels_resampled", "kept", "plans", "background")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class GpuPatcher:
    """`box_reduce=False` (default) refuses a crop of side >= 2 S with ValueError; `box_reduce=True` takes it the way Pillow's
    `reducing_gap=1.0` does (box-reduce by int(side / S), then bilinear from the reduced image), on the device in the same
    launch.  The reference always behaves like `box_reduce=True`."""

    def __init__(self, patch_height=256, patch_aspect_ratio=1.0, perturb_scale=False, device="cuda:0", box_reduce=False):
        self.size = (patch_height, int(patch_height * patch_aspect_ratio))   # nuscenes.py:67
        if self.size[0] != self.size[1]:
            raise ValueError("the reference asserts equal resampling factors (nuscenes.py:172): square patches only")
        self.S = int(patch_height)
        self.perturb_scale = bool(perturb_scale)
        self.box_reduce = bool(box_reduce)
        self.device = torch.device(device)
        self._slot = {}
        self._host_tables = []
        self._host_mults = []
        self._factors = []
        self._tables = None

    def _table_slot(self, crop, reduce):
        """Slot of the tables for one crop size; `reduce` = resize with reducing_gap (objects) or without (backgrounds).  The two
        differ only for crop >= 2 S, where the plain resize is refused."""
        reduce = reduce and crop >= 2 * self.S
        slot = self._slot.get((crop, reduce))
        if slot is None:
            f, tab = reduced_resample_table(crop, self.S) if reduce else (1, resample_table(crop, self.S))
            slot = self._slot[(crop, reduce)] = len(self._host_tables)
            self._host_tables.append(tab)
            self._host_mults.append(reduce_multipliers(crop, f))
            self._factors.append(f)
            self._tables = None
        return slot

    def _device_tables(self):
        if self._tables is None:
            self._tables = (torch.from_numpy(np.stack(self._host_tables)).to(self.device),
                            torch.from_numpy(np.stack(self._host_mults).view(np.int32)).to(self.device))
        return self._tables

    def __call__(self, images, instances, backgrounds=()):
        """images: list of u8 [H,W,3] tensors on the device (decoded camera images); instances: iterable of
        (image_index, bbox[4], center_2d[2]); backgrounds: iterable of (image_index, x, y, size), explicit squares
        [x, x+size) x [y, y+size) cut like the reference's background samples (nuscenes.py:539-560): plain BILINEAR resize
        without `reducing_gap`, all-zero mask.  A background of side >= 2 S would need windows wider than the kernel's 5
        taps and raises ValueError (it cannot happen at S >= 201 with PATCH_SIZES <= 400).  One launch for all kept
        instances and all backgrounds."""
        staged = self.stage(images, instances, backgrounds)
        return self.launch(staged) if staged["n"] else PatchBatch(
            patch=None, mask=None, patch_size=None, resampling_factor=[], padding_pixels_resampled=[], kept=[], plans=[], background=[])

    def _check_image(self, img):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous() or not 6 <= img.numel() < 2 ** 31:
            raise ValueError("camera images must be contiguous u8 [H,W,3] tensors")
        if not img.is_cuda:
            raise _lib.HipLibraryError("camera images must live on the HIP device (no CPU fallback), got %s" % img.device)

    def stage(self, images, instances, backgrounds=()):
        """Host half: plan every instance and ship pointers, geometry and mask rectangles in one H2D copy."""
        plans, kept = [], []
        for i, (img_idx, bbox, center) in enumerate(instances):
            img = images[img_idx]
            self._check_image(img)
            plan = plan_patch(bbox, center, img.shape[1], img.shape[0], self.perturb_scale)
            if plan is not None:
                plans.append((img_idx, plan, self.box_reduce))
                kept.append(i)
        n_obj = len(plans)
        for img_idx, x, y, size in backgrounds:
            self._check_image(images[img_idx])
            if int(size) <= 0:
                raise ValueError("background square of side %r" % (size,))
            if int(size) >= 2 * self.S:
                raise ValueError("background %d -> %d: a plain BILINEAR resize (no reducing_gap) needs windows wider than 5 taps; "
                                 "not supported" % (size, self.S))
            plans.append((img_idx, PatchPlan(int(x), int(y), int(size), 0, (0, 0), (0, 0)), False))   # empty mask rectangle
        n = len(plans)
        if n == 0:
            return {"n": 0}
        # staging buffer: [n] pointers (8 B) | [n][8] geometry | [n][4] mask rectangle
        ptr_bytes = (8 * n + 15) // 16 * 16
        host = np.zeros(ptr_bytes + 32 * n + 16 * n, np.uint8)
        ptrs = host[:8 * n].view(np.int64)
        geom = host[ptr_bytes:ptr_bytes + 32 * n].view(np.int32).reshape(n, 8)
        rect = host[ptr_bytes + 32 * n:].view(np.int32).reshape(n, 4)
        for j, (img_idx, plan, reduce) in enumerate(plans):
            img = images[img_idx]
            slot = self._table_slot(plan.size, reduce)
            ptrs[j] = img.data_ptr()
            geom[j, :7] = (img.shape[0], img.shape[1], plan.x1, plan.y1, plan.size, slot, self._factors[slot])
            rect[j] = (plan.mask_x[0], plan.mask_x[1], plan.mask_y[0], plan.mask_y[1])
        return {"n": n, "n_obj": n_obj, "ptr_bytes": ptr_bytes, "dev": torch.from_numpy(host).to(self.device, non_blocking=True),
                "tables": self._device_tables(), "plans": [p for _, p, _ in plans], "kept": kept,
                "reduced": bool((geom[:, 6] > 1).any()),
                "images": [images[k] for k, _, _ in plans]}   # keeps the camera images alive until the launch is issued

    def launch(self, staged, entry=None):
        """Device half: one kernel launch on the current stream.  entry: "crop" = odvae_patch_crop_resize_u8 (no instance may
        have a reduce factor > 1), "reduce" = odvae_patch_reduce_resize_u8 (any batch); None picks by the batch."""
        L = _lib.load()
        n, n_obj, S, plans = staged["n"], staged["n_obj"], self.S, staged["plans"]
        entry = entry or ("reduce" if staged["reduced"] else "crop")
        if entry not in ("crop", "reduce") or (entry == "crop" and staged["reduced"]):
            raise ValueError("entry %r cannot run this batch" % (entry,))
        patch = torch.empty((n, S, S, 3), dtype=torch.float32, device=self.device)
        mask = torch.empty((n, 1, S, S), dtype=torch.float32, device=self.device)
        base, (tables, mults) = staged["dev"].data_ptr(), staged["tables"]
        args = (base, base + staged["ptr_bytes"], base + staged["ptr_bytes"] + 32 * n, tables.data_ptr())
        tail = (tables.shape[0], n, S, patch.data_ptr(), mask.data_ptr(), _lib.stream_ptr())
        if entry == "reduce":
            _lib.check(L.odvae_patch_reduce_resize_u8(*args, mults.data_ptr(), *tail), "patch_reduce_resize")
        else:
            _lib.check(L.odvae_patch_crop_resize_u8(*args, *tail), "patch_crop_resize")
        background = [j >= n_obj for j in range(n)]
        factor = [(S / p.size, S / p.size) for p in plans]
        return PatchBatch(patch=patch.permute(0, 3, 1, 2), mask=mask,
                          patch_size=torch.tensor([[S, S] if bg else [p.size, p.size] for p, bg in zip(plans, background)], dtype=torch.float32),
                          resampling_factor=factor,
                          padding_pixels_resampled=[p.padding_pixels * f[0] for p, f in zip(plans, factor)],
                          kept=staged["kept"], plans=plans, background=background)
