"""Patch extraction with Pillow's box pre-reduction on the device (csrc/patch_u8.hip, odvae_patch_reduce_resize_u8, through
GpuPatcher(box_reduce=True)) and background squares, against Pillow itself (oracle/patches.py generate_patch_pil goes through
`Image.resize(BILINEAR, reducing_gap=1.0)`) and against the reference's own run (tests/golden/reference_patches.npz).
Byte work: the bar is bit-exact, no tolerance anywhere."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PIL_Image = pytest.importorskip("PIL.Image")

from test_patches import _ref_gold, random_instances  # noqa: E402

IMAGE_HW = [(120, 150), (300, 333)]


def _images(rng, shapes):
    imgs = []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)), ((xx + yy) % 256)], -1).astype(np.uint8)
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        imgs.append(np.where(rng.random((h, w, 1)) < 0.5, smooth, noise).astype(np.uint8))
    return imgs


def mixed_instances(rng, S):
    """Per image: extents up to the whole image (f = 1 ... image side / S, every remainder), boxes over all four borders, small
    boxes (f = 1), and small boxes wholly outside the image with the centre inside (the reference's corner case, never snapped to
    PATCH_SIZES: the f = 1 instances of a `perturb_scale` batch at S = 16 / 24)."""
    inst = []
    for k, (h, w) in enumerate(IMAGE_HW):
        for bbox, center in random_instances(rng, 14, w, h, max_extent=max(h, w)):
            inst.append((k, bbox, center))
        for bbox, center in random_instances(rng, 6, w, h, max_extent=2 * S - 2)[:6]:
            inst.append((k, bbox, center))
        e = S + 3.0
        inst += [(k, [w + 2.0, 10.0, w + 2.0 + e, 10.0 + e], [w - 1.5, 20.0]), (k, [-e - 3.0, 30.0, -3.0, 30.0 + e], [0.5, 40.0]),
                 (k, [20.0, h + 1.0, 20.0 + e, h + 1.0 + e], [30.0, h - 0.5]), (k, [40.0, -e - 2.0, 40.0 + e, -2.0], [50.0, 1.0]),
                 (k, [0.0, 0.0, float(w), float(h)], [w / 2, h / 2]), (k, [-30.0, -20.0, w + 25.0, h + 35.0], [w / 2 + 0.4, h / 2 + 0.6])]
    return inst


def _check_against_pil(out, refs, inst):
    kept = [i for i, r in enumerate(refs) if r[0] is not None]
    assert out.kept == kept
    patch, mask = out.patch.cpu().numpy(), out.mask.cpu().numpy()
    for j, i in enumerate(kept):
        ref = refs[i]
        assert np.array_equal(patch[j], ref[0]), ("patch", i, inst[i], out.plans[j].size)
        assert np.array_equal(mask[j], ref[4]), ("mask", i, inst[i], out.plans[j].size)
        assert np.array_equal(out.patch_size[j].numpy(), ref[1])
        assert out.resampling_factor[j] == ref[2]
        assert out.padding_pixels_resampled[j] == ref[3]
        assert out.background[j] is False


@pytest.mark.parametrize("perturb_scale", [False, True])
@pytest.mark.parametrize("S", [16, 24, 80, 96])
def test_reduced_patch_batch_is_bit_identical_to_pil(hip_lib, S, perturb_scale):
    """f = 1 and f > 1 instances in one launch.  S = 80 / 96 put the seam between two 64-column blocks inside a reduced window."""
    from odvae_amd.patches import GpuPatcher
    from oracle import patches as oracle
    rng = np.random.default_rng(100 + S)
    host_imgs = _images(rng, IMAGE_HW)
    dev_imgs = [torch.from_numpy(a).to("cuda:0") for a in host_imgs]
    inst = mixed_instances(rng, S)
    out = GpuPatcher(patch_height=S, perturb_scale=perturb_scale, box_reduce=True)(dev_imgs, inst)
    torch.cuda.synchronize()
    factors = [p.size // S or 1 for p in out.plans]
    assert sum(f >= 2 for f in factors) >= 8 and sum(f == 1 for f in factors) >= 4, factors
    if not perturb_scale:
        assert len({p.size % f for p, f in zip(out.plans, factors) if f >= 2}) >= (6 if S <= 24 else 2)   # remainders size % f
    assert out.patch.shape == (len(out.kept), 3, S, S) and out.patch.is_contiguous(memory_format=torch.channels_last)
    refs = [oracle.generate_patch_pil(host_imgs[k], bbox, center, (S, S), perturb_scale) for k, bbox, center in inst]
    _check_against_pil(out, refs, inst)
    assert len(out.kept) < len(inst)


@pytest.mark.parametrize("perturb", [False, True])
def test_reduced_patches_match_the_reference_run(hip_lib, perturb):
    """Every instance of the reference-run fixture in ONE call with box_reduce=True, the crops >= 2 S among them (the ones
    tests/test_patches_gpu.py sees refused at the default): u8 patch and mask CRC-32 as the reference's own `_generate_patch` wrote
    them, for the large crops and, unchanged, for the small ones."""
    from odvae_amd.patches import GpuPatcher
    g, rc = _ref_gold()
    S, p = int(g["S"]), int(perturb)
    assert S == 96
    dev_img = torch.from_numpy(rc.patch_image()).to("cuda:0")
    out = GpuPatcher(patch_height=S, perturb_scale=perturb, box_reduce=True)([dev_img], [(0, b, c) for b, c in rc.patch_instances()])
    torch.cuda.synchronize()
    kept = list(g["p%d.kept" % p])
    assert out.kept == kept
    big = [i for i, plan in zip(kept, out.plans) if plan.size >= 2 * S]
    assert big == ([10, 13, 16, 20, 25, 26, 32, 35] if perturb else [13])
    patch = (out.patch.cpu().numpy() * 255.0).round().astype(np.uint8)
    mask = out.mask.cpu().numpy().round().astype(np.uint8)
    for j, i in enumerate(kept):
        pre = "p%d.%d" % (p, i)
        assert np.array_equal(patch[j].astype(np.float32) / np.float32(255), out.patch[j].cpu().numpy())      # the f32 values ARE u8 / 255
        assert zlib.crc32(np.ascontiguousarray(patch[j]).tobytes()) == int(g[pre + ".patch_crc"]), i
        assert zlib.crc32(np.ascontiguousarray(mask[j]).tobytes()) == int(g[pre + ".mask_crc"]), i
        assert np.array_equal(out.patch_size[j].numpy(), g[pre + ".size_sq"])
        assert tuple(out.resampling_factor[j]) == tuple(g[pre + ".factor"])
        assert float(out.padding_pixels_resampled[j]) == float(g[pre + ".padding_resampled"])


@pytest.mark.parametrize("S", [24, 96])
def test_no_large_crop_gives_the_same_bits_either_way(hip_lib, S):
    """A batch without a crop >= 2 S: box_reduce=True and False give identical tensors, and so do the two entry points on the very
    same staged batch (f = 1 through the LDS kernel = the bits of the existing kernel)."""
    from odvae_amd.patches import GpuPatcher
    rng = np.random.default_rng(7 + S)
    host_imgs = _images(rng, IMAGE_HW)
    dev_imgs = [torch.from_numpy(a).to("cuda:0") for a in host_imgs]
    inst = [(k, bbox, center) for k, (h, w) in enumerate(IMAGE_HW) for bbox, center in random_instances(rng, 16, w, h, max_extent=2 * S - 2)]
    inst = [(k, b, c) for k, b, c in inst if max(int(b[2]) - int(b[0]), int(b[3]) - int(b[1])) < 2 * S]
    plain = GpuPatcher(patch_height=S)
    reducing = GpuPatcher(patch_height=S, box_reduce=True)
    a, b = plain(dev_imgs, inst), reducing(dev_imgs, inst)
    assert len(a.kept) >= 12 and a.kept == b.kept and max(p.size for p in a.plans) < 2 * S
    assert torch.equal(a.patch, b.patch) and torch.equal(a.mask, b.mask)
    staged = reducing.stage(dev_imgs, inst)
    c, d = reducing.launch(staged, entry="crop"), reducing.launch(staged, entry="reduce")
    assert torch.equal(c.patch, a.patch) and torch.equal(c.mask, a.mask)
    assert torch.equal(d.patch, a.patch) and torch.equal(d.mask, a.mask)
    assert a.mask.sum().item() > 0 and a.patch.std().item() > 0.05


@pytest.mark.parametrize("box_reduce", [False, True])
@pytest.mark.parametrize("S,sizes", [(128, (50, 100, 200)), (256, (400,))])
def test_backgrounds_ride_with_the_objects(hip_lib, S, sizes, box_reduce):
    """Background squares = Image.crop(...).resize((S, S), BILINEAR) WITHOUT reducing_gap, all-zero mask, patch_size (S, S),
    resampling_factor S / size (nuscenes.py:539-560), in the same call as objects (one of them box-reduced where allowed)."""
    from odvae_amd.patches import GpuPatcher
    from oracle import patches as oracle
    rng = np.random.default_rng(31 + S)
    (img,) = _images(rng, [(450, 800)])
    dev = [torch.from_numpy(img).to("cuda:0")]
    objects = [(0, [100.2, 80.7, 180.9, 150.1], [140.5, 115.3]), (0, [600.0, 300.0, 790.0, 440.0], [700.0, 380.0])]
    if box_reduce:
        objects.append((0, [10.0, 10.0, 10.0 + 2 * S + 44, 380.0], [10.0 + S + 22, 195.0]))     # box-reduced: f = 2
    backgrounds = [(0, int(rng.integers(0, 800 - s + 1)), int(rng.integers(0, 450 - s + 1)), s) for s in sizes for _ in range(2)]
    backgrounds.append((0, 800 - sizes[0] // 2, -7, sizes[0]))                                     # hangs over two borders: zero fill
    out = GpuPatcher(patch_height=S, box_reduce=box_reduce)(dev, objects, backgrounds=backgrounds)
    torch.cuda.synchronize()
    n_obj = len(objects)
    assert out.kept == list(range(n_obj)) and out.background == [False] * n_obj + [True] * len(backgrounds)
    assert out.patch.shape == (n_obj + len(backgrounds), 3, S, S)
    refs = [oracle.generate_patch_pil(img, bbox, center, (S, S), False) for _, bbox, center in objects]
    patch, mask = out.patch.cpu().numpy(), out.mask.cpu().numpy()
    for j, ref in enumerate(refs):
        assert np.array_equal(patch[j], ref[0]) and np.array_equal(mask[j], ref[4]), j
        assert np.array_equal(out.patch_size[j].numpy(), ref[1])
    pil = PIL_Image.fromarray(img)
    for j, (_, x, y, s) in enumerate(backgrounds, start=n_obj):
        ref = np.asarray(pil.crop((x, y, x + s, y + s)).resize((S, S), resample=PIL_Image.Resampling.BILINEAR))
        assert np.array_equal(patch[j], oracle.to_tensor(ref)), (x, y, s)
        assert not mask[j].any()
        assert out.patch_size[j].tolist() == [S, S] and out.resampling_factor[j] == (S / s, S / s)
        assert out.padding_pixels_resampled[j] == 0


def test_oversize_background_is_refused(hip_lib):
    from odvae_amd.patches import GpuPatcher
    img = torch.zeros((450, 800, 3), dtype=torch.uint8, device="cuda:0")
    for box_reduce in (False, True):
        with pytest.raises(ValueError):
            GpuPatcher(patch_height=128, box_reduce=box_reduce)([img], [], backgrounds=[(0, 10, 10, 400)])
    with pytest.raises(ValueError):                                                               # the default refusal of objects stays
        GpuPatcher(patch_height=128)([img], [(0, [100.0, 100.0, 500.0, 400.0], [300.0, 250.0])])
    out = GpuPatcher(patch_height=128, box_reduce=True)([img], [(0, [100.0, 100.0, 500.0, 400.0], [300.0, 250.0])])
    assert out.plans[0].size == 400 and out.patch.shape == (1, 3, 128, 128)


def test_every_byte_value_through_an_f2_reduce(hip_lib):
    """128 x 128 image, S = 64: f = 2 and then a 64 -> 64 identity resize.  Every 2 x 2 box is constant, so all 256 byte values come
    out of the reduce exactly and go through u8 -> f32 / 255; a second image with a +1 / -1 checker inside each box rounds .5 up."""
    from odvae_amd.patches import GpuPatcher
    yy, xx = np.mgrid[0:128, 0:128]
    base = ((yy // 2) * 64 + xx // 2)[:, :, None] + np.asarray([0, 85, 170])[None, None, :]
    flat = (base % 256).astype(np.uint8)
    bump = np.clip((base % 256) + ((xx + yy) % 2 == 0)[:, :, None] * 1, 0, 255).astype(np.uint8)   # box sums 4 v + 2 -> v + 1 after + n/2
    dev = [torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(bump).to("cuda:0")]
    whole = ([0.0, 0.0, 128.0, 128.0], [64.0, 64.0])
    out = GpuPatcher(patch_height=64, box_reduce=True)(dev, [(0,) + whole, (1,) + whole])
    torch.cuda.synchronize()
    assert [p.size for p in out.plans] == [128, 128] and out.mask.min().item() == 1.0
    for j, img in enumerate((flat, bump)):
        ref = np.asarray(PIL_Image.fromarray(img).resize((64, 64), resample=PIL_Image.Resampling.BILINEAR, reducing_gap=1.0))
        want = torch.from_numpy(ref.copy()).permute(2, 0, 1).to(torch.float32).div(255)
        assert torch.equal(out.patch[j].cpu(), want)
        assert len(np.unique(ref)) == (256 if j == 0 else 255)
    assert np.array_equal((out.patch[0].cpu().numpy() * 255).round().astype(np.uint8).transpose(1, 2, 0), flat[::2, ::2])
