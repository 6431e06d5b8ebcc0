"""The ResnetBlock dropout mask on the host (odvae_amd/dropout_mask.py, the numpy restatement of csrc/dropout_mask.h) and the module
surface of `ddconfig.dropout`.  No GPU: the kernels are held to this module bit for bit in tests/test_resnet_dropout_gpu.py, so what is
checked here is the definition itself -- Philox4x32-10 against the Random123 known answers, the threshold rule, seeds and indices."""
import math

import numpy as np
import pytest
import torch

N_ELEMS = 1 << 20


def _lanes(seed, octets=N_ELEMS // 8, first=0):
    from odvae_amd import dropout_mask as dm
    return dm.dropout_lanes(seed, first, octets)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox4x32_10_known_answers(counter, key, want):
    """The Random123 kat_vectors of philox4x32 with 10 rounds."""
    from odvae_amd import dropout_mask as dm
    got = dm.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want
    # vectorised: the same words when the call is one row of an array
    c = [np.array([1, v, 2], dtype=np.uint64) for v in counter]
    k = [np.array([3, v, 4], dtype=np.uint64) for v in key]
    assert tuple(int(v[1]) for v in dm.philox4x32_10(c, k)) == want


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_fraction(p):
    """2^20 elements: the kept fraction within 5 sigma of 1 - thr / 65536 (a binomial with that success rate if the lanes are uniform)."""
    from odvae_amd import dropout_mask as dm
    n, c, h, w = 4, 64, 64, 64
    assert n * c * h * w == N_ELEMS
    keep = dm.resnet_dropout_keep(12345, p, n, c, h, w)
    assert keep.shape == (n, c, h, w) and keep.dtype == torch.float32
    vals = set(keep.unique().tolist())
    assert vals == {0.0, float(dm.dropout_scale(p))}
    frac = (keep != 0).double().mean().item()
    want = 1.0 - dm.dropout_threshold(p) / 65536.0
    sigma = math.sqrt(p * (1 - p) / N_ELEMS)
    print("p=%.1f kept %.6f want %.6f (%.2f sigma)" % (p, frac, want, abs(frac - want) / sigma))
    assert abs(frac - want) <= 5 * sigma


def test_mask_layout_is_nhwc_octets():
    """Element (n, c, y, x) of the logical-NCHW mask is lane c % 8 of octet ((n * HW + y * W + x) * C + c) / 8."""
    from odvae_amd import dropout_mask as dm
    n, c, h, w, p, seed = 2, 32, 5, 7, 0.5, 99
    keep = dm.resnet_dropout_keep(seed, p, n, c, h, w)
    lanes = _lanes(seed, n * h * w * c // 8).reshape(n, h, w, c)
    want = torch.from_numpy((lanes >= dm.dropout_threshold(p)).astype(np.float32) * 2.0).permute(0, 3, 1, 2)
    assert torch.equal(keep, want)
    # one element by hand through the scalar call
    ni, ci, yi, xi = 1, 13, 3, 4
    g = ((ni * h * w + yi * w + xi) * c + ci) // 8
    words = dm.philox4x32_10((g, 0, 0, 0), (seed, 0))
    word = int(words[(ci % 8) // 2])
    lane = (word >> 16) if ci % 2 else (word & 0xFFFF)
    assert (keep[ni, ci, yi, xi].item() != 0) == (lane >= dm.dropout_threshold(p))


def test_edge_values_of_p():
    from odvae_amd import dropout_mask as dm
    assert dm.dropout_threshold(0.0) == 0 and dm.dropout_threshold(1.0) == 65536
    assert dm.dropout_scale(0.0) == 1.0 and dm.dropout_scale(1.0) == 0.0
    assert dm.dropout_scale(0.5) == 2.0 and dm.dropout_scale(0.75) == 4.0
    assert dm.dropout_scale(0.1) == np.float32(1.0 / 0.9)
    k0 = dm.resnet_dropout_keep(7, 0.0, 2, 32, 4, 4)
    assert torch.equal(k0, torch.ones(2, 32, 4, 4))
    k1 = dm.resnet_dropout_keep(7, 1.0, 2, 32, 4, 4)
    assert torch.equal(k1, torch.zeros(2, 32, 4, 4)) and torch.isfinite(k1).all()      # scale 0, not inf * 0
    # a lane of 0xFFFF is kept for every p < 1 and dropped at p = 1: the compare is wider than 16 bits
    assert dm.dropout_threshold(1.0) > 0xFFFF
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            dm.dropout_threshold(bad)
        with pytest.raises(ValueError):
            dm.resnet_dropout_keep(7, bad, 2, 32, 4, 4)
    with pytest.raises(ValueError):
        dm.resnet_dropout_keep(7, 0.5, 2, 12, 4, 4)      # C % 8 != 0


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_two_seeds_agree_like_independent_masks(p):
    """Independent masks agree (both kept or both dropped) on (1 - q)^2 + q^2 of the elements, q = thr / 65536; 5 sigma of that binomial."""
    from odvae_amd import dropout_mask as dm
    thr = dm.dropout_threshold(p)
    a, b = _lanes(1) >= thr, _lanes(2) >= thr
    q = thr / 65536.0
    want = (1 - q) ** 2 + q ** 2
    got = float((a == b).mean())
    sigma = math.sqrt(want * (1 - want) / N_ELEMS)
    print("p=%.1f agree %.6f want %.6f (%.2f sigma)" % (p, got, want, abs(got - want) / sigma))
    assert abs(got - want) <= 5 * sigma
    # the seed's high word is part of the key
    assert not np.array_equal(_lanes(1, 64), _lanes(1 + (1 << 32), 64))
    assert np.array_equal(_lanes(1, 64), _lanes(1 + (1 << 64), 64))      # the seed is a 64-bit integer


def test_high_word_of_the_octet_index_changes_the_output():
    """counter = (lo32(g), hi32(g), 0, 0).  This is the ONLY place the high word is exercised: no tensor that fits a test reaches 2^32
    octets (2^35 elements), so the kernels' 64-bit index arithmetic above 2^32 is checked against nothing but this definition."""
    from odvae_amd import dropout_mask as dm
    lo = _lanes(5, 16, first=3)
    hi = _lanes(5, 16, first=3 + (1 << 32))
    assert not np.array_equal(lo, hi)
    w = dm.philox4x32_10((3, 1, 0, 0), (5, 0))
    assert int(w[0]) & 0xFFFF == int(hi[0, 0]) and int(w[3]) >> 16 == int(hi[0, 7])
    # consecutive octets across the 2^32 boundary are distinct calls
    edge = _lanes(5, 2, first=(1 << 32) - 1)
    assert np.array_equal(edge[0], _lanes(5, 1, first=(1 << 32) - 1)[0]) and np.array_equal(edge[1], _lanes(5, 1, first=1 << 32)[0])


def test_module_surface():
    from odvae_amd import modules
    block = modules.ResnetBlock(in_channels=64, dropout=0.1, temb_channels=0)
    assert isinstance(block.dropout, torch.nn.Dropout) and block.dropout.p == 0.1 and block.last_dropout_seed is None
    plain = modules.ResnetBlock(in_channels=64, dropout=0.0, temb_channels=0)
    assert list(block.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in block.named_modules()] == [n for n, _ in plain.named_modules()]
    with pytest.raises(ValueError):
        modules.ResnetBlock(in_channels=64, dropout=1.5, temb_channels=0)
    with pytest.raises(ValueError):
        modules.ResnetBlock(in_channels=64, dropout=-0.1, temb_channels=0)
    dec = modules.Decoder(double_z=True, z_channels=16, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2, 4],
                          num_res_blocks=2, attn_resolutions=[16], dropout=0.2)
    assert all(m.dropout.p == 0.2 for m in dec.modules() if isinstance(m, modules.ResnetBlock))


def test_op_layer_validates_p_and_seed():
    from odvae_amd import ops
    assert ops._gn_drop(0.0, None) is None
    assert ops._gn_drop(0.25, 3) == (0.25, 3)
    assert ops._gn_drop(0.25, -1) == (0.25, 0xFFFFFFFFFFFFFFFF)
    with pytest.raises(ValueError):
        ops._gn_drop(1.5, 3)
    with pytest.raises(ValueError):
        ops._gn_drop(0.5, None)
