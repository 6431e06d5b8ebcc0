"""Host-only companion of tests/test_wgrad_wino_split_gpu.py: the exact recipes of tests/wgrad_wino_math.py do what they are for.  An
emulation of the split loop (three bf16 planes per operand, the six kept products) equals the float64 gradient on them bit for bit, and the
same comparison rejects a loop that drops any one of the six products, pairs two planes wrongly, or loses a tile or a channel of a chunk."""
import pytest
import torch

import wgrad_wino_math as wm

SHAPE = (2, 128, 128, 4, 32)      # N, Cin, Cout, H, W: 64 tiles = 4 chunks of 16, one tile row per chunk
RECIPES = ("x3", "dy3", "22")


def gradient(x, dy, **kw):
    v, m = wm.domain(x, dy)
    return wm.to_weights(wm.split_sum(v, m, **kw)).float()


@pytest.mark.parametrize("recipe", RECIPES)
def test_domain_form_is_the_convolution_weight_gradient(recipe):
    x, dy = wm.make_exact(recipe, *SHAPE, seed=3)
    v, m = wm.domain(x, dy)
    ref, _ = wm.wgrad_f64(x, dy)
    assert torch.equal(wm.to_weights(torch.einsum("xti,xto->xio", v, m)), ref)


@pytest.mark.parametrize("recipe", RECIPES)
def test_six_product_sum_is_exact_on_the_recipes(recipe):
    x, dy = wm.make_exact(recipe, *SHAPE, seed=3)
    ref, _ = wm.wgrad_f64(x, dy)
    assert torch.equal(ref.float().double(), ref), "the reference is an f32 number in every entry"
    assert torch.equal(gradient(x, dy), ref.float())


def test_every_kept_product_is_populated_by_some_recipe():
    assert set(sum((wm.populated(r) for r in RECIPES), ())) == set(wm.KEPT)


@pytest.mark.parametrize("recipe", RECIPES)
def test_a_dropped_product_is_rejected(recipe):
    x, dy = wm.make_exact(recipe, *SHAPE, seed=3)
    ref = wm.wgrad_f64(x, dy)[0].float()
    for gone in wm.populated(recipe):
        got = gradient(x, dy, pairs=tuple(pq for pq in wm.KEPT if pq != gone))
        assert not torch.equal(got, ref), "dropping %s went unnoticed on %s" % (gone, recipe)


def test_a_wrong_pairing_is_rejected():
    x, dy = wm.make_exact("x3", *SHAPE, seed=3)      # mid . lo in place of mid . hi
    ref = wm.wgrad_f64(x, dy)[0].float()
    wrong = tuple((wm.MID, wm.LO) if pq == (wm.MID, wm.HI) else pq for pq in wm.KEPT)
    assert not torch.equal(gradient(x, dy, pairs=wrong), ref)
    x, dy = wm.make_exact("dy3", *SHAPE, seed=3)     # lo . mid in place of hi . mid
    ref = wm.wgrad_f64(x, dy)[0].float()
    wrong = tuple((wm.LO, wm.MID) if pq == (wm.HI, wm.MID) else pq for pq in wm.KEPT)
    assert not torch.equal(gradient(x, dy, pairs=wrong), ref)


@pytest.mark.parametrize("recipe", RECIPES)
def test_a_lost_tile_or_channel_of_a_chunk_is_rejected(recipe):
    x, dy = wm.make_exact(recipe, *SHAPE, seed=3)
    ref = wm.wgrad_f64(x, dy)[0].float()
    v, m = wm.domain(x, dy)
    contrib = torch.einsum("xti,xto->ti", v.abs(), m.abs())      # what (tile, input channel) feeds into the result
    tile, ci = divmod(int(contrib.argmax()), contrib.shape[1])
    keep = torch.ones(1, v.shape[1], v.shape[2], dtype=torch.float64)
    keep[0, tile, :] = 0.0                                        # one tile of one chunk
    assert not torch.equal(gradient(x, dy, keep=keep), ref)
    keep = torch.ones(1, v.shape[1], v.shape[2], dtype=torch.float64)
    c0 = tile // wm.CHUNK * wm.CHUNK
    keep[0, c0:c0 + wm.CHUNK, ci] = 0.0                           # one channel of one chunk
    assert not torch.equal(gradient(x, dy, keep=keep), ref)
