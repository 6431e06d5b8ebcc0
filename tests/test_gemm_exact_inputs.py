"""Host-only checks of tests/gemm_exact_inputs.py: every recipe's summability assertion on the shapes the GPU tests use, the plane
assertions of the split recipes, the poisoned layout, the dispatch mirror's arithmetic, and the coverage meta-test: the case lists of
tests/test_gemm_f32_exact_gpu.py reach every instantiation gemm_f32.hip and gemm_f32_split.hip launch."""
import pytest
import torch

import gemm_exact_inputs as G


def test_case_list_reaches_every_instantiation():
    got = G.forms_reached()
    assert got == G.ALL_FORMS, (sorted(G.ALL_FORMS - got), sorted(got - G.ALL_FORMS))
    assert len(G.ALL_FORMS) == 4 * 3 + 1 + 4 + 1 + 4 + 2 + 2 + 2
    # the instantiations named in the issue, by the case meant to reach them
    assert ("reg_batched", "TN", "none") in G.gemm_forms("TN", 132, 132, 36, 3, 0)
    assert ("reg", "TN", "none") in G.gemm_forms("TN", 132, 132, 36, 1, 0)
    assert G.gemm_forms("TN", 132, 132, 36, 3, -1) == {("dma32", "TN", "none")}
    assert G.gemm_forms("NT", 132, 132, 36, 3, -1) == {("reg", "NT", "none")}
    assert G.smb_forms(132, 132, 68, 128, -1) == {("split", "NT", "smb")} and G.smb_forms(132, 132, 68, 128, 1) == {("dma32", "NT", "smb")}
    assert G.expb_forms(132, 132, 68, 128, -1) == {("split", "NT", "expb")} and G.expb_forms(132, 132, 36, 3, -1) == {("reg", "NT", "expb")}
    assert G.rownorm_forms(132, 132, 1024, 2, -1) == {("split", "NN", "rownorm")}
    assert G.rownorm_forms(132, 132, 1028, 2, -1) == {("reg", "NN", "rownorm")}
    assert G.rownorm_forms(132, 132, 1028, 128, -1) == {("split", "NN", "rownorm")}


def test_split_k_arithmetic_of_the_cases():
    """the split counts the cases were designed for, the partial last step, the pass-and-remainder of the reduce, the empty last split"""
    for layout, m, n, k, batch, splits in G.SPLITK_CASES:
        assert G.choose_splits(m, n, k, batch) == splits
        assert G.workspace_bytes(m, n, k, batch) == splits * batch * m * n * 4
        for st in G.STAGINGS:
            assert ("splitk_reduce",) in G.gemm_forms(layout, m, n, k, batch, st)
    assert G.k_per_split(1028, 2) == 544 and (1028 - 544) % 32 == 4 and (1027 - 544) % 32 == 3
    assert G.k_per_split(3000, 5) == 608 and 4 * 608 < 3000 and 5 % 4 == 1
    assert G.k_per_split(9220, 18) == 544 and 17 * 544 > 9220 > 16 * 544 and 18 % 4 == 2
    for layout, m, n, k, batch in G.PRED_CASES:
        assert G.workspace_bytes(m, n, k, batch) == 0
    assert G.tiles_of(132, 132) * 2 == 8 and G.tiles_of(132, 132) * 260 == 1040 > 1024


def test_split_gate_of_the_cases():
    """K = 1024 opens the bf16-split form at any tile count; K = 1028 / 1051 need 512 (tile, batch) pairs"""
    for layout, m, n, k, batch, shared in G.SPLIT_CASES:
        forms = G.gemm_forms(layout, m, n, k, batch, -1)
        if k == 1024 or batch == 128:
            assert forms == {("split", layout, "none")}
        else:
            assert ("splitk_reduce",) in forms and G.choose_splits(m, n, k, batch) == 2
        assert not G.split_eligible(1, 0, m, n, k, batch)
        assert not G.split_eligible(-1, 0, m, n, k, batch, bias=True) and not G.split_eligible(-1, 1, m, n, k, batch)
    assert G.split_tt_eligible(-1, 132, 132, 68, 128) and not G.split_tt_eligible(-1, 132, 132, 68, 127)
    assert not G.split_tt_eligible(-1, 132, 132, 60, 128) and not G.split_tt_eligible(0, 132, 132, 68, 128)


def test_conv1x1_cases_reach_three_kernel_forms():
    f = {case: G.conv1x1_forms(*case) for case in G.CONV1X1_CASES}
    assert f[(3, 36, 20, 5, 7)] == {"forward": {("reg", "NT", "none")}, "dx": {("reg", "NN", "none")}, "dw": {("dma32", "TN", "none")}}
    assert f[(2, 32, 64, 24, 24)]["dw"] == {("dma32", "TN", "none"), ("splitk_reduce",)}      # 1152 pixels: two splits
    assert f[(1, 32, 64, 32, 32)]["dw"] == {("split", "TN", "none")}                          # exactly 1024: the bf16-split kernel
    assert f[(2, 128, 132, 16, 9)]["dx"] == {("reg", "NN", "none")}


UNSPLIT_SHAPES = sorted({(r, e) + tuple(c[3:]) for c in G.UNSPLIT_CASES for r, e in [(c[1], c[2])]})


@pytest.mark.parametrize("case", UNSPLIT_SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_recipes_a_and_b_are_exactly_summable(case):
    recipe, epi, m, n, k, batch = case
    c = G.make_case(recipe, m, n, k, batch, epi)
    s = G.assert_exactly_summable(c)
    assert (c["bias"] is not None) == (epi != "plain") and (c["res"] is not None) == (epi == "bias_res")
    assert torch.equal(G.reference(c).float().double(), G.reference(c))
    if recipe == "B":
        assert (c["a"].abs() % 2 == 1).all() and c["a"].abs().max().item() <= 511
        assert ((c["b"] * 128).abs() % 2 == 1).all() and (c["b"] * 128).abs().max().item() <= 255
        assert s["product"] <= 511 * 255 * 128


def test_recipe_b_worst_case_is_under_the_limit():
    assert 511 * 255 * 128 == 16679040 < G.LIMIT
    c = G.make_case("B", 4, 4, 128, 1, "bias_res")
    c["a"] = torch.full_like(c["a"], 511.0)
    c["b"] = torch.full_like(c["b"], 255.0 / 128)
    G.assert_exactly_summable(c)


def test_recipe_a_is_good_to_k_16384():
    c = G.make_case("A", 8, 8, 16384, 1, "alpha_bias")
    c["a"] = torch.full_like(c["a"], -8.0)
    c["b"] = torch.full_like(c["b"], 2.0)
    s = G.assert_exactly_summable(c)
    assert s["product"] == 64 * 16384 == 2 ** 20


@pytest.mark.parametrize("epi", G.EPILOGUES)
def test_split_k_cases_are_exactly_summable(epi):
    for k, batch in sorted({(c[3], c[4]) for c in G.SPLITK_CASES}):
        G.assert_exactly_summable(G.make_case("A", 128, 128, k, batch, epi))


@pytest.mark.parametrize("recipe", G.SPLIT_RECIPES)
def test_split_recipes_planes_and_summability(recipe):
    for layout, m, n, k, batch, shared in G.SPLIT_CASES:
        if batch > 2:
            batch = 3      # the same generator at a batch the host test can afford
        c = G.make_case(recipe, m, n, k, batch, shared_b=shared)
        G.assert_exactly_summable(c)
        if recipe != "A":
            pp = G.assert_planes(c)
            assert pp[("hi", "hi")] > 0
    if recipe == "S2":
        assert (c["b"] != 0).sum(1).max().item() <= 8 and (G.split3(c["a"])[1] != 0).any() and (G.split3(c["b"])[1] != 0).any()
    if recipe == "S3":
        assert (c["b"] != 0).sum(1).max().item() <= 32 and (G.split3(c["a"])[2] != 0).any()
    if recipe == "S3T":
        assert (c["a"] != 0).sum(2).max().item() <= 32 and (G.split3(c["b"])[2] != 0).any()


def test_assert_planes_rejects_a_live_dropped_product():
    c = G.make_case("S3", 8, 8, 64, 1)
    c["b"][0, 0, 0] = 257.0      # a mid plane on the other side: a_lo b_mid is dropped by the kernel
    c["a"][0, 0, 0] = 2.0 ** 17 + 2 ** 9 + 1
    with pytest.raises(AssertionError):
        G.assert_planes(c)


def test_summability_rejects_what_can_round():
    c = G.make_case("A", 4, 4, 16, 1)
    c["a"][0, 0, 0] = 0.5 ** 3 * 3      # not an integer
    with pytest.raises(AssertionError):
        G.assert_exactly_summable(c)
    c = G.make_case("B", 4, 4, 128, 1)
    c["a"] = c["a"] * 4                  # four times the worst case: past 2^24 units
    c["a"][:] = 2044.0
    c["b"][:] = 255.0 / 128
    with pytest.raises(AssertionError):
        G.assert_exactly_summable(c)


def test_row_vector_recipes():
    for m, n, k, batch in ((132, 132, 36, 3), (132, 132, 68, 2)):
        for scaled in (False, True):
            c = G.make_smb_case(m, n, k, batch, scaled)
            G.assert_smb_exact(c)
            assert (c["rowmul"] is not None) == scaled
        c = G.make_expb_case(m, n, k, batch)
        G.assert_expb_exact(c)
        assert all((c["cls"][132 - 4:] == v).any() for v in (0, 1, 2))
    for m, n, k, batch, shared in G.ROWNORM_CASES:
        c = G.make_rownorm_case(m, n, k, min(batch, 3), shared_b=shared)
        l = G.assert_rownorm_exact(c)
        assert torch.equal((1.0 / l).float().double(), 1.0 / l)
        ref = torch.matmul(c["a"], c["b"]) / l[:, :, None]
        assert torch.equal(ref.float().double(), ref)


def test_poisoned_layout():
    for layout in G.LAYOUTS:
        c = G.make_case("A", 8, 12, 4, 3)
        ea, ba, eb, bb = G.embed_operands(layout, c)
        ta, tb = G.LAYOUTS[layout]
        assert ea.ld % 4 == 0 and ea.stride % 4 == 0 and ea.ld > ea.cols and ea.stride > ea.rows * ea.ld
        assert (ea.rows, ea.cols) == ((4, 8) if ta else (8, 4)) and (eb.rows, eb.cols) == ((12, 4) if tb else (4, 12))
        for e, buf, logical, t in ((ea, ba, c["a"], ta), (eb, bb, c["b"], tb)):
            assert torch.isnan(buf[~e.mask()]).all() and int(e.mask().sum()) == logical.numel()
            assert torch.equal(buf[e.index].double(), G.stored(t, logical))
            assert int(e.index.max()) + 2 * e.ld < e.numel + e.ld and torch.isnan(buf[:G.LEAD]).all() and torch.isnan(buf[-e.ld:]).all()
            assert e.index[1, 0, 0] - e.index[0, 0, 0] == e.stride and e.index[0, 1, 0] - e.index[0, 0, 0] == e.ld
    c = G.make_case("A", 8, 12, 4, 3, shared_b=True)
    _, _, eb, bb = G.embed_operands("NN", c)
    assert eb.stride == 0 and tuple(eb.index.shape) == (1, 4, 12)
