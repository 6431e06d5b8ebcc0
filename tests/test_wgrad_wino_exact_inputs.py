"""Host-only companion of tests/test_wgrad_wino_exact_gpu.py: tests/wgrad_wino_exact_inputs.py does what it is for.  The mirror of plan()
reproduces the plans the shapes were chosen for, the dense recipe keeps its conditions, the float64 model of the f32 loop equals the float64
gradient exactly on every shape, and the same comparison rejects each planted fault on the shapes named to guard against it."""
import pytest
import torch

import wgrad_wino_exact_inputs as E
import wgrad_wino_math as wm

F32_SHAPES = list(E.F32_CASES)
SPLIT_SHAPES = list(E.SPLIT_CASES)


@pytest.mark.parametrize("shape", F32_SHAPES + SPLIT_SHAPES, ids=E.case_id)
def test_mirror_reproduces_the_plan_of_the_tables(shape):
    want = E.F32_CASES.get(shape) or E.SPLIT_CASES[shape]
    assert E.table_row(shape) == want
    p = E.plan(*shape)
    n, cin, cout, h, w = shape
    assert E.supported(n, h, w, cin, cout) == 1
    assert p.chunks == -(-p.tiles // 16) and (p.nsplit - 1) * p.chunks_per_split + p.last_split == p.chunks and 1 <= p.last_split <= p.chunks_per_split
    assert E.nsplit_from_workspace(p.workspace_bytes, cin, cout) == p.nsplit
    assert p.wide == (w // 2 >= 16) and p.xcd_map == (p.nsplit % 8 == 0)
    if shape in E.SPLIT_CASES:
        assert p.split_eligible
    if shape in E.F32_CASES and shape not in E.SPLIT_CASES:
        assert not p.split_eligible, "selector 1 would still run the f32 loop here: nothing is forced"


def test_the_tables_hold_the_plans_they_are_there_for():
    rows = {s: E.plan(*s) for s in F32_SHAPES}
    assert {p.nsplit for p in rows.values()} >= {1, 2, 3, 4, 5, 8, 9, 33, 64}, "reduction wavefronts with no slab, one, two, sixteen"
    assert {p.chunks_per_split for p in rows.values()} >= {1, 2, 3, 4}
    assert any(p.xcd_map and p.nsplit > 32 for p in rows.values()) and any(p.xcd_map and not p.wide for p in rows.values())
    assert any(p.last_split < p.chunks_per_split for p in rows.values()), "a short last split"
    assert any(p.tiles % 16 and not p.wide for p in rows.values()) and any(p.tiles % 16 and p.wide for p in rows.values()), "ragged ends"
    assert any(p.wide and p.TX % 16 and p.chunks_per_split > 1 for p in rows.values()), "the wide walk's advance is consumed off whole chunks"
    srows = {s: E.plan(*s) for s in SPLIT_SHAPES}
    assert {p.nsplit for p in srows.values()} >= {1, 8, 16} and {p.chunks_per_split for p in srows.values()} >= {1, 2, 3, 4}
    assert any(p.last_split < p.chunks_per_split for p in srows.values())
    assert all(E.plan(*s).nsplit >= 2 for _, s in E.NAN_CASES)
    assert all((s in E.SPLIT_CASES) if form else (s in E.F32_CASES or s in E.SPLIT_CASES) for form, s in E.NAN_CASES)


def test_limits_of_the_mirror():
    assert E.supported(2, 2048, 2048, 128, 128) == 0 and E.supported(1, 2, 4194302, 128, 128) == 1      # 2^23 pixels x 512 bytes = 2^32
    assert E.supported(1, 2, 1398102, 384, 128) == 0 and E.supported(1, 2, 1398100, 384, 128) == 1
    assert E.workspace_bytes(2, 128, 128, 2048, 2048) == 0
    p = E.plan(1, 128, 128, 2, 4194302)
    assert (p.tiles, p.chunks, p.chunks_per_split, p.nsplit) == (2097151, 131072, 2048, 64)


@pytest.mark.parametrize("shape", F32_SHAPES, ids=E.case_id)
def test_dense_recipe_and_unfaulted_model(shape):
    x, dy, dw64, db64, sbar = E.dense_case(shape)
    assert torch.equal(x, x.round()) and x.abs().max() <= 3 and torch.equal(dy, dy.round()) and dy.abs().max() <= 2
    assert (x != 0).double().mean() > 0.8 and (dy != 0).double().mean() > 0.7, "dense: every pixel is drawn"
    assert sbar < 2.0 ** 21 and torch.equal(dw64.float().double(), dw64) and torch.equal(db64.float().double(), db64)
    dw, db = E.model(x, dy)
    assert torch.equal(dw, dw64) and torch.equal(db, db64)


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=E.case_id)
def test_dense_recipe_on_the_split_shapes(shape):
    x, dy, dw64, db64, sbar = E.dense_case(shape)
    assert sbar < 2.0 ** 21
    dw, db = E.model(x, dy)
    assert torch.equal(dw, dw64) and torch.equal(db, db64)


@pytest.mark.parametrize("recipe", E.RECIPES)
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=E.case_id)
def test_sparse_recipes_keep_their_conditions_on_the_split_shapes(shape, recipe):
    x, dy, dw64, db64 = E.sparse_case(recipe, shape)      # make_exact asserts the recipe's conditions
    v, m = wm.domain(x, dy)
    assert torch.equal(wm.to_weights(wm.split_sum(v, m)).float().double(), dw64), "the six kept products are the float64 gradient"


FAULT_CASES = [(f, s) for f in E.FAULTS for s in E.GUARDS[f]]


def test_every_fault_has_a_guard_among_the_cases():
    assert set(E.GUARDS) == set(E.FAULTS) and len(E.FAULTS) >= 10
    assert all(s in E.F32_CASES for f in E.FAULTS for s in E.GUARDS[f]) and all(E.GUARDS[f] for f in E.FAULTS)


@pytest.mark.parametrize("fault,shape", FAULT_CASES, ids=["%s-%s" % (f, E.case_id(s)) for f, s in FAULT_CASES])
def test_planted_fault_is_rejected_by_its_guard(fault, shape):
    x, dy, dw64, db64, _ = E.dense_case(shape)
    dw, db = E.model(x, dy, fault=fault)
    if fault in ("dbias_misses_last_split", "past_end_taken"):
        assert torch.equal(dw, dw64) and not torch.equal(db, db64)
    else:
        assert not torch.equal(dw, dw64), "%s went unnoticed" % fault
    if fault in ("reduce_skips_3_mod_4", "reduce_starts_at_k_plus_4", "no_left_mask", "no_right_mask", "no_top_mask", "no_bottom_mask", "stale_stage"):
        assert torch.equal(db, db64), "this fault does not reach dbias"


def test_wide_walk_faults_hide_at_one_chunk_per_split():
    """why the tables hold wide shapes of several chunks per split: at one chunk per split the division at the start places every tile"""
    for shape in ((1, 128, 128, 4, 34), (1, 128, 128, 2, 62), (3, 128, 128, 2, 48)):
        x, dy, dw64, _, _ = E.dense_case(shape)
        for fault in ("wide_wrap_on_equal", "tty_not_reset"):
            assert torch.equal(E.model(x, dy, fault=fault)[0], dw64)
