"""tests/vq_inputs.py held to account on the host: the acceptance rule for indices admits torch's f32 evaluation of upstream's own
expression and rejects planted faults; the float64 closed forms reject theirs.  No GPU."""
import numpy as np
import pytest
import torch

import vq_inputs as V

# (D, K, M, uniform): the shapes the rule was checked at, with fewer rows
RULE_SHAPES = [(3, 8192, 512, False), (4, 16384, 256, False), (8, 16384, 256, False), (64, 300, 777, False), (256, 1024, 256, False),
               (4, 64, 128, True)]


def torch_f32_indices(z, E):
    zt, Et = torch.tensor(z), torch.tensor(E)
    d = (zt ** 2).sum(1, keepdim=True) + (Et ** 2).sum(1) - 2 * zt @ Et.t()
    return d.argmin(1).numpy()


@pytest.mark.parametrize("d,k,m,uniform", RULE_SHAPES, ids=lambda v: str(v))
def test_rule_admits_torch_f32(d, k, m, uniform):
    z, E = V.gaussian_case(m, d, k, seed=23, uniform=uniform)
    idx = torch_f32_indices(z, E)
    bad, undecided = V.index_violations(z, E, idx)
    print("D=%d K=%d M=%d: violations %d, mismatches %d, undecided share %.4f" % (d, k, m, len(bad), (idx != V.assign_f64(z, E)).sum(), undecided))
    assert len(bad) == 0
    assert undecided < 0.05
    assert len(V.index_violations(z, E, V.assign_f64(z, E))[0]) == 0


def test_rule_rejects_out_of_range_and_far_codes():
    z, E = V.gaussian_case(64, 4, 100, seed=1)
    idx = V.assign_f64(z, E)
    wrong = idx.copy(); wrong[5] = 100
    assert list(V.index_violations(z, E, wrong)[0]) == [5]
    wrong = idx.copy(); wrong[7] = -1
    assert list(V.index_violations(z, E, wrong)[0]) == [7]
    s = V.scores_f64(z, E)
    wrong = idx.copy(); wrong[9] = int(np.argsort(s[9])[50])
    assert list(V.index_violations(z, E, wrong)[0]) == [9]


def test_assign_rule_ties_nan_inf():
    z, E = V.exact_case(8, 3, 10, seed=2)
    E[7] = E[2]                       # duplicate rows: the lowest index wins
    z[0] = E[2]
    V.plant_winner(z, E, 0, 2, dup=7)
    idx = V.assign_f64(z, E)
    assert idx[0] == 2
    assert V.assign_f64(z, E, fault="tie_highest")[0] == 7
    z[3, 1] = np.nan
    z[4, 0] = np.inf
    idx = V.assign_f64(z, E)
    assert idx[3] == 0 and 0 <= idx[4] < 10


@pytest.mark.parametrize("fault", ["no_norm", "skip_last", "skip_chunk_edge"])
def test_rule_rejects_index_faults(fault):
    m, d, k = 96, 4, 3 * V.CHUNK
    z, E = V.gaussian_case(m, d, k, seed=4)
    E = E * np.linspace(0.5, 2.0, k, dtype=np.float32)[:, None]       # norms that differ: dropping |e|^2 changes winners
    target = {"skip_last": k - 1, "skip_chunk_edge": V.CHUNK}.get(fault)
    if target is not None:
        z[:8] = E[target] + 1e-3 * z[:8]                               # rows whose clear winner is the code the fault never visits
    good = V.assign_f64(z, E)
    bad_idx = V.assign_f64(z, E, fault=fault)
    assert len(V.index_violations(z, E, good)[0]) == 0
    assert len(V.index_violations(z, E, bad_idx)[0]) >= (8 if target is not None else 1)


def test_tie_fault_is_caught_by_the_exact_comparison():
    z, E = V.exact_case(32, 4, 2 * V.CHUNK + 3, seed=6)
    V.plant_winner(z, E, 0, 5, dup=9)                     # duplicates inside one chunk
    V.plant_winner(z, E, 1, V.CHUNK - 1, dup=V.CHUNK)     # and across a chunk boundary
    good, bad = V.assign_f64(z, E), V.assign_f64(z, E, fault="tie_highest")
    assert good[0] == 5 and good[1] == V.CHUNK - 1 and bad[0] == 9 and bad[1] == V.CHUNK
    assert len(V.index_violations(z, E, bad)[0]) == 0      # same score: only the bit-for-bit comparison of the exact test sees it


@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("fault", ["beta_wrong_term", "dE_no_2", "dE_with_gq", "dz_no_st"])
def test_gradient_faults_leave_the_bounds(fault, legacy):
    m, d, k, beta = 128, 4, 16, 0.25
    z, E = V.gaussian_case(m, d, k, seed=8)
    idx = V.assign_f64(z, E)
    rng = np.random.RandomState(9)
    gq = rng.standard_normal((m, d)).astype(np.float32)
    dz, dE = V.backward_f64(z, E, idx, gq, 1.5, beta, legacy)
    fz, fE = V.backward_f64(z, E, idx, gq, 1.5, beta, legacy, fault=fault)
    tol_z = 3 * V.U * (np.abs(gq) + np.abs(dz - gq))                       # three f32 roundings on dz
    tol_E = 1.5 * (2.0 * max(beta, 1.0) / (m * d)) * V.dE_bound(z, E, idx)  # gamma_{c+3} sum |terms|, scaled
    moved_z = (np.abs(fz - dz) > tol_z).any()
    moved_E = (np.abs(fE - dE) > tol_E).any()
    assert moved_z or moved_E
    if fault in ("dE_no_2", "dE_with_gq"):
        assert moved_E
    if fault == "dz_no_st":
        assert moved_z
    # and the references themselves sit inside their own bounds
    assert not (np.abs(dz - dz) > tol_z).any()


def test_loss_fault_leaves_the_bound():
    z, E = V.gaussian_case(64, 4, 16, seed=10)
    idx = V.assign_f64(z, E)
    _, loss = V.quantize_f64(z, E, idx, 0.25)
    _, wrong = V.quantize_f64(z, E, idx, 0.25, fault="loss_div_M")
    assert abs(wrong - loss) > 4 * V.U * abs(loss) and abs(wrong / loss - 4.0) < 1e-12


def test_exact_case_is_exactly_summable():
    for d in (1, 3, 17, 256):
        z, E = V.exact_case(33, d, 70, seed=d)
        s64 = V.scores_f64(z, E)
        s32 = (E * E).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (z @ E.T)
        assert np.array_equal(s32.astype(np.float64), s64) and np.abs(s64).max() < 2 ** 24


def test_layout_helpers_round_trip():
    rows = np.arange(2 * 6 * 3, dtype=np.float32).reshape(12, 3)
    t = V.to_nchw(rows, 2, 6)
    assert t.shape == (2, 3, 6) and t[1, 2, 4] == rows[6 + 4, 2]
    assert np.array_equal(V.from_nchw(t), rows)


def test_usage_reference():
    counts, perplexity, used = V.usage_f64(np.array([0, 0, 3, 3]), 5)
    assert list(counts) == [2, 0, 0, 2, 0] and used == 2 and abs(perplexity - 2.0) < 1e-8
