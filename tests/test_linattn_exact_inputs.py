"""tests/linattn_exact_inputs.py on the host: the cases meet the condition and cover their edges, the closed form is float64's answer,
the host model of the kernels' index space reproduces it bit for bit, every planted fault is rejected by at least one case -- and the
faults that need several tiles, splits or images are rejected by none of the single-tile, single-split cases, which is what the cases
beyond them are for."""
import pytest
import torch

import linattn_exact_inputs as X

_CACHE = {}


def case_of(shape):
    if shape not in _CACHE:
        case = X.make_case(*shape)
        _CACHE[shape] = (case, X.closed_form(case))
    return _CACHE[shape]


@pytest.mark.parametrize("shape", X.CASES, ids=str)
def test_case_is_exactly_summable_and_covers_its_edges(shape):
    case, ref = case_of(shape)
    s = X.assert_exactly_summable(case, ref)
    print(shape, {k: "%.3g" % (v / X.LIMIT) for k, v in s.items()})
    X.assert_covers_edges(case)
    for name in X.NAMES + ("dctx", "g"):
        assert torch.equal(ref[name].float().double(), ref[name]), name + " is not made of f32 numbers"


@pytest.mark.parametrize("shape", X.CASES, ids=str)
def test_closed_form_is_float64(shape):
    """float64 autograd of the definition, rounded once to f32, is the closed form (float64 keeps exp(-128) = 2.6e-56, which no f32
    number sees: not next to a non-zero value, and alone it rounds to 0)"""
    case, ref = case_of(shape)
    r64 = X.float64_autograd(case)
    for name in X.NAMES:
        assert torch.equal(r64[name].float().double(), ref[name]), name


@pytest.mark.parametrize("shape", X.CASES, ids=str)
def test_host_model_is_the_closed_form(shape):
    case, ref = case_of(shape)
    got = X.host_model(case)
    assert X.differs(got, ref) == []
    for name in ("dctx", "g"):
        assert torch.equal(got[name].double(), ref[name]), name


def fault_matrix():
    return {f: [shape for shape in X.CASES if X.differs(X.host_model(case_of(shape)[0], f), case_of(shape)[1])] for f in X.FAULTS}


def test_every_fault_is_rejected_and_some_only_by_the_larger_cases():
    matrix = fault_matrix()
    for f, shapes in matrix.items():
        print("%-28s %s" % (f, " ".join("(%d,%d,%d)" % s for s in shapes)))
        assert shapes, "no case rejects " + f
    for f in X.NEEDS_SEVERAL:
        assert not set(matrix[f]) & set(X.SINGLE), "%s is rejected by a single-tile, single-split case" % f
    assert len(X.SINGLE) >= 6
