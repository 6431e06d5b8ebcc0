"""The bf16-split form of the direct 3x3 weight-gradient kernels (csrc/conv3x3_wgrad_f32.hip, odvae_conv3x3_wgrad_select(1)) through the C
ABI, against the f32 form of the same library (select(0)) and the float64 gradient on the CPU.

Exact cases: operands are whole numbers +-1 ... +-7 with sum |x| |dy| < 2^24 (tests/wgrad_direct_inputs.py), which bf16 holds in its hi
plane alone; every kept product and every partial sum is a whole number below 2^24, so dw and db must equal the float64 gradient bit for
bit, in any order of the k index.  tests/test_wgrad_direct_split_inputs.py asserts on the host that every case is admitted by the gate
and planned with the properties it is listed for.  Outputs are NaN-filled with canaries behind them, the workspace is exactly the asked
size, NaN-filled, with canary bytes behind it (the Launch of tests/test_wgrad_direct_exact_gpu.py).

Accuracy on random operands, the project's rule for a split product (tests/test_gemm_split_gpu.py, tests/test_wgrad_wino_split_gpu.py):
with e(form) = max |dw - dw64| and sbar = max over (co, ci, tap) of sum |x| |dy| (float64), e(split) <= e(f32) + 2^-22 sbar: the three
dropped products are below 2^-22 of sum |a| |b|, everything kept is accumulated in f32 as the f32 kernel does.  Each case prints its
figures before it asserts; profiles/wgrad_direct_split.md records them."""
import pytest
import torch

import wgrad_direct_inputs as W
import wgrad_direct_split_cases as C
from test_wgrad_direct_exact_gpu import Launch, mismatch

pytestmark = pytest.mark.gpu


def run(hip_lib, launch, form, bias=True):
    prev = hip_lib.odvae_conv3x3_wgrad_select(form)
    try:
        return launch.run(bias=bias)
    finally:
        hip_lib.odvae_conv3x3_wgrad_select(prev)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(C.CASES))
def test_exact_operands_give_the_float64_gradient_bit_for_bit(hip_lib, name):
    mode, n, cin, cout, hi, wi, _ = C.CASES[name]
    assert hip_lib.odvae_conv3x3_wgrad_split_supported(mode, n, hi, wi, cin, cout) == 1
    x, dy = W.make_exact(mode, n, cin, cout, hi, wi, W.case_seed(name))
    dw64, db64 = W.wgrad_f64(mode, x, dy)
    launch = Launch(hip_lib, mode, x, dy)
    dw, db = run(hip_lib, launch, 1)
    assert not torch.isnan(dw).any().item() and not torch.isnan(db).any().item(), "an output element was never written"
    assert torch.equal(dw.double(), dw64), "dw: " + mismatch(dw, dw64)
    assert torch.equal(db.double(), db64), "db: " + mismatch(db, db64)
    dw2, db2 = run(hip_lib, launch, 1)                     # a second launch: same bits
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dw3, db3 = run(hip_lib, launch, 1, bias=False)         # dbias = NULL: the same dw, and nothing else written
    assert torch.equal(dw3, dw), "dw without dbias: " + mismatch(dw3, dw64)
    assert torch.isnan(db3).all().item()
    dw0, db0 = run(hip_lib, launch, 0)                     # the f32 kernel is exact here too
    assert torch.equal(dw0, dw) and torch.equal(db0, db)


def random_case(kind, name):
    mode, n, cin, cout, hi, wi, _ = C.CASES[name]
    x, dy = W.make_normal(mode, n, cin, cout, hi, wi, W.case_seed(name) + len(kind))
    if kind == "mean3":
        x = x + 3.0
    elif kind == "x100":
        x = x * 100.0
    return mode, x, dy


_REFERENCE = {}


def reference(kind, name):
    """(mode, x, dy, dw64, db64, sbar) of one random operand set, computed once"""
    if (kind, name) not in _REFERENCE:
        mode, x, dy = random_case(kind, name)
        dw64, db64 = W.wgrad_f64(mode, x, dy)
        sbar = W.wgrad_f64(mode, x.abs(), dy.abs())[0].max().item()
        _REFERENCE[kind, name] = (mode, x, dy, dw64, db64, sbar)
    return _REFERENCE[kind, name]


@pytest.mark.parametrize("kind,mode", [("normal", 5), ("normal", 1), ("mean3", 5), ("mean3", 1), ("x100", 5), ("x100", 1)])
def test_split_form_is_as_close_to_float64_as_the_f32_form(hip_lib, kind, mode):
    name = C.ACCURACY_SHAPES[mode]
    mode, x, dy, dw64, db64, sbar = reference(kind, name)
    launch = Launch(hip_lib, mode, x, dy)
    d0, b0 = run(hip_lib, launch, 0)
    d1, b1 = run(hip_lib, launch, 1)
    e0 = (d0.double() - dw64).abs().max().item()
    e1 = (d1.double() - dw64).abs().max().item()
    print("%s %s: e(f32) %.3e e(split) %.3e sbar %.3e max|dw| %.3e  e(split)/sbar %.3e  bound - e(split) %.3e"
          % (kind, name, e0, e1, sbar, dw64.abs().max().item(), e1 / sbar, e0 + 2.0 ** -22 * sbar - e1))
    assert e1 <= e0 + 2.0 ** -22 * sbar
    assert bits_equal(b0, b1), "dbias is summed from the unsplit dy in the f32 kernel's order"
    assert not bits_equal(d0, d1), "selector 1 ran the f32 kernel"
    assert (b1.double() - db64).abs().max().item() <= 1e-5 * max(1.0, db64.abs().max().item())


@pytest.mark.parametrize("mode", [5, 1])
def test_the_default_follows_the_shape_rule(hip_lib, mode):
    """-1 gives the bits of one of the two forms; which one is the measured rule of profiles/wgrad_direct_split.md"""
    mode, x, dy, _, _, _ = reference("normal", C.ACCURACY_SHAPES[mode])
    launch = Launch(hip_lib, mode, x, dy)
    d0, b0 = run(hip_lib, launch, 0)
    d1, _ = run(hip_lib, launch, 1)
    dd, bd = run(hip_lib, launch, -1)
    assert bits_equal(dd, d0) or bits_equal(dd, d1)
    assert bits_equal(bd, b0)


@pytest.mark.parametrize("name", list(C.ADMITTED_BY_THE_RULE))
def test_the_shape_rule_admits_sixteen_tiles_per_block_of_full_channel_tiles(hip_lib, name):
    """the smallest shapes the default (-1) sends to the split form: its bits, not the f32 kernel's"""
    mode, n, cin, cout, hi, wi = C.ADMITTED_BY_THE_RULE[name]
    x, dy = W.make_normal(mode, n, cin, cout, hi, wi, W.case_seed(name))
    launch = Launch(hip_lib, mode, x, dy)
    d0, b0 = run(hip_lib, launch, 0)
    d1, b1 = run(hip_lib, launch, 1)
    dd, bd = run(hip_lib, launch, -1)
    assert not bits_equal(d0, d1)
    assert bits_equal(dd, d1), "the default ran the f32 kernel"
    assert bits_equal(bd, b0) and bits_equal(b1, b0)
    assert (d1 - d0).abs().max().item() <= 1e-4 * d0.abs().max().item()


@pytest.mark.parametrize("name", list(C.BELOW_THE_GATE))
def test_calls_below_the_gate_keep_the_f32_kernels_bit_for_bit(hip_lib, name):
    mode, n, cin, cout, hi, wi = C.BELOW_THE_GATE[name]
    assert hip_lib.odvae_conv3x3_wgrad_split_supported(mode, n, hi, wi, cin, cout) == 0
    x, dy = W.make_normal(mode, n, cin, cout, hi, wi, W.case_seed(name))
    launch = Launch(hip_lib, mode, x + 3.0, dy)
    d0, b0 = run(hip_lib, launch, 0)
    for form in (-1, 1):
        d, b = run(hip_lib, launch, form)
        assert bits_equal(d, d0) and bits_equal(b, b0), "form %d" % form
    dw64, _ = W.wgrad_f64(mode, x + 3.0, dy)
    assert (d0.double() - dw64).abs().max().item() <= 2e-4 * dw64.abs().max().item()


@pytest.mark.parametrize("mode", [5, 1])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_x_marks_its_channel_and_nothing_else(hip_lib, value, mode):
    mode, x, dy, _, _, _ = reference("normal", C.ACCURACY_SHAPES[mode])
    x = x.clone()
    ch = 37
    x[1, ch, 3, 17] = value      # an interior pixel: it meets all nine taps (mode 1: the four taps of odd row and column)
    launch = Launch(hip_lib, mode, x, dy)
    dw, db = run(hip_lib, launch, 1)
    bad = ~torch.isfinite(dw)
    want = torch.zeros_like(bad)
    if mode == 1:
        want[:, ch, 1::2, 1::2] = True      # input (3, 17) = (2 oy + kh, 2 ox + kw) only with kh = kw = 1
    else:
        want[:, ch] = True
    assert torch.equal(bad, want), "%d entries non-finite, %d expected" % (bad.sum().item(), want.sum().item())
    assert torch.isfinite(db).all()
