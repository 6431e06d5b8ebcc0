"""The pose head's dense layers (linear_f32.hip) bit for bit against float64, on exactly summable operands (tests/pose_head_inputs.py):
y, pre, dpre, dx and dw through the C ABI with act none and relu, with and without bias, at ragged and full tiles, reductions of 1 to
17 steps, every split boundary of the forward and the data gradient (fewer splits used than picked among them), the weight gradient
over batches of 1 to 67, and both epilogues past their 1024-block grid.  Outputs lie in NaN-filled buffers with canaries behind them;
the workspace is exactly what odvae_linear_workspace_bytes asks for.  tanh and swish: pre bit for bit, y and dpre within 4x the
distance of torch's own f32 from float64 on the same pre values (profiles/pose_head_exact.md)."""
import pytest
import torch

import pose_head_inputs as P
from canary_buffers import DEV, assert_canary, assert_workspace_canary, call, out_buf, workspace
from exact_inputs import assert_bits_equal

pytestmark = pytest.mark.gpu
ERR_WORKSPACE = 2       # ODVAE_ERR_WORKSPACE
ACT_ID = {"none": 0, "tanh": 1, "swish": 2, "relu": 3}


class Layer(object):
    """one forward + backward of a case through the C ABI, every output inside a canary-guarded buffer"""

    def __init__(self, L, c, act, dx=True, dw=True):
        from odvae_amd import lib
        m, n, k = c["m"], c["n"], c["k"]
        dev = lambda t: None if t is None else t.float().contiguous().to(DEV)
        x, w, b, dy = dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["dy"])
        need = L.odvae_linear_workspace_bytes(m, n, k)
        assert need == P.workspace_bytes(m, n, k)
        ws = workspace(need)
        bufs = {name: out_buf(size) for name, size in (("y", m * n), ("pre", m * n), ("dpre", m * n), ("dx", m * k), ("dw", n * k))}
        v = {name: view for name, (_, view) in bufs.items()}
        a = ACT_ID[act]
        call(L.odvae_linear_fwd_f32, x.data_ptr(), w.data_ptr(), lib.ptr(b), m, n, k, a, v["y"].data_ptr(), v["pre"].data_ptr(),
             ws.data_ptr(), need)
        call(L.odvae_linear_bwd_f32, x.data_ptr(), w.data_ptr(), v["pre"].data_ptr(), dy.data_ptr(), m, n, k, a, v["dpre"].data_ptr(),
             v["dx"].data_ptr() if dx else None, v["dw"].data_ptr() if dw else None, ws.data_ptr(), need)
        torch.cuda.synchronize()
        assert_canary(*(buf for buf, _ in bufs.values()))
        assert_workspace_canary(ws)
        shapes = {"y": (m, n), "pre": (m, n), "dpre": (m, n), "dx": (m, k), "dw": (n, k)}
        self.out = {name: v[name].cpu().view(shapes[name]) for name in v}


@pytest.mark.parametrize("m,n,k", P.LINEAR_SHAPES)
def test_linear_is_float64_bit_for_bit(hip_lib, m, n, k):
    if (m, n, k) in P.SPLIT_INTENT:         # the case is at the boundary it is there for
        product, picked, lengths = P.SPLIT_INTENT[(m, n, k)]
        i, j, red = P.product_dims(product, m, n, k)
        assert P.pick_splits(i, j, red) == picked and P.split_lengths(i, j, red) == lengths
    for bias, act in ((True, "none"), (True, "relu"), (False, "none"), (False, "relu")):
        c = P.make_linear_case(m, n, k, bias=bias, zero_pre=True)
        P.assert_exactly_summable(c)
        P.assert_case_is_live(c)
        want = P.linear_references(c, act)
        if act == "relu" and n >= 2:
            assert (want["pre"] == 0).any()             # relu'(0) = 0 is in the case
        got = Layer(hip_lib, c, act).out
        for name in ("pre", "y", "dpre", "dx", "dw"):
            assert_bits_equal(got[name], want[name].float(), "%s, act %s, bias %s" % (name, act, bias))


@pytest.mark.parametrize("m,n,k,act,bias", [(33, 31, 9, "relu", True), (3, 5, 200, "none", False), (4, 129, 40, "relu", True)])
def test_autograd_route_is_the_same(hip_lib, m, n, k, act, bias):
    from odvae_amd import ops
    c = P.make_linear_case(m, n, k, bias=bias, zero_pre=True)
    P.assert_exactly_summable(c)
    want = P.linear_references(c, act)
    x, w = (c[name].float().to(DEV).requires_grad_() for name in ("x", "w"))
    b = c["b"].float().to(DEV).requires_grad_() if bias else None
    y = ops.linear_act(x, w, b, act)
    y.backward(c["dy"].float().to(DEV))
    assert_bits_equal(y.detach().cpu(), want["y"].float(), "y")
    assert_bits_equal(x.grad.cpu(), want["dx"].float(), "dx")
    assert_bits_equal(w.grad.cpu(), want["dw"].float(), "dw")
    if bias:
        assert_bits_equal(b.grad.cpu(), want["db"].float(), "db")


@pytest.mark.parametrize("m,n,k", [(33, 31, 9), (4, 129, 40)])
def test_null_dx_or_dw_leaves_the_other_output_alone(hip_lib, m, n, k):
    c = P.make_linear_case(m, n, k, zero_pre=True)
    both = Layer(hip_lib, c, "relu").out
    no_dx = Layer(hip_lib, c, "relu", dx=False).out
    no_dw = Layer(hip_lib, c, "relu", dw=False).out
    assert torch.isnan(no_dx["dx"]).all() and torch.isnan(no_dw["dw"]).all()        # a NULL output is not written: its buffer keeps the fill
    for name in ("y", "pre", "dpre", "dw"):
        assert_bits_equal(no_dx[name], both[name], name + " with dx = NULL", summed=False)
    for name in ("y", "pre", "dpre", "dx"):
        assert_bits_equal(no_dw[name], both[name], name + " with dw = NULL", summed=False)


@pytest.mark.parametrize("m,n,k", [(3, 5, 129), (4, 129, 40)])
def test_workspace_one_byte_short_is_refused_and_nothing_is_written(hip_lib, m, n, k):
    from odvae_amd import lib
    L = hip_lib
    c = P.make_linear_case(m, n, k)
    x, w, b, dy = (c[name].float().to(DEV) for name in ("x", "w", "b", "dy"))
    need = L.odvae_linear_workspace_bytes(m, n, k)
    assert need > 1
    ws = workspace(need)
    bufs = [out_buf(size) for size in (m * n, m * n, m * n, m * k, n * k)]
    y, pre, dpre, dx, dw = (view for _, view in bufs)
    pre_in = torch.zeros(m, n, device=DEV)
    assert L.odvae_linear_fwd_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), m, n, k, 3, y.data_ptr(), pre.data_ptr(), ws.data_ptr(), need - 1,
                                  lib.stream_ptr()) == ERR_WORKSPACE
    assert L.odvae_last_error()
    assert L.odvae_linear_bwd_f32(x.data_ptr(), w.data_ptr(), pre_in.data_ptr(), dy.data_ptr(), m, n, k, 3, dpre.data_ptr(), dx.data_ptr(),
                                  dw.data_ptr(), ws.data_ptr(), need - 1, lib.stream_ptr()) == ERR_WORKSPACE
    torch.cuda.synchronize()
    for buf, view in bufs:
        assert torch.isnan(view).all()
        assert_canary(buf)
    assert (ws == 0xA5).all().item()


@pytest.mark.parametrize("act", ["tanh", "swish"])
@pytest.mark.parametrize("m,n,k", P.ACT_SHAPES)
def test_tanh_and_swish_within_four_times_torch(hip_lib, m, n, k, act):
    c = P.make_act_case(m, n, k)
    P.assert_exactly_summable(c)
    pre64 = c["x"] @ c["w"].t() + c["b"]
    for v in P.PLANTED_PRE:
        assert (pre64 == v).any()
    got = Layer(hip_lib, c, act, dx=False, dw=False).out
    assert_bits_equal(got["pre"], pre64.float(), "pre")
    figures = P.act_error_figures(got["y"], got["dpre"], got["pre"], c["dy"].float(), act)
    bounds = P.act_bounds(act)
    print("linear_f32 %s (%d, %d, %d): %s" % (act, m, n, k, {key: float("%.4g" % f) for key, f in figures.items()}))
    assert torch.isfinite(got["y"]).all() and torch.isfinite(got["dpre"]).all()
    for key, f in figures.items():
        assert f <= bounds[key], "%s: %s is %.4g, bound %.4g (4 x torch's %.4g)" % (act, key, f, bounds[key], P.TORCH_ACT_FIGURES[act][key])
