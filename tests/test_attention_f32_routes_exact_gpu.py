"""The GEMM routes of f32 attention (ops._Attention with the folded and with the separate softmax, ops._AttentionRecompute) through
ops.attention_qkv, on the selector inputs of tests/attn_exact_inputs.py.  Scores of integer operands are exact and a selected probability
of the separate softmax is exp(0) / g, so o and dv agree bit for bit (families A, B, C at T = 2^n) and dq = dk = 0 of a selector do;
the folded softmax's E = exp(scale (s - bound)) is not 1 and its results are held per element to bounds counted in f32 roundings
(attn_exact_inputs' docstring, "f32 routes").  Every case asserts which route ran: _ATTN_LAST_FLAG keeps a sentinel on the separate
and recompute routes, is 0 on a "bound holds" case and 1 on a "bound underflows" one, whose fallback must equal the separate route bit
for bit in o.  The routes take T % 4 == 0 only (float4 rows of P); for the other T of the list they must refuse, not fall back.
tests/test_attn_f32_exact_inputs.py shows on the host which planted faults these rules reject; tests/test_ops_gpu.py keeps the Gaussian
tests.  Observed margins: profiles/attn_f32_exact.md."""
import pytest
import torch

import attn_exact_inputs as ax
import gemm_exact_inputs as gx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
RECOMPUTE_TS = tuple(t for t in ax.GEMM_TS if t % 4 == 0)      # the recompute route takes what the GEMM route takes


def run_op(ops, case):
    """forward and backward of ops.attention_qkv on channels-last [N, 3C, H, W]; everything back on the host as [n, t, c]"""
    n, t, c = case["n"], case["t"], case["c"]
    h = 4 if t % 4 == 0 else 1
    w = t // h

    def nchw(x):
        return x.float().to(DEV).reshape(n, h, w, -1).permute(0, 3, 1, 2)

    def ntc(x):
        return x.detach().permute(0, 2, 3, 1).reshape(n, t, -1).cpu().contiguous()

    qkv = nchw(torch.cat([case["q"], case["k"], case["v"]], 2)).requires_grad_(True)
    o = ops.attention_qkv(qkv)
    fn = type(o.grad_fn).__name__
    o.backward(nchw(case["do"]))
    torch.cuda.synchronize()
    g = ntc(qkv.grad)
    return {"o": ntc(o), "dq": g[:, :, :c].contiguous(), "dk": g[:, :, c:2 * c].contiguous(), "dv": g[:, :, 2 * c:].contiguous(), "dqkv": g, "fn": fn}


def settings(monkeypatch, ops, folded, fused_bwd=True, budget=1 << 40):
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", False)
    monkeypatch.setattr(ops, "ATTN_FOLDED_SOFTMAX", folded)
    monkeypatch.setattr(ops, "FUSED_SOFTMAX_BWD", fused_bwd)
    monkeypatch.setattr(ops, "ATTN_SCORE_BUDGET", budget)
    sentinel = object()
    monkeypatch.setattr(ops, "_ATTN_LAST_FLAG", sentinel)
    return sentinel


def show(route, kw, margins):
    print("MARGIN %s %s C=%d T=%d N=%d %s" % (route, kw["family"], kw["c"], kw["t"], kw["n"], " ".join("%s=%.3f" % kv for kv in sorted(margins.items()))))


def run_separate(monkeypatch, ops, case, fused_bwd=True):
    sentinel = settings(monkeypatch, ops, folded=False, fused_bwd=fused_bwd)
    got = run_op(ops, case)
    assert got["fn"] == "_AttentionBackward" and ops._ATTN_LAST_FLAG is sentinel, "the separate-softmax route did not run"
    return got


def run_folded(monkeypatch, ops, case, side):
    sentinel = settings(monkeypatch, ops, folded=True)
    got = run_op(ops, case)
    assert got["fn"] == "_AttentionBackward" and ops._ATTN_LAST_FLAG is not sentinel, "the folded-softmax route did not run"
    assert int(ops._ATTN_LAST_FLAG.item()) == (1 if side == "underflows" else 0), "flag on a bound-%s case" % side
    return got


def check_all_gemm_routes(monkeypatch, ops, kw):
    case = ax.make_case(**kw)
    ax.assert_preconditions(case, dtype=F32)
    show("separate", kw, ax.check_case_f32(case, run_separate(monkeypatch, ops, case), "separate"))
    show("separate_unfused", kw, ax.check_case_f32(case, run_separate(monkeypatch, ops, case, fused_bwd=False), "separate_unfused"))
    for fcase, side in ax.folded_variants(kw):
        ax.assert_preconditions(fcase, dtype=F32)
        got = run_folded(monkeypatch, ops, fcase, side)
        if side == "holds":
            show("folded", kw, ax.check_case_f32(fcase, got, "folded"))
            continue
        sep = run_separate(monkeypatch, ops, fcase)
        assert torch.equal(got["o"], sep["o"]), "the fallback is not the separate-softmax computation"
        err, ref = (got["dqkv"] - sep["dqkv"]).abs().max().item(), max(1.0, sep["dqkv"].abs().max().item())
        assert err <= 1e-6 * ref, "dqkv after the fallback vs the separate pass: max err %.3e > 1e-6 * %.3e" % (err, ref)
        show("fallback", kw, ax.check_case_f32(fcase, got, "separate"))


@pytest.mark.parametrize("c,t", ax.gemm_grid())
def test_gemm_routes_exact(hip_lib, monkeypatch, c, t):
    """Separate softmax (backward in the dP product's epilogue and as a row pass), folded softmax where the bound holds and where it
    underflows, every family of one (C, T), every element of o and dqkv.  T around the 128-wide GEMM tiles from both sides."""
    from odvae_amd import lib, ops
    if t % 4:
        case = ax.make_case("A", 1, t, c)
        for folded in (False, True):
            settings(monkeypatch, ops, folded=folded)
            with pytest.raises(lib.HipLibraryError):
                run_op(ops, case)
        torch.cuda.synchronize()
        return
    for kw in ax.gemm_cases_for(c, t):
        check_all_gemm_routes(monkeypatch, ops, kw)


@pytest.mark.parametrize("budget_images", [2, 1])
@pytest.mark.parametrize("c,t", [(c, t) for c in ax.GEMM_CS for t in RECOMPUTE_TS])
def test_recompute_route_exact(hip_lib, monkeypatch, c, t, budget_images):
    """N = 5 through a score buffer of 2 images and of 1: the last group is not full, the backward's group is halved to 1, and drow is
    read at a per-group offset.  Every family and every T the GEMM routes take.  Bit-equal to the separate-softmax route, and under the
    closed forms."""
    from odvae_amd import ops
    for kw in ax.recompute_cases_for(c, t):
        case = ax.make_case(**kw)
        ax.assert_preconditions(case, dtype=F32)
        sep = run_separate(monkeypatch, ops, case)
        sentinel = settings(monkeypatch, ops, folded=True, budget=budget_images * t * t * 4)
        got = run_op(ops, case)
        assert got["fn"] == "_AttentionRecomputeBackward" and ops._ATTN_LAST_FLAG is sentinel, "the recompute route did not run"
        assert torch.equal(got["o"], sep["o"]) and torch.equal(got["dqkv"], sep["dqkv"]), "recompute vs separate softmax"
        show("recompute", kw, ax.check_case_f32(case, got, "recompute"))


@pytest.mark.parametrize("staging", [-1, 1], ids=["bf16-split-tt", "f32-mfma"])
def test_split_tt_products_exact(hip_lib, monkeypatch, staging):
    """N = 57, T = 300, C = 64: 513 blocks of 128 x 128, so the two T x T products with tails (E of the folded forward, dS of the
    backward) run on the bf16-split kernels (gemm_tile::split_tt_eligible); a forced staging keeps them on the f32 MFMA kernel.  The
    same exact claims and bounds must hold on both."""
    from odvae_amd import ops
    n, t, c = (ax.SPLIT_TT[x] for x in "ntc")
    assert gx.split_tt_eligible(staging, t, t, c, n) == (staging == -1), "N, T, C no longer sit on the intended side of the gate"
    prev = hip_lib.odvae_gemm_select_staging(staging)
    try:
        for fam in ("A", "B"):
            kw = dict(family=fam, group=4, **ax.SPLIT_TT)
            case = ax.make_case(**kw)
            ax.assert_preconditions(case, dtype=F32)
            show("separate", kw, ax.check_case_f32(case, run_separate(monkeypatch, ops, case), "separate"))
            for fcase, side in ax.folded_variants(kw):
                got = run_folded(monkeypatch, ops, fcase, side)
                if side == "underflows":
                    sep = run_separate(monkeypatch, ops, fcase)
                    assert torch.equal(got["o"], sep["o"]), "the fallback is not the separate-softmax computation"
                    err, ref = (got["dqkv"] - sep["dqkv"]).abs().max().item(), max(1.0, sep["dqkv"].abs().max().item())
                    assert err <= 1e-6 * ref, "dqkv after the fallback vs the separate pass: max err %.3e > 1e-6 * %.3e" % (err, ref)
                show("folded" if side == "holds" else "fallback", kw, ax.check_case_f32(fcase, got, "folded" if side == "holds" else "separate"))
    finally:
        hip_lib.odvae_gemm_select_staging(prev)
