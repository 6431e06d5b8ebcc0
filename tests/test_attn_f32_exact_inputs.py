"""The f32 part of tests/attn_exact_inputs.py on the host (no GPU): float32 models of the four f32 attention routes must pass every
family's rule at the GPU tests' shapes, each planted fault must be rejected by the rules on at least one case of the GPU grids, and the
folded route's "bound holds" / "bound underflows" cases must land on their side of the 1e-30 threshold by host arithmetic alone.

model_fused_* follows csrc/flash_attn_f32.hip in what decides a bit: 32-key tiles, row indices clamped to T - 1 and masked with < T, the
scaled score rounded before the running maximum is taken off it (forward), alpha / l / 1 / l, and exp2(s sc - lse2) in the backward with
and without fma contraction.  model_gemm follows ops._Attention / _AttentionRecompute: the separate softmax exp((s - max) scale) / sum,
the folded one (row bound of the row's own image, E = exp2((s - bound) scale log2 e), l, the flag where l is no normal number >= 1e-30,
rinv, the predicated fallback), the backward with delta from rowdot(dO, o) or from sum_j P dP, and the recompute route's groups.
Neither is a bit-exact twin of the kernels (sums run in another order, exp2 / log2 of the host are other functions); the rules they
are held to are those a correct kernel meets regardless."""
import math

import pytest
import torch

import attn_exact_inputs as ax

F32 = torch.float32
NAN = float("nan")
FUSED_FAULTS = ("fwd_clamp_valid", "dq_clamp_valid", "dkv_clamp_valid", "last_query_masked", "lse2_next", "delta_next",
                "perm_one_operand", "no_dv_launch_512", "dk_scaled_twice")
GEMM_FAULTS = ("bound_image0", "rinv_neighbour", "flag_ignored", "fallback_keeps_rinv", "drow_offset_dropped")


def _f(x):
    return torch.tensor(x, dtype=F32)


def _scale32(c):
    return _f(ax.scale_of(c))


def _perm16(c):
    """channel 16 t + 4 g + e read as 16 t + 4 e + g: the score products' lane-group order applied to one operand only"""
    i = torch.arange(c)
    return 16 * (i // 16) + 4 * (i % 4) + (i % 16) // 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def model_fused_forward(case, fault=None):
    n, t, c = case["n"], case["t"], case["c"]
    sc = _scale32(c) * _f(ax.LOG2E)
    o = torch.full((n, t, c), NAN, dtype=F32)
    lse2 = torch.full((n, t), NAN, dtype=F32)
    for b in range(n):
        q, k, v = case["q"][b], case["k"][b], case["v"][b]
        ks = k[:, _perm16(c)] if fault == "perm_one_operand" else k
        m = torch.full((t,), -float("inf"), dtype=F32)
        l = torch.zeros(t, dtype=F32)
        acc = torch.zeros(t, c, dtype=F32)
        for kt in range(0, t, 32):
            raw = torch.arange(kt, kt + 32)
            idx = raw.clamp(max=t - 1)
            valid = raw < t
            if fault == "fwd_clamp_valid":
                valid = torch.ones_like(valid)
            s = (q @ ks[idx].T).float() * sc                         # exact integers, one rounding
            s[:, ~valid] = -float("inf")
            mn = torch.maximum(m, s.max(1).values)
            alpha = torch.exp2(m - mn)
            p = torch.exp2(s - mn[:, None])
            l = l * alpha + p.sum(1)
            acc = ((acc * alpha[:, None]).double() + p.double() @ v[idx]).float()
            m = mn
        o[b] = acc * (1.0 / l)[:, None]
        lse2[b] = m + torch.log2(l)
        if fault == "last_query_masked" and t % 64:
            o[b, t - 1], lse2[b, t - 1] = NAN, NAN
    return o, lse2


def model_fused_backward(case, o, lse2, fault=None, contract=True):
    n, t, c = case["n"], case["t"], case["c"]
    scale = _scale32(c)
    sc = scale * _f(ax.LOG2E)
    out = {name: torch.empty(n, t, c, dtype=F32) for name in ("dq", "dk", "dv")}
    dup = (-t) % 32                                                   # copies of row T - 1 in the ragged tile
    nxt = (torch.arange(t) + 1).clamp(max=t - 1)
    for b in range(n):
        q, k, v, do = case["q"][b], case["k"][b], case["v"][b], case["do"][b]
        perm = fault == "perm_one_operand"
        s = q @ (k[:, _perm16(c)] if perm else k).T
        dp = (do @ (v[:, _perm16(c)] if perm else v).T).float()
        delta = (do * o[b].double()).sum(1).float()

        def p_ds(lse, dl):
            if contract:
                x = (s * sc.double() - lse.double()[:, None]).float()        # fma(s, sc, -lse2): one rounding
            else:
                x = s.float() * sc - lse[:, None]
            p = torch.exp2(x)
            return p, p * (dp - dl[:, None])

        p, ds = p_ds(lse2[b], delta)
        dq = ds.double() @ k
        if fault == "dq_clamp_valid":
            dq = dq + dup * ds[:, t - 1, None].double() * k[t - 1][None]
        out["dq"][b] = dq.float() * scale
        if fault in ("lse2_next", "delta_next"):
            p, ds = p_ds(lse2[b][nxt] if fault == "lse2_next" else lse2[b], delta[nxt] if fault == "delta_next" else delta)
        dk, dv = ds.double().T @ q, p.double().T @ do
        if fault == "dkv_clamp_valid":
            dk = dk + dup * ds[t - 1, :, None].double() * q[t - 1][None]
            dv = dv + dup * p[t - 1, :, None].double() * do[t - 1][None]
        out["dk"][b] = dk.float() * scale * (scale if fault == "dk_scaled_twice" else 1.0)
        out["dv"][b] = dv.float()
        if fault == "no_dv_launch_512" and c == 512:
            out["dv"][b] = NAN
    return out


def model_fused(case, fault=None, contract=True):
    o, lse2 = model_fused_forward(case, fault)
    got = model_fused_backward(case, o, lse2, fault, contract)
    got.update(o=o, lse2=lse2)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# the GEMM routes
# ---------------------------------------------------------------------------------------------------------------------------------
def model_gemm(case, route, fault=None, group=2):
    """route: separate | separate_unfused | recompute | folded.  Returns o, dq, dk, dv, flag (folded: 1 if the fallback had to run) and
    ran ("folded" or "separate": which arithmetic produced the result)."""
    n, t, c = case["n"], case["t"], case["c"]
    scale = _scale32(c)
    s = [case["q"][b] @ case["k"][b].T for b in range(n)]                # exact

    def softmax(b):
        x = (s[b] - s[b].max(1, keepdim=True).values).float() * scale
        e = torch.exp(x)
        return e * (1.0 / e.sum(1))[:, None]

    def mm(a, b_):
        return (a.double() @ b_).float()

    flag, rinv = 0, None
    if route == "folded":
        a2 = scale * _f(1.44269504088896)
        nq = [case["q"][b].float().pow(2).sum(1).sqrt() for b in range(n)]
        mk = [case["k"][b].float().pow(2).sum(1).sqrt().max() * _f(ax.BOUND_GROW) for b in range(n)]
        p, rinv, o = [], [], []
        for b in range(n):
            src = 0 if fault == "bound_image0" else b
            bound = nq[src] * mk[src]
            e = torch.exp2((s[b] - bound.double()[:, None]).float() * a2)
            l = e.sum(1)
            if not bool(((l >= 1e-30) & (l < 3.0e38)).all()):
                flag = 1
            ri = 1.0 / l
            if fault == "rinv_neighbour":
                ri = ri[(torch.arange(t) + 1).clamp(max=t - 1)]
            p.append(e), rinv.append(ri), o.append(mm(e, case["v"][b]) * ri[:, None])
        if flag and fault != "flag_ignored":
            p = [softmax(b) for b in range(n)]
            o = [mm(p[b], case["v"][b]) for b in range(n)]
            if fault != "fallback_keeps_rinv":
                rinv = [torch.ones(t, dtype=F32) for _ in range(n)]
    else:
        p = [softmax(b) for b in range(n)]
        o = [mm(p[b], case["v"][b]) for b in range(n)]
    got = {name: torch.empty(n, t, c, dtype=F32) for name in ("dq", "dk", "dv")}
    got["o"] = torch.stack(o)
    bgroup = max(1, group // 2)
    for b in range(n):
        q, k, v, do = case["q"][b], case["k"][b], case["v"][b], case["do"][b]
        dp = (do @ v.T).float()
        src = b
        if route == "recompute" and fault == "drow_offset_dropped":
            src = b - (b // bgroup) * bgroup                                  # the group's rows read from the start of drow
        if route == "separate_unfused":
            d = (p[b] * dp).sum(1)
        else:
            d = (case["do"][src] * o[src].double()).sum(1).float()
        if rinv is not None:
            got["dv"][b] = mm(p[b].T, (do.float() * rinv[b][:, None]).double())
            ds = (dp - d[:, None]) * (scale * rinv[b])[:, None] * p[b]
        else:
            got["dv"][b] = mm(p[b].T, do)
            ds = (dp - d[:, None]) * scale * p[b]
        got["dq"][b], got["dk"][b] = mm(ds, k), mm(ds.T, q)
    got["flag"] = flag
    got["ran"] = "folded" if route == "folded" and not (flag and fault != "flag_ignored") else "separate"
    return got


def check_gemm(case, got, route, side=None):
    """the rules of one GEMM-route result, as tests/test_attention_f32_routes_exact_gpu.py applies them: the flag the case's side
    demands, then the closed forms -- of the folded arithmetic where the bound held, of the separate softmax where the fallback ran"""
    if route == "folded":
        assert got["flag"] == (1 if side == "underflows" else 0), "flag %d on a bound-%s case" % (got["flag"], side)
        return ax.check_case_f32(case, got, "folded" if side == "holds" else "separate")
    return ax.check_case_f32(case, got, route)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the fault-free models stay within every rule at the GPU tests' shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ax.CS)
def test_fused_model_passes_every_family(c):
    worst = {}
    for cc, t in ax.grid_f32():
        if cc != c:
            continue
        for kw in ax.cases_for_f32(c, t):
            case = ax.make_case(**kw)
            ax.assert_preconditions(case, dtype=F32)
            for contract in ((True,) if t > 300 else (True, False)):
                for name, val in ax.check_case_f32(case, model_fused(case, contract=contract), "fused").items():
                    worst[(kw["family"], name)] = max(worst.get((kw["family"], name), 0.0), val)
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("c", ax.GEMM_CS)
def test_gemm_models_pass_every_family(c):
    worst = {}
    for t in ax.GEMM_TS:
        for kw in ax.gemm_cases_for(c, t):
            case = ax.make_case(**kw)
            ax.assert_preconditions(case, dtype=F32)
            runs = [(case, route, None) for route in ("separate", "separate_unfused")]
            runs += [(fc, "folded", side) for fc, side in ax.folded_variants(kw)]
            for cs, route, side in runs:
                for name, val in check_gemm(cs, model_gemm(cs, route), route, side).items():
                    worst[(route, kw["family"], name)] = max(worst.get((route, kw["family"], name), 0.0), val)
    assert worst and max(worst.values()) <= 1.0


def test_recompute_and_split_cases_pass():
    for kw in ax.recompute_cases_for(64, 132) + [dict(family="A", **ax.SPLIT_TT)]:
        case = ax.make_case(**kw)
        ax.assert_preconditions(case, dtype=F32)
        ax.check_case_f32(case, model_gemm(case, "recompute", group=2), "recompute")


def test_f32_recipe_leaves_the_bf16_cases_alone():
    """decoy=None is the recipe as it was; an amplitude scales the decoy columns only and moves no score"""
    a, b = ax.make_case("B", 3, 97, 64, group=4), ax.make_case("B", 3, 97, 64, group=4, decoy=(0.25, 4.0, 4.0))
    assert torch.equal(a["v"], b["v"]) and torch.equal(a["do"], b["do"]) and torch.equal(a["qcode"], b["qcode"])
    assert torch.equal(a["q"] @ a["k"].transpose(1, 2), b["q"] @ b["k"].transpose(1, 2))
    assert torch.equal(b["q"][0], a["q"][0] * torch.where(a["q"][0].abs() == ax.A_CODE, 1.0, 0.25)) and not torch.equal(a["q"][1], b["q"][1])
    assert ax.pack_qkv(a).dtype == torch.bfloat16 and ax.pack_qkv(a, F32).dtype == F32
    assert torch.equal(ax.pack_qkv(a, F32).double(), torch.cat([a["q"], a["k"], a["v"]], 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) every planted fault is rejected on at least one case of the GPU grids
# ---------------------------------------------------------------------------------------------------------------------------------
def _fused_fault_cases():
    kws = ax.cases_for_f32(64, 33) + ax.cases_for_f32(128, 129) + ax.cases_for_f32(512, 97)
    return [ax.make_case(**kw) for kw in kws]


@pytest.fixture(scope="module")
def fused_fault_cases():
    cases = _fused_fault_cases()
    for case in cases:
        ax.check_case_f32(case, model_fused(case), "fused")      # fault-free: accepted
    return cases


def _rejecting(cases, run):
    fams = set()
    for case in cases:
        try:
            run(case)
        except AssertionError:
            fams.add(case["family"])
    return fams


@pytest.mark.parametrize("contract", [True, False], ids=["fma", "mul-sub"])
@pytest.mark.parametrize("fault", FUSED_FAULTS)
def test_fused_fault_is_rejected(fused_fault_cases, fault, contract):
    fams = _rejecting(fused_fault_cases, lambda case: ax.check_case_f32(case, model_fused(case, fault, contract), "fused"))
    print("FAULT %s rejected by %s" % (fault, sorted(fams)))
    assert fams, "no family rejects the fused-route fault %r" % fault
    if fault in ("fwd_clamp_valid", "delta_next", "perm_one_operand"):
        assert "A" in fams        # the selector sees a duplicated key (lse2 moves by 1), a neighbour's delta, a mixed-up column
    if fault == "lse2_next":
        assert "A" not in fams and "B" in fams      # every row of a selector case has the same lse2; the tie groups of g and g / 2 do not


def _gemm_fault_cases():
    out = []
    for c, t in ((64, 132), (32, 260)):
        for kw in ax.gemm_cases_for(c, t):
            out += [(fc, "folded", side) for fc, side in ax.folded_variants(kw)]
    out += [(ax.make_case(**kw), "recompute", None) for kw in ax.recompute_cases_for(64, 132)]
    return out


@pytest.fixture(scope="module")
def gemm_fault_cases():
    cases = _gemm_fault_cases()
    for case, route, side in cases:
        check_gemm(case, model_gemm(case, route), route, side)
    return cases


@pytest.mark.parametrize("fault", GEMM_FAULTS)
def test_gemm_fault_is_rejected(gemm_fault_cases, fault):
    hit = set()
    for case, route, side in gemm_fault_cases:
        try:
            check_gemm(case, model_gemm(case, route, fault), route, side)
        except AssertionError:
            hit.add((case["family"], route, side))
    print("FAULT %s rejected by %s" % (fault, sorted(hit, key=str)))
    assert hit, "no case rejects the GEMM-route fault %r" % fault
    if fault == "bound_image0":
        assert all(side == "underflows" for _, _, side in hit)      # P = E / l does not see the bound: only the flag does
    if fault in ("flag_ignored", "fallback_keeps_rinv"):
        assert all(side == "underflows" for _, _, side in hit)
    if fault == "drow_offset_dropped":
        assert ("A", "recompute", None) in hit


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the folded route's threshold: every case used lands on its side by host arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ax.GEMM_CS)
def test_folded_cases_land_on_their_side(c):
    sides = {}
    for t in ax.GEMM_TS:
        for kw in ax.gemm_cases_for(c, t):
            for underflows in (False, True):
                case = ax.make_case(decoy=ax.folded_decoy(kw["n"], underflows), **kw)
                lo, hi = ax.folded_slack(case)[0].min().item(), ax.folded_slack(case)[0].max().item()
                side = ax.folded_side(case)
                if kw["family"] in ("A", "B"):
                    assert side == ("underflows" if underflows else "holds")
                    ax.assert_folded_precondition(case, underflows)
                    if underflows and kw["n"] > 1:      # image 0 holds: a bound taken from it would keep the flag down
                        assert ax.folded_slack(case)[0][0].max().item() <= ax.SLACK_HOLDS
                if kw["family"] == "C":
                    assert side == "holds" and hi == 0.0
                sides.setdefault((kw["family"], kw.get("level"), underflows), set()).add(side)
                assert lo >= -1e-9
    print("SIDES C=%d %s" % (c, sorted(sides.items(), key=str)))
    assert ax.SLACK_HOLDS < -math.log2(1e-30) < ax.SLACK_UNDERFLOWS - math.log2(max(ax.GEMM_TS))


def test_folded_precondition_rejects_the_wrong_side():
    kw = dict(family="A", n=3, t=132, c=64)
    with pytest.raises(AssertionError, match="more than 90"):
        ax.assert_folded_precondition(ax.make_case(decoy=ax.DECOY_UNDERFLOWS, **kw), False)
    with pytest.raises(AssertionError, match="no row"):
        ax.assert_folded_precondition(ax.make_case(decoy=ax.DECOY_HOLDS, **kw), True)


def test_f32_checkers():
    a = torch.tensor([1.0, -0.0, 3.0], dtype=F32)
    ax.assert_bits_equal_f32(a, torch.tensor([1.0, 0.0, 3.0], dtype=F32), "signed zero")
    with pytest.raises(AssertionError, match="differ in bits"):
        ax.assert_bits_equal_f32(a, torch.tensor([1.0, 0.0, 3.0 + 2.0 ** -22], dtype=F32), "one ulp")
    up = torch.nextafter(a, torch.full_like(a, 10.0))
    ax.assert_within_one_ulp_f32(up, a, "one step")
    with pytest.raises(AssertionError, match="more than one f32 ulp"):
        ax.assert_within_one_ulp_f32(torch.nextafter(up, torch.full_like(a, 10.0)), a, "two steps")
    assert ax.ulp32(1.0) == 2.0 ** -23 and ax.ulp32(1023.0) == 2.0 ** -14
