"""tests/attn_exact_inputs.py on the host (no GPU): a model of the bf16 flash-attention kernels' arithmetic must pass every family's
acceptance rule at the GPU test's shapes, each planted fault must be rejected by at least one family, and the precondition asserts
must reject inputs that break them.

The model follows csrc/flash_attn_bf16.hip in what decides a bit: 32-key tiles, the reference point m moved for a whole wave (32
queries) when any of its rows exceeds it by more than 8, exp2 in f32 with results below 2^-126 flushed to 0, the f32 P summed into l and
the bf16 P multiplied with V, O (1 / l) rounded once; the backward rebuilds P from lse2 and forms dS from the f32 P (C = 64 / 512 and
the pair dQ kernel) or from the bf16 P (pair dK/dV kernel), with fmaf(dP, scale, -delta scale) in the pair kernels.  It is no
bit-exact twin of the kernels (exp2 / log2 of the host are other functions, sums run in another order); the assertions it is held to
are those a correct kernel meets regardless."""
import pytest
import torch

import attn_exact_inputs as ax

BF = torch.bfloat16
NEG_BIG = -1.0e30
FWD_FAULTS = ("no_tail_mask", "skip_last_tile", "stale_v", "key_off_by_one", "no_rescale", "k_chunks_swapped", "next_image_rows")
BWD_FAULTS = ("lse2_prev_tile", "delta_prev_tile", "drop_query_tile", "k_chunks_swapped")


def _exp2(x):
    y = torch.exp2(x.float())
    return torch.where(y < 2.0 ** -126, torch.zeros_like(y), y)


def _c32(c):
    return (torch.tensor(ax.scale_of(c), dtype=torch.float32) * torch.tensor(ax.LOG2E, dtype=torch.float32))


def _swap_chunks(k):
    k = k.clone()
    k[:, 0:8], k[:, 8:16] = k[:, 8:16].clone(), k[:, 0:8].clone()
    return k


def model_forward(case, fault=None):
    n, t, c = case["n"], case["t"], case["c"]
    c32 = _c32(c).double()
    nq = -(-t // 32) * 32
    ntiles = nq // 32
    o = torch.empty(n, t, c, dtype=BF)
    lse2 = torch.empty(n, t, dtype=torch.float32)
    for b in range(n):
        q = torch.zeros(nq, c, dtype=torch.float64)
        q[:t] = case["q"][b]
        k, v = torch.zeros(nq + 32, c, dtype=torch.float64), torch.zeros(nq + 32, c, dtype=torch.float64)    # rows past T read as zeros
        k[:t], v[:t] = case["k"][b], case["v"][b]
        if fault == "next_image_rows" and b + 1 < n:
            k[t:nq], v[t:nq] = case["k"][b + 1][: nq - t], case["v"][b + 1][: nq - t]
        m = torch.full((nq,), NEG_BIG, dtype=torch.float32)
        l = torch.zeros(nq, dtype=torch.float32)
        acc = torch.zeros(nq, c, dtype=torch.float32)
        for ti in range(ntiles - 1 if fault == "skip_last_tile" and ntiles > 1 else ntiles):
            k0 = 32 * ti
            kt = k[k0 + 1:k0 + 33] if fault == "key_off_by_one" else k[k0:k0 + 32]
            if fault == "k_chunks_swapped":
                kt = _swap_chunks(kt)
            vt = v[k0 - 32:k0] if fault == "stale_v" and ti >= 1 else v[k0:k0 + 32]
            s = (q @ kt.T).float()
            if fault not in ("no_tail_mask", "next_image_rows"):
                s[:, max(0, t - k0):] = NEG_BIG
            mx = s.max(1).values * c32.float()
            trig = (mx > m + 8.0).view(-1, 32).any(1).repeat_interleave(32)       # the ballot of a wave: its 32 queries
            m_new = torch.where(trig, torch.maximum(m, mx), m)
            alpha = _exp2(m - m_new)
            l = l * alpha
            if fault != "no_rescale":
                acc = acc * alpha[:, None]
            m = m_new
            p = _exp2((s.double() * c32 - m.double()[:, None]).float())
            l = l + p.sum(1)
            acc = (acc.double() + p.to(BF).double() @ vt).float()
        o[b] = (acc * (1.0 / l)[:, None]).to(BF)[:t]
        lse2[b] = (m + torch.log2(l))[:t]
    return o, lse2


def model_backward(case, o, lse2, fault=None):
    n, t, c = case["n"], case["t"], case["c"]
    pair = c in (128, 256)
    c32 = _c32(c).double()
    scale = torch.tensor(ax.scale_of(c), dtype=torch.float32)
    out = {name: torch.empty(n, t, c, dtype=BF) for name in ("dq", "dk", "dv")}

    def prev_tile(x):      # a row constant taken from the tile before (the first tile keeps its own)
        y = x.clone()
        y[32:] = x[:-32]
        return y

    for b in range(n):
        q, k, v, do = case["q"][b], case["k"][b], case["v"][b], case["do"][b]
        s = (q @ (_swap_chunks(k) if fault == "k_chunks_swapped" else k).T).float()
        dp = (do @ v.T).float()
        delta = (do * o[b].double()).sum(1).float()
        lse = lse2[b]

        def p_and_ds(lse_r, delta_r, bf16_p):
            p = _exp2((s.double() * c32 - lse_r.double()[:, None]).float())
            if pair:
                x = (dp.double() * scale.double() - (delta_r * scale).double()[:, None]).float()      # fmaf(dP, scale, -round(delta scale))
                ds = (p.to(BF).float() if bf16_p else p) * x
            else:
                ds = p * (dp - delta_r[:, None]) * scale
            return p.to(BF).double(), ds.to(BF).double()

        _, ds_q = p_and_ds(lse, delta, False)
        pb, ds_kv = p_and_ds(prev_tile(lse) if fault == "lse2_prev_tile" else lse, prev_tile(delta) if fault == "delta_prev_tile" else delta, True)
        if fault == "drop_query_tile":
            r0 = 32 if t > 32 else 0
            pb[r0:r0 + 32], ds_kv[r0:r0 + 32] = 0.0, 0.0
        out["dq"][b] = (ds_q @ k).float().to(BF)
        out["dk"][b] = (ds_kv.T @ q).float().to(BF)
        out["dv"][b] = (pb.T @ do).float().to(BF)
    return out


def model(case, fwd_fault=None, bwd_fault=None):
    o, lse2 = model_forward(case, fwd_fault)
    got = model_backward(case, o, lse2, bwd_fault)
    got.update(o=o, lse2=lse2)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the fault-free model stays within every rule at the GPU test's shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ax.CS)
def test_model_passes_every_family(c):
    worst = {}
    for cc, t in ax.grid():
        if cc != c:
            continue
        for kw in ax.cases_for(c, t):
            case = ax.make_case(**kw)
            ax.assert_preconditions(case)
            for name, val in ax.check_case(case, model(case)).items():
                worst[(kw["family"], name)] = max(worst.get((kw["family"], name), 0.0), val)
    assert worst and max(worst.values()) <= 1.0


def test_selector_closed_form_matches_dense():
    """family A's gather / scatter reference against the masked-softmax path the other families use"""
    for kw in (dict(family="A", n=2, t=45, c=64), dict(family="A", n=1, t=97, c=128, many_to_one=True)):
        case = ax.make_case(**kw)
        o_used = ax.rne(ax.references(case)["o"] + 1.0).double()      # a wrong o: delta off, dq and dk not zero
        a, d = ax.references(case, o_used, dense=False), ax.references(case, o_used, dense=True)
        for name in a:
            assert torch.allclose(a[name], d[name], rtol=1e-12, atol=1e-12), name      # float64 sums in another order
        assert a["dq"].abs().max() > 0 and a["dk"].abs().max() > 0


def test_recipes_are_what_they_claim():
    case = ax.make_case("A", 3, 97, 64)
    assert not torch.equal(case["v"][0], case["v"][1]) and not torch.equal(case["qcode"][0], case["qcode"][1])
    nz_q, nz_k = (case["q"] != 0).any(0).any(0), (case["k"] != 0).any(0).any(0)
    code = (case["k"].abs() == ax.A_CODE).all(0).all(0)
    assert not (nz_q & nz_k & ~code).any(), "q and k decoys share a column"
    assert code.view(-1, 16).any(1).all(), "a 16-column k-step carries no code column"
    m2o = ax.make_case("A", 1, 97, 64, many_to_one=True)
    assert len(set(m2o["qcode"][0].tolist())) <= 48
    b = ax.make_case("B", 1, 300, 64, group=8)
    for u in (0, 1):      # the members of a group lie in different 32-key tiles and 128-row blocks
        keys = (b["cid"] == u).nonzero()[:, 0]
        assert keys.numel() == (8 if u == 0 else 4) and len(set((keys // 32).tolist())) == keys.numel() and len(set((keys // 128).tolist())) > 1
    d = ax.make_case("D", 1, 300, 64, level=9, high_first=False)
    assert set(((d["cid"] < 2).nonzero()[:, 0][-2:] // 32).tolist()) == {9}


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) every planted fault is rejected by at least one family
# ---------------------------------------------------------------------------------------------------------------------------------
def _fault_cases():
    return [ax.make_case("A", 3, 97, 64), ax.make_case("A", 3, 300, 128, many_to_one=True), ax.make_case("B", 1, 160, 256, group=4),
            ax.make_case("C", 1, 45, 64), ax.make_case("C", 3, 97, 512), ax.make_case("D", 1, 160, 64, level=9, high_first=False),
            ax.make_case("D", 1, 257, 128, level=9, high_first=False)]


@pytest.fixture(scope="module")
def fault_cases():
    cases = _fault_cases()
    for case in cases:
        ax.assert_preconditions(case)
        ax.check_case(case, model(case))      # fault-free: accepted
    return cases


def _rejected_by(cases, **fault):
    fams = set()
    for case in cases:
        try:
            ax.check_case(case, model(case, **fault))
        except AssertionError:
            fams.add(case["family"])
    return fams


@pytest.mark.parametrize("fault", FWD_FAULTS)
def test_forward_fault_is_rejected(fault_cases, fault):
    fams = _rejected_by(fault_cases, fwd_fault=fault)
    assert fams, "no family rejects the forward fault %r" % fault
    if fault == "no_tail_mask":
        assert fams == {"C"}, "zero pad keys are invisible to a selecting softmax: only the uniform family counts them in l"
    if fault == "no_rescale":
        assert "D" in fams


@pytest.mark.parametrize("fault", BWD_FAULTS)
def test_backward_fault_is_rejected(fault_cases, fault):
    assert _rejected_by(fault_cases, bwd_fault=fault), "no family rejects the backward fault %r" % fault


def test_lagging_maximum_is_exercised():
    """family D at -6 with the level-0 key last: m stays at the low level (no rescale) and P reaches 2^6; at -9 it must move"""
    for level, moved in ((6, False), (9, True)):
        case = ax.make_case("D", 1, 160, 64, level=level, high_first=False)
        o, _ = model_forward(case)
        o_nr, _ = model_forward(case, "no_rescale")
        assert torch.equal(o, o_nr) != moved


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the preconditions reject what breaks them
# ---------------------------------------------------------------------------------------------------------------------------------
def test_preconditions_reject_violations():
    case = ax.make_case("A", 1, 97, 64)
    gap, top = ax.assert_preconditions(case)
    assert gap >= 160.0 and top < 2.0 ** 13
    weak = dict(case, q=case["q"] / 2, k=case["k"])                 # half the amplitude on q: the gap halves
    with pytest.raises(AssertionError, match=r"\(P1\)"):
        ax.assert_preconditions(weak)
    loud = dict(case, q=case["q"] * 8, k=case["k"] * 2)             # |s_sel c| x 16
    with pytest.raises(AssertionError, match=r"\(P2\)"):
        ax.assert_preconditions(loud)
    off = dict(case, v=case["v"] + 2.0 ** -10)
    with pytest.raises(AssertionError, match="bf16 numbers"):
        ax.assert_preconditions(off)
    wide = ax.make_case("D", 1, 160, 64, level=9)
    wide["k"] = torch.where((wide["k"] < 0) & (wide["k"].abs() > 16.0), wide["k"] * 2, wide["k"])     # the low level at -18
    with pytest.raises(AssertionError, match=r"\(P1\)"):
        ax.assert_preconditions(wide)


@pytest.mark.parametrize("c,r,gap", [(64, 2, 184.0), (128, 3, 195.0), (256, 4, 184.0), (512, 5, 163.0)])
def test_code_repeats(c, r, gap):
    assert ax.repeats_for(c) == r
    assert abs(2 * r * ax.A_CODE ** 2 * ax.c_of(c) - gap) < 1.0
    assert ax.assert_preconditions(ax.make_case("A", 1, 300, c))[0] >= 160.0
