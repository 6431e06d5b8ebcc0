"""tests/pose_head_inputs.py held to what it mirrors.  Host only: the launch-rule mirror against odvae_linear_workspace_bytes (pure host
code of the library), the exact operands against their own precondition, the float64 pose reference against the float64 oracle with
autograd, and the acceptance rule from both sides -- it admits the oracle's own f32 evaluation on every case, and it rejects every
planted fault of the host model."""
import functools

import pytest
import torch

import pose_head_inputs as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


# ------------------------------------------------------------------------------------------------------------------------------
# dense layers
# ------------------------------------------------------------------------------------------------------------------------------
def test_launch_rule_mirror_matches_the_library(lib):
    L = lib.load()
    for m, n, k in P.LINEAR_SHAPES + P.ACT_SHAPES + [(32, 500, 500), (32, 27, 500), (1, 1024, 512), (32, 4096, 500), (513, 513, 513)]:
        assert L.odvae_linear_workspace_bytes(m, n, k) == P.workspace_bytes(m, n, k), (m, n, k)


def test_split_cases_hit_the_boundaries_they_are_named_for():
    for (m, n, k), (product, picked, lengths) in P.SPLIT_INTENT.items():
        i, j, red = P.product_dims(product, m, n, k)
        assert P.pick_splits(i, j, red) == picked and P.split_lengths(i, j, red) == lengths, (m, n, k)
    assert P.used_splits(2, 40, 4100) == 57 and P.pick_splits(2, 40, 4100) == 64            # fewer splits used than picked
    assert P.used_splits(5, 27, 500) == P.pick_splits(5, 27, 500) == 7
    for m, n, k in P.WGRAD_SHAPES:
        assert m in (1, 7, 8, 9, 67)                                                            # reduced over M in one split: 1 to 9 steps of 8
    assert {len(range(0, k, 8)) for _, _, k in P.TILE_SHAPES} >= {1, 2, 3}                      # 1 to 17 reduction elements
    (m1, n1, k1), (m2, n2, k2) = P.CAP_SHAPES
    assert m1 * n1 > P.EPILOGUE_CAP >= m1 * k1 and m2 * k2 > P.EPILOGUE_CAP >= m2 * n2          # forward / data-gradient epilogue wraps


@pytest.mark.parametrize("m,n,k", P.LINEAR_SHAPES)
def test_linear_cases_are_exactly_summable(m, n, k):
    for bias in (True, False):
        c = P.make_linear_case(m, n, k, bias=bias, zero_pre=True)
        P.assert_exactly_summable(c)
        P.assert_case_is_live(c)
        for act in ("none", "relu"):
            r = P.linear_references(c, act)
            for name, t in r.items():
                assert torch.equal(t.float().double(), t), name                                 # the float64 answers are f32 numbers
        if n >= 2:
            assert (P.linear_references(c, "relu")["pre"] == 0).any()
    c2 = P.make_linear_case(m, n, k, seed=1)
    if m * n * k > 64:
        assert not torch.equal(c2["x"], P.make_linear_case(m, n, k)["x"])


def test_summability_rejects_what_can_round():
    c = P.make_linear_case(5, 27, 500)
    c["x"] = c["x"] * 2.0 ** 14
    c["units"]["x"] = 2.0 ** -3
    with pytest.raises(AssertionError):
        P.assert_exactly_summable(c)
    c = P.make_linear_case(5, 27, 500)
    c["w"][0, 0] = 1.0 / 3.0
    with pytest.raises(AssertionError):
        P.assert_exactly_summable(c)


def test_a_lost_or_doubled_k_step_changes_the_answer():
    c = P.make_linear_case(3, 5, 129)
    want = P.linear_references(c)["pre"]
    for k in (0, 71, 72, 128):
        lost = want - c["x"][:, k:k + 1] @ c["w"][:, k:k + 1].t()
        assert not torch.equal(lost, want)


@pytest.mark.parametrize("act", ["tanh", "swish"])
def test_torch_activation_figures_are_the_recorded_ones(act):
    """torch's f32 forward and autograd backward on this host against float64, on the pre values the GPU test uses: the recorded
    figures (the kernel is held to 4x of them) are not below what is measured here"""
    worst, seen = {}, []
    fn = torch.tanh if act == "tanh" else torch.nn.functional.silu
    for m, n, k in P.ACT_SHAPES:
        c = P.make_act_case(m, n, k)
        P.assert_exactly_summable(c)
        pre64 = c["x"] @ c["w"].t() + c["b"]
        assert torch.equal(pre64.float().double(), pre64)
        for v in P.PLANTED_PRE:
            assert (pre64 == v).any()
        seen.append(pre64[(pre64.abs() <= 12)])
        pre = pre64.float().requires_grad_()
        y = fn(pre)
        dy = c["dy"].float()
        y.backward(dy)
        for key, f in P.act_error_figures(y.detach(), pre.grad, pre.detach(), dy, act).items():
            worst[key] = max(worst.get(key, 0.0), f)
    inside = torch.cat(seen).unique()
    assert inside.numel() >= 1000 and inside.min() < -11.5 and inside.max() > 11.5 and inside.diff().max() <= 0.5      # [-12, 12], finely
    print("torch f32 %s: %s" % (act, {k: float("%.4g" % v) for k, v in worst.items()}))
    rec = P.TORCH_ACT_FIGURES[act]
    assert set(rec) == set(worst)
    for key, f in worst.items():
        assert f <= rec[key] <= 1.25 * f, (key, f, rec[key])        # what is recorded is what this host measures, rounded up a little


def test_ulp_distance_never_admits_nan_or_a_spurious_non_zero():
    ref = torch.tensor([1.0, 0.0, 1e-40, 3.0], dtype=torch.float64)
    got = torch.tensor([1.0 + 2.0 ** -23, 1e-45, 0.0, float("nan")])
    d = P.ulp_distance(got, ref)
    assert d[0].item() == 1.0 and d[1].item() == float("inf") and d[3].item() == float("inf")
    assert 0 < d[2].item() < 2 ** 23


# ------------------------------------------------------------------------------------------------------------------------------
# pose terms
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_terms(c, dtype):
    """oracle.losses.PoseLoss.pose_terms (the code oracle forward() runs) with autograd, in `dtype`: out [9], d dec_pose, d moments"""
    import oracle.losses as OL
    from oracle.distributions import DiagonalGaussianDistribution as DG
    loss = object.__new__(OL.PoseLoss)
    torch.nn.Module.__init__(loss)
    loss.train_on_yaw = c["yaw"]
    loss.pose_loss = torch.nn.MSELoss(reduction="none") if c["l2"] else torch.nn.L1Loss(reduction="none")
    loss.rot_loss_fn = torch.nn.SmoothL1Loss(reduction="none")
    loss.bbox_loss_fn = torch.nn.MSELoss(reduction="none")
    loss.fill_factor_loss_fn = torch.nn.MSELoss(reduction="none")
    loss.bbox_distribution_dict = {}
    for l in range(c["L"]):
        mean, var, logvar = (c["prior"][l, i].to(dtype) for i in range(3))
        dist = DG(torch.stack([mean, logvar], 1))
        dist.var = var[:, None]           # the kernel is handed the table's variance; exp(logvar) rounds differently
        loss.bbox_distribution_dict["lab%d" % l] = dist
    labels = ["background" if i < 0 else "lab%d" % i for i in c["prior_idx"].tolist()]
    dp = c["dec_pose"].to(dtype).requires_grad_()
    mo = c["moments"].to(dtype).requires_grad_()
    mask_bg = (c["class_gt"] != c["bg_idx"]).long()
    saved, saved_dtype = OL.sigmoid_focal_loss_mean, torch.get_default_dtype()
    OL.sigmoid_focal_loss_mean = functools.partial(saved, gamma=c["gamma"], alpha=c["alpha"])
    torch.set_default_dtype(dtype)        # pose_terms gathers the per-sample KL in a torch.zeros of the default dtype
    try:
        t = loss.pose_terms(dp, c["pose_gt"].to(dtype), c["bbox_gt"].to(dtype), c["fill_gt"].to(dtype), c["class_gt"], labels, DG(mo),
                            mask_bg=mask_bg)
    finally:
        OL.sigmoid_focal_loss_mean = saved
        torch.set_default_dtype(saved_dtype)
    out = torch.stack([t[k].to(dtype) for k in ("pose_loss", "class_loss", "bbox_loss", "fill_factor_loss", "kl_loss_bbox")]
                      + [t[k].mean() for k in ("t1", "t2", "t3", "v3")])
    (out * torch.tensor(P.G9, dtype=dtype)).sum().backward()
    zero = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)
    return out.detach(), zero(dp), zero(mo)


_REFS = {}


def ref_of(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = P.pose_reference(c)
    return _REFS[c["name"]]


CASE_IDS = [c["name"] for c in P.POSE_CASES]


def test_case_list_covers_what_it_names():
    names = set(CASE_IDS)
    assert len(names) == len(CASE_IDS)
    assert {c["B"] for c in P.POSE_CASES} >= {1, 2, 255, 256, 257, 513, 1000}
    assert {c["NC"] for c in P.POSE_CASES} >= {1, 8, 11, 40} and {c["L"] for c in P.POSE_CASES} == {1, 3}
    assert {c["bg_idx"] for c in P.POSE_CASES} == {0, 1}
    assert {(c["l2"], c["yaw"]) for c in P.POSE_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["gamma"], c["alpha"]) for c in P.POSE_CASES} >= {(g, a) for g in (2.0, 1.5, 1.0, 0.0) for a in (0.25, 0.5)}
    c = P.pose_case("fg_last")
    fgm = c["class_gt"] != c["bg_idx"]
    assert fgm.nonzero().flatten().tolist() == [c["B"] - 1]
    c = P.pose_case("fg_tail")
    fgm = c["class_gt"] != c["bg_idx"]
    assert not fgm[:256].any() and fgm[256:].all()
    assert not (P.pose_case("all_bg")["class_gt"] != 1).any() and (P.pose_case("prior_neg")["prior_idx"] < 0).all()
    for name in CASE_IDS:
        c = P.pose_case(name)
        if c["B"] < 37:
            continue
        mixed = name not in ("all_bg", "fg_last", "fg_tail")
        fgm = c["class_gt"] != c["bg_idx"]
        tg = torch.arange(c["NC"])[None, :] == c["class_gt"][:, None]
        x = c["dec_pose"][:, 8:]
        for v in P.LOGITS:
            assert (x[~tg] == v).any(), (name, v)
            if c["NC"] >= 8 and mixed:
                assert (x[tg] == v).any(), (name, v, "positive column")
        assert not mixed or (c["class_gt"] == c["NC"]).any()
        for v in P.LOGVARS + [25.0, -40.0]:
            assert (c["moments"][:, 8:] == torch.tensor(v, dtype=torch.float32)).any(), (name, v)
        assert P.LOGVARS[1] < -30.0 and P.LOGVARS[3] > 20.0
        if mixed:
            for v in P.YAWS:
                assert (c["dec_pose"][fgm, 3] == torch.tensor(v, dtype=torch.float32)).any(), (name, v)
            assert ((c["dec_pose"][:, :3] == c["pose_gt"][:, :3]) & fgm[:, None]).any()          # d == 0 under L1
        if c["yaw"]:
            d = (torch.sin(c["dec_pose"][:, 3]) - torch.sin(c["pose_gt"][:, 3])).abs()
            assert (d == 1.0).any() and (d == 2.0).any()
        var = c["prior"][:, 1]
        assert (var == torch.tensor(1e-6)).any() and (var == torch.tensor(1e3)).any()
    assert (P.pose_case("B1")["prior_idx"] >= 0).all()          # the smallest batch runs the KL
    assert all(g != 0 for g in P.G9[:5])


@pytest.mark.parametrize("name", CASE_IDS)
def test_reference_is_the_float64_oracle(name):
    c = P.pose_case(name)
    ref = ref_of(c)
    out, d_pose, d_mom = oracle_terms(c, torch.float64)
    for what, got, want in (("out", out, ref["out"]), ("d_pose", d_pose, ref["d_pose"]), ("d_mom", d_mom, ref["d_mom"])):
        # float64 against float64.  The oracle's own cancellations (1 - sigmoid at a logit of 20) lose in float64 what the rule's bound
        # admits in f32, scaled from 2^-24 to 2^-53 -- taken with a factor 64 to spare; beside it 2^-43 of the value for the roundings of
        # up to 40000 additions
        bound = ref[what + "_bound"] * 2.0 ** -23 + 2.0 ** -43 * want.abs() + 1e-300
        assert torch.isfinite(want).all()
        excess = ((got - want).abs() / bound).max().item()
        assert excess <= 1.0, "%s: worst |err| / (bound 2^-23) = %.3g" % (what, excess)


@pytest.mark.parametrize("name", CASE_IDS)
def test_rule_admits_the_oracle_in_f32(name):
    c = P.pose_case(name)
    out, d_pose, d_mom = oracle_terms(c, torch.float32)
    P.assert_rule(ref_of(c), out, d_pose, d_mom, "oracle f32 on " + name)


@pytest.mark.parametrize("name", CASE_IDS)
def test_rule_admits_the_host_model_in_f32(name):
    c = P.pose_case(name)
    out, d_pose, d_mom, _ = P.pose_model(c, torch.float32)
    P.assert_rule(ref_of(c), out, d_pose, d_mom, "host model f32 on " + name)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_rule_rejects_the_planted_fault(fault):
    """every fault is rejected on every case in which it changes anything the rule could see: more than 16 ulps of some element"""
    rejected = []
    for c in P.POSE_CASES:
        ref = ref_of(c)
        out, d_pose, d_mom, _ = P.pose_model(c, torch.float32, fault=fault)
        good = P.pose_model(c, torch.float32)
        changed = any(((a.double() - b.double()).abs() > 16 * 2.0 ** -23 * b.double().abs()).any().item()
                      for a, b in zip((out, d_pose, d_mom), good[:3]))
        bad = P.rule_failures(ref, out, d_pose, d_mom)
        if changed and c["B"] <= 37:
            assert bad, "fault %s goes unnoticed on %s" % (fault, c["name"])
        if bad:
            rejected.append(c["name"])
    assert P.EDGE_CASE in rejected and len(rejected) >= 8, rejected
