"""CPU: the float64 restatement of the alpha-mask branch (tests/image_mask_ref.py) is held to what the REFERENCE's PoseLoss.forward
returned and logged (tests/golden/reference_mask.npz), every planted misreading of that branch is rejected by the same comparison, and
the exactly summable inputs of tests/test_rgba_terms_gpu.py meet their precondition.

Tolerances: the fixture is the reference's code evaluated in float64 and so is the restatement; what separates them is the order of
float64 additions (2^-53 per operation over sums of at most 2^14 terms, condition numbers of the logit means ~1e3): 1e-9 relative with
1e-12 absolute for a scalar, 1e-9 of the gradient's norm."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import image_mask_ref as R  # noqa: E402

GOLD = os.path.join(HERE, "golden", "reference_mask.npz")
STEPS = (5, 12, 20, 40)
RTOL, ATOL, GTOL = 1e-9, 1e-12, 1e-9


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def inputs(gold):
    return {k[3:]: (torch.from_numpy(gold[k]).double() if gold[k].dtype.kind == "f" else torch.from_numpy(gold[k]))
            for k in gold.files if k.startswith("in.") and k != "in.global_steps"}


def mismatches(gold, pre, out):
    """The fixture's entries under `pre` that `out` = (loss, log, grad) misses, as (key, got, want) triples."""
    loss, log, grad = out
    bad = []

    def scalar(key, got, want):
        got, want = float(got), float(want)
        # (the reference gathers the box-posterior KL per sample in an f32 torch.zeros buffer, :195, whatever the dtype of its inputs)
        rtol = 2.0 ** -22 if "kl_loss_bbox" in key else RTOL
        if not abs(got - want) <= rtol * abs(want) + ATOL:
            bad.append((key, got, want))

    scalar("loss_mean", loss, gold[pre + ".loss_mean"])
    keys = [f[len(pre + ".log.train/"):] for f in gold.files if f.startswith(pre + ".log.")]
    assert sorted(keys) == sorted(log.keys()), (sorted(keys), sorted(log.keys()))
    for k in keys:
        scalar(k, log[k], gold[pre + ".log.train/" + k])
    if pre + ".grad.dec_obj.norm" in gold.files:
        assert grad is not None
        gn = float(gold[pre + ".grad.dec_obj.norm"])
        norm, samples = R.digest_small(grad)
        if not abs(norm - gn) <= GTOL * gn:
            bad.append(("grad.norm", norm, gn))
        e = float(np.abs(samples - gold[pre + ".grad.dec_obj.samples"]).max())
        if not e <= GTOL * gn:
            bad.append(("grad.samples", e, gn))
    else:
        assert grad is None or float(grad.abs().max()) == 0.0
    return bad


def run_all(gold, inputs, fn, uml, faults=()):
    """Every case of one (use_mask_loss, mask_loss_fn) pair on one loss object, as the fixture's generator ran them."""
    ref = R.MaskLossRef(fn, use_mask_loss=uml, faults=faults)
    bad = []
    for gs in STEPS:
        for opt in (0, 1):
            pre = "mask.uml%d.%s.step%d.opt%d" % (int(uml), fn, gs, opt)
            bad += [(pre,) + b for b in mismatches(gold, pre, ref(inputs, opt, gs))]
    return bad


def run_sticky(gold, inputs, fn, faults=()):
    ref = R.MaskLossRef(fn, use_mask_loss=True, faults=faults)
    assert ref(inputs, 2, 40, with_mask=False) is None
    pre = "sticky.%s.step40.opt0" % fn
    return [(pre,) + b for b in mismatches(gold, pre, ref(inputs, 0, 40))]


@pytest.mark.parametrize("fn", ["l1", "l2"])
@pytest.mark.parametrize("uml", [True, False])
def test_restatement_matches_the_reference(gold, inputs, fn, uml):
    assert run_all(gold, inputs, fn, uml) == []


@pytest.mark.parametrize("fn", ["l1", "l2"])
def test_use_mask_loss_is_sticky_in_the_reference(gold, inputs, fn):
    assert float(gold["sticky.%s.step40.opt0.log.train/mask_loss" % fn]) == 0.0
    assert float(gold["mask.uml1.%s.step40.opt0.log.train/mask_loss" % fn]) > 0.1
    assert run_sticky(gold, inputs, fn) == []


def test_the_reference_returns_a_tensor_only_in_the_full_phase_with_the_mask_loss(gold):
    for uml in (0, 1):
        for fn in ("l1", "l2"):
            for gs in STEPS:
                for opt in (0, 1):
                    shape = tuple(gold["mask.uml%d.%s.step%d.opt%d.loss_shape" % (uml, fn, gs, opt)])
                    assert shape == ((4, 1, 32, 32) if (uml and opt == 0 and gs > 10) else ()), (uml, fn, gs, opt, shape)


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f != "not_sticky"])
def test_a_planted_fault_is_rejected(gold, inputs, fault):
    bad = run_all(gold, inputs, "l2", True, faults=(fault,))
    assert bad, "the fixture does not see %s" % fault
    seen = {b[1] for b in bad}
    expect = {"times_mask_bg": "mask_loss", "summed": "mask_loss", "l1_all4": "rec_loss", "alpha_unboxed": "mask_loss",
              "disc_rgb_only": "g_loss"}[fault]
    assert expect in seen, (fault, sorted(seen))


def test_dropped_stickiness_is_rejected(gold, inputs):
    bad = run_sticky(gold, inputs, "l2", faults=("not_sticky",))
    assert "mask_loss" in {b[1] for b in bad}


@pytest.mark.parametrize("hw,q,a", [(1, 8, 2), (7, 8, 2), (64, 8, 2), (255, 8, 2), (256, 8, 2), (257, 8, 2), (4100, 8, 2), (65536 + 259, 2, 1)])
def test_exact_inputs_meet_their_precondition(hw, q, a):
    """Every partial sum of the kernel on these inputs is exact: the bound of image_mask_ref.sums_are_exact, and -- checked directly -- the
    f32 running sums taken in two different orders equal the float64 sums bit for bit."""
    assert R.sums_are_exact(hw, q, a)
    rec, rgb, alpha, box = R.exact_rgba_inputs(2, hw, seed=hw, q=q, a=a)
    for l2 in (False, True):
        l1, ms = R.rgba_terms_f64(rec, rgb, alpha, box, l2)[:2]
        w = box[..., None]
        t1 = (rgb * w - rec[..., :3] * w).abs().sum(-1).float()
        d = (alpha * box - rec[..., 3] * box).float()
        t2 = d * d if l2 else d.abs()
        for t, want in ((t1, l1), (t2, ms)):
            assert torch.equal(t.double().sum(1), want)
            assert torch.equal(torch.cumsum(t, 1)[:, -1].double(), want) and torch.equal(torch.cumsum(t.flip(1), 1)[:, -1].double(), want)
            assert torch.equal(want.float().double(), want)
    assert not R.sums_are_exact(4100, 8, 4)      # (what a wider value range would break)
