"""odvae_gan_logit_terms_f32 / _bwd_f32 (csrc/gan_f32.hip) through the C ABI, and ops.gan_logit_terms on top of them.

  hinge terms, plain means, their gradients   bit for bit against the float64 model of tests/plain_vae_ref.py rounded once, on logits that
                                              are multiples of 1/8 in [-4, 4] (exact +-1 among them) and an upstream gradient of powers of
                                              two: no partial sum can round, so the order of the reduction cannot show
  softplus terms and their gradients          within 4x of what torch's own f32 F.softplus / mean / autograd is from float64 on the same
                                              logits (plain_vae_ref.TORCH_SOFTPLUS_FIGURES, measured on the host by test_plain_vae_ref.py):
                                              out 4 x 1.3 ulp, gradients 4 x 2.3 units of 2^-24 max|dout| / n.  Measured on an MI355X: see
                                              profiles/plain_vae.md
Sizes 1 ... 28 800 (N = 32 at 256 x 256), one past the grid cap of the partial stage (1024 blocks of 256 threads), n_real != n_fake,
real = NULL.  Outputs sit in canary buffers, the workspace is exactly the bytes the library asks for."""
import numpy as np
import pytest
import torch

import plain_vae_ref as R
from canary_buffers import DEV, assert_canary, assert_workspace_canary, out_buf, padded, workspace

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_WORKSPACE = 1, 2           # ODVAE_ERR_ARG, ODVAE_ERR_WORKSPACE


def run_terms(L, real, fake, short=0):
    """out6 (numpy f32) of one forward call; `short` bytes are withheld from the workspace and the return code comes back instead"""
    from odvae_amd import lib
    n_real = 0 if real is None else len(real)
    fb, fd = padded(torch.from_numpy(fake))
    rb, rd = (None, None) if real is None else padded(torch.from_numpy(real))
    ob, out = out_buf(6)
    need = L.odvae_gan_logit_terms_workspace_bytes(n_real, len(fake))
    assert need == min(max(-(-max(n_real, len(fake)) // 256), 1), R.GRID_CAP_BLOCKS) * 6 * 8
    ws = workspace(need - short)
    rc = L.odvae_gan_logit_terms_f32(None if rd is None else rd.data_ptr(), n_real, fd.data_ptr(), len(fake), out.data_ptr(), ws.data_ptr(),
                                     need - short, lib.stream_ptr())
    torch.cuda.synchronize()
    assert_canary(fb, ob, *([] if rb is None else [rb]))
    assert_workspace_canary(ws)
    if short:
        return rc, out.cpu().numpy()
    lib.check(rc, "odvae_gan_logit_terms_f32")
    return out.cpu().numpy()


def run_bwd(L, real, fake, dout, want_real=True, want_fake=True):
    from odvae_amd import lib
    n_real = 0 if real is None else len(real)
    fb, fd = padded(torch.from_numpy(fake))
    rb, rd = (None, None) if real is None else padded(torch.from_numpy(real))
    db, dd = padded(torch.from_numpy(np.asarray(dout, dtype=np.float32)))
    bufs = [fb, db] + ([] if rb is None else [rb])
    dreal = dfake = None
    if want_real and real is not None:
        b, dreal = out_buf(n_real)
        bufs.append(b)
    if want_fake:
        b, dfake = out_buf(len(fake))
        bufs.append(b)
    lib.check(L.odvae_gan_logit_terms_bwd_f32(None if rd is None else rd.data_ptr(), n_real, fd.data_ptr(), len(fake), dd.data_ptr(),
                                              None if dreal is None else dreal.data_ptr(), None if dfake is None else dfake.data_ptr(),
                                              lib.stream_ptr()), "odvae_gan_logit_terms_bwd_f32")
    torch.cuda.synchronize()
    assert_canary(*bufs)
    return (None if dreal is None else dreal.cpu().numpy()), (None if dfake is None else dfake.cpu().numpy())


def bits(a):
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)      # (+0.0: a sum that is exactly zero has no sign to compare)


def assert_bits(got, want64, what):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)      # float64 rounded once
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, "%s: %d of %d differ in bits; first at %d: got %r, want %r" % (what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("n", R.SIZES + [R.PAST_CAP])
def test_hinge_terms_and_means_bit_for_bit(hip_lib, n):
    real, fake = R.dyadic_logits(n, 1), R.dyadic_logits(n, 2)
    R.assert_partial_sums_exact(real)
    R.assert_partial_sums_exact(fake)
    out = run_terms(hip_lib, real, fake)
    assert_bits(out[:4], R.logit_terms_f64(real, fake)[:4], "out[:4] at n = %d" % n)
    assert np.isfinite(out[4:]).all()
    dreal, dfake = run_bwd(hip_lib, real, fake, R.DOUT_HINGE)
    wr, wf = R.logit_terms_grad_f64(real, fake, R.DOUT_HINGE)
    assert_bits(dreal, wr, "dreal at n = %d" % n)
    assert_bits(dfake, wf, "dfake at n = %d" % n)
    if n >= 9:      # the kink is among the logits, and it is on the zero side: relu'(0) = 0
        assert (dreal[real == 1.0] == np.float32(0.5 / n)).all() and (dfake[fake == -1.0] == np.float32(-2.0 / n)).all()


@pytest.mark.parametrize("n_real,n_fake", R.UNEQUAL)
def test_unequal_counts(hip_lib, n_real, n_fake):
    real, fake = R.dyadic_logits(n_real, 1), R.dyadic_logits(n_fake, 2)
    assert_bits(run_terms(hip_lib, real, fake)[:4], R.logit_terms_f64(real, fake)[:4], "out[:4]")
    dreal, dfake = run_bwd(hip_lib, real, fake, R.DOUT_HINGE)
    wr, wf = R.logit_terms_grad_f64(real, fake, R.DOUT_HINGE)
    assert_bits(dreal, wr, "dreal")
    assert_bits(dfake, wf, "dfake")
    # one gradient alone
    only_real, none = run_bwd(hip_lib, real, fake, R.DOUT_HINGE, want_fake=False)
    assert none is None and np.array_equal(bits(only_real), bits(dreal))
    none, only_fake = run_bwd(hip_lib, real, fake, R.DOUT_HINGE, want_real=False)
    assert none is None and np.array_equal(bits(only_fake), bits(dfake))


@pytest.mark.parametrize("n", [1, 257, 28800])
def test_generator_phase_has_no_real_logits(hip_lib, n):
    fake = R.dyadic_logits(n, 2)
    out = run_terms(hip_lib, None, fake)
    assert out[[0, 2, 4]].tolist() == [0.0, 0.0, 0.0]
    assert_bits(out[[1, 3]], R.logit_terms_f64(None, fake)[[1, 3]], "out[1], out[3]")
    none, dfake = run_bwd(hip_lib, None, fake, R.DOUT_HINGE)
    assert none is None
    assert_bits(dfake, R.logit_terms_grad_f64(None, fake, R.DOUT_HINGE)[1], "dfake")


def test_softplus_terms_within_4x_of_torch(hip_lib):
    worst = {}
    for n_real, n_fake in R.SOFTPLUS_CASES + [(R.PAST_CAP, 900)]:
        real, fake = R.softplus_logits(n_real, 1), R.softplus_logits(n_fake, 2)
        out = run_terms(hip_lib, real, fake)
        dreal, dfake = run_bwd(hip_lib, real, fake, R.DOUT_FULL)
        assert np.isfinite(out).all()
        f = R.softplus_figures(out, dreal, dfake, real, fake, R.DOUT_FULL)
        print("softplus terms at n = (%d, %d): %s" % (n_real, n_fake, f))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the plain means and hinge terms of the same call, on logits that are no dyadic numbers: one rounding of the float64 value
        assert R.ulp_distance(out[:4], R.logit_terms_f64(real, fake)[:4]).max() <= 0.5 + 1e-6
    print("softplus terms, worst: %s (torch f32 on the host: %s)" % (worst, R.TORCH_SOFTPLUS_FIGURES))
    for k, v in worst.items():
        assert v <= R.SOFTPLUS_MARGIN * R.TORCH_SOFTPLUS_FIGURES[k], (k, v)


def test_softplus_is_finite_and_right_at_100(hip_lib):
    x = np.array([100.0, -100.0, 0.0], dtype=np.float32)
    out = run_terms(hip_lib, x, x)
    dout = np.array([0, 0, 0, 0, 1.0, 1.0], dtype=np.float32)
    dreal, dfake = run_bwd(hip_lib, x, x, dout)
    # the closed forms: softplus(+-100) = 100 | 0 and sigmoid(+-100) = 1 | 0 to far below f32, softplus(0) = ln 2, sigmoid(0) = 1 / 2
    want = R.logit_terms_f64(x, x)
    assert abs(want[4] - (100.0 + np.log(2.0)) / 3) < 1e-13 and abs(want[5] - want[4]) < 1e-13
    wr, wf = R.logit_terms_grad_f64(x, x, dout)
    assert np.allclose(wr * 3, [0.0, -1.0, -0.5], atol=1e-40) and np.allclose(wf * 3, [1.0, 0.0, 0.5], atol=1e-40)
    f = R.softplus_figures(out, dreal, dfake, x, x, dout)       # the rule of the test above, at these three points alone
    for k, v in f.items():
        assert v <= R.SOFTPLUS_MARGIN * R.TORCH_SOFTPLUS_FIGURES[k], (k, v)


def test_a_nan_logit_poisons_exactly_its_terms(hip_lib):
    real, fake = R.dyadic_logits(900, 1), R.dyadic_logits(900, 2)
    bad = real.copy()
    bad[517] = np.nan
    out = run_terms(hip_lib, bad, fake)
    assert np.isnan(out[[0, 2, 4]]).all() and np.array_equal(bits(out[[1, 3, 5]]), bits(run_terms(hip_lib, real, fake)[[1, 3, 5]]))
    dreal, dfake = run_bwd(hip_lib, bad, fake, R.DOUT_FULL)
    good_r, good_f = run_bwd(hip_lib, real, fake, R.DOUT_FULL)
    assert np.isnan(dreal[517]) and np.array_equal(bits(np.delete(dreal, 517)), bits(np.delete(good_r, 517)))
    assert np.array_equal(bits(dfake), bits(good_f))
    bad = fake.copy()
    bad[0] = np.nan
    out = run_terms(hip_lib, real, bad)
    assert np.isnan(out[[1, 3, 5]]).all() and np.isfinite(out[[0, 2, 4]]).all()
    out = run_terms(hip_lib, real, np.where(np.arange(900) == 899, np.float32(np.inf), fake).astype(np.float32))
    assert out[1] == np.inf and out[3] == np.inf and out[5] == np.inf and np.isfinite(out[[0, 2, 4]]).all()


@pytest.mark.parametrize("n", [1, 257, R.PAST_CAP])
def test_a_workspace_one_byte_short_is_refused(hip_lib, n):
    x = R.dyadic_logits(n, 1)
    rc, out = run_terms(hip_lib, x, x, short=1)
    assert rc == ERR_WORKSPACE and np.isnan(out).all()          # nothing was launched
    assert b"workspace" in hip_lib.odvae_last_error()


def test_bad_arguments_are_refused(hip_lib):
    from odvae_amd import lib
    _, x = padded(torch.zeros(8))
    _, out = out_buf(6)
    ws = workspace(64)
    s = lib.stream_ptr()
    L = hip_lib
    assert L.odvae_gan_logit_terms_f32(x.data_ptr(), 8, None, 8, out.data_ptr(), ws.data_ptr(), 64, s) == ERR_ARG        # no fake logits
    assert L.odvae_gan_logit_terms_f32(x.data_ptr(), 8, x.data_ptr(), 0, out.data_ptr(), ws.data_ptr(), 64, s) == ERR_ARG
    assert L.odvae_gan_logit_terms_f32(None, 8, x.data_ptr(), 8, out.data_ptr(), ws.data_ptr(), 64, s) == ERR_ARG          # NULL real with a count
    assert L.odvae_gan_logit_terms_f32(x.data_ptr(), -1, x.data_ptr(), 8, out.data_ptr(), ws.data_ptr(), 64, s) == ERR_ARG
    assert L.odvae_gan_logit_terms_f32(x.data_ptr(), 8, x.data_ptr(), 8, None, ws.data_ptr(), 64, s) == ERR_ARG
    assert L.odvae_gan_logit_terms_f32(x.data_ptr(), 8, x.data_ptr(), 8, out.data_ptr(), None, 64, s) == ERR_WORKSPACE
    assert L.odvae_gan_logit_terms_bwd_f32(x.data_ptr(), 8, x.data_ptr(), 8, out.data_ptr(), None, None, s) == ERR_ARG      # no output asked for
    assert L.odvae_gan_logit_terms_bwd_f32(None, 0, x.data_ptr(), 8, out.data_ptr(), x.data_ptr(), None, s) == ERR_ARG      # dreal without real
    assert L.odvae_gan_logit_terms_bwd_f32(x.data_ptr(), 8, x.data_ptr(), 8, None, x.data_ptr(), None, s) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_two_runs_are_bit_identical(hip_lib):
    rng = np.random.RandomState(7)
    real, fake = (rng.randn(28800) * 3).astype(np.float32), (rng.randn(28800) * 3).astype(np.float32)
    a, b = run_terms(hip_lib, real, fake), run_terms(hip_lib, real, fake)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ga, gb = run_bwd(hip_lib, real, fake, R.DOUT_FULL), run_bwd(hip_lib, real, fake, R.DOUT_FULL)
    assert np.array_equal(ga[0].view(np.uint32), gb[0].view(np.uint32)) and np.array_equal(ga[1].view(np.uint32), gb[1].view(np.uint32))


# ---- the op layer --------------------------------------------------------------------------------------------------------------------
def test_op_is_the_kernel_pair_with_autograd(hip_lib):
    from odvae_amd import ops
    real_np, fake_np = R.softplus_logits(900, 1), R.softplus_logits(450, 2)
    real = torch.from_numpy(real_np).to(DEV).reshape(1, 1, 30, 30).requires_grad_()
    fake = torch.from_numpy(fake_np).to(DEV).reshape(2, 1, 15, 15).requires_grad_()
    out = ops.gan_logit_terms(real, fake)
    assert out.shape == (6,) and out.dtype == torch.float32 and out.is_cuda
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), run_terms(hip_lib, real_np, fake_np).view(np.uint32))
    (out * torch.from_numpy(R.DOUT_FULL).to(DEV)).sum().backward()
    wr, wf = run_bwd(hip_lib, real_np, fake_np, R.DOUT_FULL)
    assert real.grad.shape == real.shape and fake.grad.shape == fake.shape
    assert np.array_equal(real.grad.cpu().numpy().reshape(-1).view(np.uint32), wr.view(np.uint32))
    assert np.array_equal(fake.grad.cpu().numpy().reshape(-1).view(np.uint32), wf.view(np.uint32))
    # (the losses these terms serve are held to the float64 restatement in tests/test_plain_vae_gpu.py, hinge and vanilla)


def test_op_generator_phase_and_detached_inputs(hip_lib):
    from odvae_amd import ops
    fake_np = R.dyadic_logits(257, 2)
    fake = torch.from_numpy(fake_np).to(DEV).requires_grad_()
    out = ops.gan_logit_terms(None, fake)
    assert out[[0, 2, 4]].tolist() == [0.0, 0.0, 0.0]
    (-out[1]).backward()                                    # g_loss = -mean D(x_rec)
    assert torch.equal(fake.grad, torch.full_like(fake, -1.0 / 257))
    real = torch.from_numpy(R.dyadic_logits(63, 1)).to(DEV)      # no gradient asked for the real logits
    fake.grad = None
    ops.gan_logit_terms(real, fake)[3].backward()
    assert_bits(fake.grad.cpu().numpy(), R.logit_terms_grad_f64(real.cpu().numpy(), fake_np, [0, 0, 0, 1.0, 0, 0])[1], "dfake")
    assert not ops.gan_logit_terms(real, fake.detach()).requires_grad
