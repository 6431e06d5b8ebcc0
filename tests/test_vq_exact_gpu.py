"""csrc/vq_f32.hip through the C ABI.

Exactly summable operands (tests/vq_inputs.exact_case: whole numbers |v| <= 8, every score exact in f32 in any order): indices equal the
float64 argmin with the lowest-index rule bit for bit, z_q equals the codebook rows in bits, dz and dE equal float64 in bits.  The kernels
form dz and dE in f64 with one rounding (no contraction), and the float64 reference repeats their order of operations, so this holds at
every shape, not only where M D is a power of two (those are among the cases).  The loss takes differences, squares and sums in f64 and
rounds once: it is held to 1.01 * 2^-24 relative (the issue's 4 * 2^-24 is for squares taken in f32).

Gaussian operands: indices under the rule of tests/vq_inputs.py (n = D + 2: one fmaf chain per dot product and per norm, one subtraction;
no MFMA path, so no other n); everything else against float64 taken AT THE DEVICE'S INDICES: dz within 3 roundings, dE[k] within
gamma_{c_k + 3} sum |terms|.
"""
import numpy as np
import pytest
import torch

import canary_buffers as C
import vq_inputs as V

pytestmark = pytest.mark.gpu
DEV = C.DEV
BETA = 0.25
ERR_ARG, ERR_WORKSPACE = 1, 2


def strides(layout, d, hw):
    return (d * hw, hw, 1) if layout == "nchw" else (hw * d, 1, d)


def pack(rows, n, hw, layout):
    rows = np.asarray(rows, dtype=np.float32)
    return V.to_nchw(rows, n, hw).reshape(-1) if layout == "nchw" else np.ascontiguousarray(rows).reshape(-1)


def unpack(flat, n, hw, d, layout):
    flat = np.asarray(flat)
    return V.from_nchw(flat.reshape(n, d, hw)) if layout == "nchw" else flat.reshape(n * hw, d)


def assign(L, rows, E, n, hw, layout="nchw", beta=BETA):
    """(idx, z_q rows, loss) of odvae_vq_assign_f32 + odvae_vq_loss_finalize, canaries checked"""
    m, d = rows.shape
    k = E.shape[0]
    assert m == n * hw
    sn, sc, sp = strides(layout, d, hw)
    zbuf, z = C.padded(torch.tensor(pack(rows, n, hw, layout)))
    ebuf, e = C.padded(torch.tensor(np.ascontiguousarray(E, dtype=np.float32)))
    ibuf = torch.full((m + C.PAD,), -7, dtype=torch.int64, device=DEV)
    qbuf, zq = C.out_buf(m * d)
    lbuf, loss = C.out_buf(1)
    nbytes = L.odvae_vq_assign_workspace_bytes(m, k, d)
    assert nbytes > 0
    ws = C.workspace(nbytes)
    C.call(L.odvae_vq_assign_f32, z.data_ptr(), sn, sc, sp, n, hw, d, e.data_ptr(), k, ibuf.data_ptr(), zq.data_ptr(), sn, sc, sp,
           ws.data_ptr(), nbytes)
    C.call(L.odvae_vq_loss_finalize, ws.data_ptr(), nbytes, m, k, d, beta, loss.data_ptr())
    torch.cuda.synchronize()
    C.assert_canary(zbuf, ebuf, qbuf, lbuf)
    C.assert_workspace_canary(ws)
    assert (ibuf[m:] == -7).all().item(), "the kernel wrote past the end of the indices"
    assert np.array_equal(zbuf[:m * d].cpu().numpy(), pack(rows, n, hw, layout), equal_nan=True), "the input was written to"
    return ibuf[:m].cpu().numpy(), unpack(zq.cpu().numpy(), n, hw, d, layout), float(loss.item())


def backward(L, rows, E, idx, gq, gl, n, hw, layout="nchw", beta=BETA, legacy=True, want_dz=True, want_de=True):
    m, d = rows.shape
    k = E.shape[0]
    sn, sc, sp = strides(layout, d, hw)
    zbuf, z = C.padded(torch.tensor(pack(rows, n, hw, layout)))
    ebuf, e = C.padded(torch.tensor(np.ascontiguousarray(E, dtype=np.float32)))
    gbuf, g = C.padded(torch.tensor(pack(gq, n, hw, layout))) if gq is not None else (None, None)
    idx_t = torch.tensor(np.asarray(idx, dtype=np.int64), device=DEV)
    gl_t = torch.tensor([gl], dtype=torch.float32, device=DEV)
    dzbuf, dz = C.out_buf(m * d)
    debuf, de = C.out_buf(k * d)
    nbytes = L.odvae_vq_backward_workspace_bytes(m, k, d)
    ws = C.workspace(nbytes)
    C.call(L.odvae_vq_backward_f32, z.data_ptr(), None if g is None else g.data_ptr(), dz.data_ptr() if want_dz else None, sn, sc, sp, n, hw, d,
           e.data_ptr(), k, idx_t.data_ptr(), gl_t.data_ptr(), beta, int(legacy), de.data_ptr() if want_de else None, ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    C.assert_canary(zbuf, ebuf, dzbuf, debuf)
    C.assert_workspace_canary(ws)
    dz_rows = unpack(dz.cpu().numpy(), n, hw, d, layout)
    return dz_rows, de.cpu().numpy().reshape(k, d)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def check_exact(L, rows, E, n, hw, layout, legacy=True, gl=1.0, seed=0):
    m, d = rows.shape
    want_idx = V.assign_f64(rows, E)
    idx, zq, loss = assign(L, rows, E, n, hw, layout)
    assert np.array_equal(idx, want_idx), "indices differ at rows %s" % np.nonzero(idx != want_idx)[0][:8]
    assert np.array_equal(bits(zq), bits(E[want_idx]))
    _, want_loss = V.quantize_f64(rows, E, want_idx, BETA)
    assert abs(loss - want_loss) <= 1.01 * V.U * abs(want_loss), (loss, want_loss)
    rng = np.random.RandomState(seed + 1)
    gq = (rng.randint(-16, 17, size=rows.shape) / 8.0).astype(np.float32)
    dz, de = backward(L, rows, E, idx, gq, gl, n, hw, layout, legacy=legacy)
    want_dz, want_de = V.backward_f64(rows, E, want_idx, gq, gl, BETA, legacy)
    assert np.array_equal(bits(dz), bits(want_dz.astype(np.float32)))
    assert np.array_equal(bits(de), bits(want_de.astype(np.float32)))
    return idx


def test_plan_is_what_the_inputs_module_assumes(hip_lib):
    from odvae_amd import ops
    p = ops.vq_plan(100, 300, 4)
    assert p["chunk"] == V.CHUNK and p["tile_rows"] == 64


@pytest.mark.parametrize("d", [1, 3, 4, 8, 17, 64, 256])
def test_exact_over_shapes(hip_lib, d):
    """K at 1, 2, one chunk - 1 / exact / + 1, 257, 1024, 5000 x (N, HW) with ragged row tiles and rows of two images in one tile; the layout
    alternates between NCHW and NHWC memory, legacy between True and False"""
    case = 0
    for k in (1, 2, V.CHUNK - 1, V.CHUNK, V.CHUNK + 1, 257, 1024, 5000):
        for n, hw in ((1, 1), (3, 7), (1, 64), (3, 100)):
            rows, E = V.exact_case(n * hw, d, k, seed=1000 * d + case)
            check_exact(hip_lib, rows, E, n, hw, "nchw" if case % 2 == 0 else "nhwc", legacy=case % 3 != 0, seed=case)
            case += 1


@pytest.mark.parametrize("d", [1, 4, 8, 64, 256])
def test_exact_with_power_of_two_scales(hip_lib, d):
    """M D a power of two and g_l = 1: the scales 2 c / (M D) are exact, so the float64 values are f32 numbers to begin with"""
    for n, hw in ((1, 64), (2, 64)):
        rows, E = V.exact_case(n * hw, d, 100, seed=d)
        for legacy in (True, False):
            check_exact(hip_lib, rows, E, n, hw, "nchw", legacy=legacy, gl=1.0)


def planted_case(m, k, d=4):
    """(rows, E, aimed): row r's exact nearest code is aimed[r] -- index 0, K - 1, the first two chunk boundaries - 1 / exact / + 1 and, where
    the plan splits the codebook, the first three and the last split boundary likewise; then duplicate codebook rows inside one chunk
    (5 and 9), across the third chunk boundary and across the fifth split boundary, where the lowest index has to win"""
    from odvae_amd import ops
    plan = ops.vq_plan(m, k, d)
    cps, nsplit = plan["codes_per_split"], plan["nsplit"]
    edges = {0, k - 1}
    bounds = [V.CHUNK, 2 * V.CHUNK]
    if nsplit > 1:
        assert nsplit >= 8 and cps % V.CHUNK == 0 and cps > 3 * V.CHUNK
        bounds += [cps, 2 * cps, 3 * cps, (nsplit - 1) * cps]
    for c in bounds:
        edges.update({c - 1, c, c + 1})
    aimed = sorted(e for e in edges if 0 <= e < k)
    dups = [(5, 9), (3 * V.CHUNK - 1, 3 * V.CHUNK)] + ([(5 * cps - 1, 5 * cps)] if nsplit > 1 else [])
    assert len(aimed) + len(dups) <= m and not {c for pair in dups for c in pair} & set(aimed)
    rows, E = V.exact_case(m, d, k, seed=k)
    for r, code in enumerate(aimed):
        V.plant_winner(rows, E, r, code)
    for j, (low, high) in enumerate(dups):
        V.plant_winner(rows, E, len(aimed) + j, low, dup=high)
    aimed = aimed + [low for low, _ in dups]
    assert list(V.assign_f64(rows, E)[:len(aimed)]) == aimed, "the planted case does not aim where it says"
    return rows, E, aimed, plan


@pytest.mark.parametrize("m,k", [(70, 3 * V.CHUNK + 5), (128, 5000)])
def test_planted_winners_at_every_edge(hip_lib, m, k):
    rows, E, aimed, plan = planted_case(m, k)
    assert (plan["nsplit"] > 1) == (k == 5000), plan
    idx = check_exact(hip_lib, rows, E, 1, m, "nchw")
    assert list(idx[:len(aimed)]) == aimed
    idx = check_exact(hip_lib, rows, E, 2, m // 2, "nhwc", legacy=False)
    assert list(idx[:len(aimed)]) == aimed


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_nan_and_inf_rows(hip_lib, layout):
    n, hw, d, k = 2, 50, 4, 130
    rows, E = V.exact_case(n * hw, d, k, seed=5)
    clean = rows.copy()
    rows[7, 2] = np.nan
    rows[64] = np.nan
    rows[20, 1] = np.inf
    rows[21, 0] = -np.inf
    idx, zq, loss = assign(hip_lib, rows, E, n, hw, layout)
    assert idx[7] == 0 and idx[64] == 0 and ((idx >= 0) & (idx < k)).all()
    ok = np.ones(n * hw, dtype=bool); ok[[7, 64, 20, 21]] = False
    assert np.array_equal(idx[ok], V.assign_f64(clean, E)[ok]), "a NaN / inf row disturbed its neighbours"
    assert np.array_equal(bits(zq), bits(E[idx]))


def test_grid_loops_past_their_caps(hip_lib):
    """M past the search cap (16 384 row tiles), the finish cap (4 096 workgroups) and the streaming cap (8 192 workgroups of 256 rows):
    D = 1, K = 2 keeps it to a few MB"""
    from odvae_amd import ops
    m = 8192 * 256 + 300
    plan = ops.vq_plan(m, 2, 1)
    assert -(-m // plan["tile_rows"]) > plan["search_grid_cap"] and -(-m // 256) > plan["finish_cap"] and -(-m // 256) > plan["stream_grid_cap"]
    rng = np.random.RandomState(3)
    rows = rng.randint(-8, 9, size=(m, 1)).astype(np.float32)
    E = np.array([[-3.0], [4.0]], dtype=np.float32)
    check_exact(hip_lib, rows, E, 1, m, "nchw")
    L = hip_lib
    idx = torch.tensor(V.assign_f64(rows, E), device=DEV)
    obuf, out = C.out_buf(m)
    ebuf, e = C.padded(torch.tensor(E))
    C.call(L.odvae_vq_gather_f32, idx.data_ptr(), 1, m, e.data_ptr(), 2, 1, out.data_ptr(), m, m, 1)
    cbuf = torch.full((2 + C.PAD,), -7, dtype=torch.int32, device=DEV)
    ubuf, u = C.out_buf(2)
    C.call(L.odvae_vq_usage, idx.data_ptr(), m, 2, cbuf.data_ptr(), u.data_ptr())
    torch.cuda.synchronize()
    C.assert_canary(obuf, ubuf)
    assert np.array_equal(out.cpu().numpy(), E[idx.cpu().numpy(), 0])
    assert np.array_equal(cbuf[:2].cpu().numpy(), np.bincount(idx.cpu().numpy(), minlength=2)) and (cbuf[2:] == -7).all().item()


def test_null_halves_and_short_workspaces(hip_lib):
    from odvae_amd import lib
    L = hip_lib
    n, hw, d, k = 2, 33, 4, 70
    rows, E = V.exact_case(n * hw, d, k, seed=8)
    idx = V.assign_f64(rows, E)
    gq = np.ones_like(rows)
    want_dz, want_de = V.backward_f64(rows, E, idx, gq, 1.0, BETA, True)
    dz, de = backward(L, rows, E, idx, gq, 1.0, n, hw, want_de=False)
    assert np.array_equal(bits(dz), bits(want_dz.astype(np.float32))) and np.isnan(de).all()          # NULL dE: untouched
    dz, de = backward(L, rows, E, idx, gq, 1.0, n, hw, want_dz=False)
    assert np.array_equal(bits(de), bits(want_de.astype(np.float32))) and np.isnan(dz).all()          # NULL dz: untouched
    dz, de = backward(L, rows, E, idx, None, 1.0, n, hw)                                              # NULL g_q counts as zero
    want_dz0, _ = V.backward_f64(rows, E, idx, None, 1.0, BETA, True)
    assert np.array_equal(bits(dz), bits(want_dz0.astype(np.float32))) and np.array_equal(bits(de), bits(want_de.astype(np.float32)))
    # a workspace one byte short is refused, and nothing is launched
    m = n * hw
    z = torch.tensor(pack(rows, n, hw, "nchw"), device=DEV)
    e = torch.tensor(E, device=DEV)
    ibuf = torch.full((m,), -7, dtype=torch.int64, device=DEV)
    zq = torch.full((m * d,), float("nan"), device=DEV)
    nbytes = L.odvae_vq_assign_workspace_bytes(m, k, d)
    ws = C.workspace(nbytes)
    rc = L.odvae_vq_assign_f32(z.data_ptr(), d * hw, hw, 1, n, hw, d, e.data_ptr(), k, ibuf.data_ptr(), zq.data_ptr(), d * hw, hw, 1, ws.data_ptr(),
                               nbytes - 1, lib.stream_ptr())
    assert rc == ERR_WORKSPACE
    nb = L.odvae_vq_backward_workspace_bytes(m, k, d)
    de_t = torch.full((k * d,), float("nan"), device=DEV)
    idx_t = torch.tensor(idx, device=DEV)
    gl_t = torch.ones(1, device=DEV)
    rc = L.odvae_vq_backward_f32(z.data_ptr(), None, None, d * hw, hw, 1, n, hw, d, e.data_ptr(), k, idx_t.data_ptr(), gl_t.data_ptr(), BETA, 1,
                                 de_t.data_ptr(), ws.data_ptr(), nb - 1, lib.stream_ptr())
    assert rc == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (ibuf == -7).all().item() and torch.isnan(zq).all().item() and torch.isnan(de_t).all().item()
    # sizes outside the supported range are an error code
    for mm, kk, dd in ((m, k, 0), (m, k, 513), (m, 0, d), (m, (1 << 20) + 1, d)):
        assert L.odvae_vq_assign_workspace_bytes(mm, kk, dd) == 0
    rc = L.odvae_vq_assign_f32(z.data_ptr(), d * hw, hw, 1, n, hw, 513, e.data_ptr(), k, ibuf.data_ptr(), zq.data_ptr(), d * hw, hw, 1, ws.data_ptr(),
                               nbytes, lib.stream_ptr())
    assert rc == ERR_ARG


def test_dE_is_bit_reproducible_also_for_a_code_with_many_rows(hip_lib):
    rng = np.random.RandomState(11)
    m, d, k = 20000, 4, 3
    E = np.array([[5.0, 5, 5, 5], [0.1, -0.2, 0.3, 0.0], [-5.0, -5, -5, -5]], dtype=np.float32)
    rows = (0.3 * rng.standard_normal((m, d))).astype(np.float32)
    rows[:40] += 5.0
    idx = V.assign_f64(rows, E)
    assert np.bincount(idx, minlength=k)[1] > 10 ** 4
    gq = rng.standard_normal((m, d)).astype(np.float32)
    runs = [backward(hip_lib, rows, E, idx, gq, 0.7, 1, m, "nhwc", legacy=False)[1] for _ in range(2)]
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    want = V.backward_f64(rows, E, idx, gq, float(np.float32(0.7)), BETA, False)[1]
    tol = (2.0 / (m * d)) * 0.7 * V.dE_bound(rows, E, idx) + 1e-30
    assert (np.abs(runs[0] - want) <= tol).all()
    # and on a spread-out case
    rows, E = V.gaussian_case(3000, 8, 300, seed=12)
    idx = V.assign_f64(rows, E)
    runs = [backward(hip_lib, rows, E, idx, None, 1.0, 3, 1000, "nchw")[1] for _ in range(2)]
    assert np.array_equal(bits(runs[0]), bits(runs[1]))


def test_gather_clamps_out_of_range_indices(hip_lib):
    """The documented rule (include/odvae_hip.h): an index outside [0, K) is clamped to the nearest valid code; E is never read outside"""
    L = hip_lib
    n, hw, d, k = 2, 9, 3, 7
    E = np.arange(k * d, dtype=np.float32).reshape(k, d)
    idx = np.array([0, 6, 7, -1, 2 ** 40, -2 ** 40, 3, 1, 5] * 2, dtype=np.int64)
    ebuf, e = C.padded(torch.tensor(E))
    for layout in ("nchw", "nhwc"):
        sn, sc, sp = strides(layout, d, hw)
        obuf, out = C.out_buf(n * hw * d)
        C.call(L.odvae_vq_gather_f32, torch.tensor(idx, device=DEV).data_ptr(), n, hw, e.data_ptr(), k, d, out.data_ptr(), sn, sc, sp)
        torch.cuda.synchronize()
        C.assert_canary(obuf, ebuf)
        assert np.array_equal(unpack(out.cpu().numpy(), n, hw, d, layout), E[np.clip(idx, 0, k - 1)])


@pytest.mark.parametrize("m,k", [(1, 1), (100, 7), (5000, 300), (70000, 16384)])
def test_usage_counts_and_perplexity(hip_lib, m, k):
    """counts equal numpy.bincount; perplexity: the device sums p log(p + 1e-10) in f64 and rounds exp(-sum) once -- half an ulp, plus the
    two f64 evaluations' difference (about 1e-15 relative, times |sum| <= ln K): 1 f32 ulp is allowed"""
    L = hip_lib
    rng = np.random.RandomState(m)
    idx = np.minimum((rng.exponential(0.2, size=m) * k).astype(np.int64), k - 1)
    cbuf = torch.full((k + C.PAD,), -7, dtype=torch.int32, device=DEV)
    ubuf, u = C.out_buf(2)
    C.call(L.odvae_vq_usage, torch.tensor(idx, device=DEV).data_ptr(), m, k, cbuf.data_ptr(), u.data_ptr())
    torch.cuda.synchronize()
    C.assert_canary(ubuf)
    counts, perplexity, used = V.usage_f64(idx, k)
    assert np.array_equal(cbuf[:k].cpu().numpy(), counts) and (cbuf[k:] == -7).all().item()
    got = u.cpu().numpy()
    print("M=%d K=%d: perplexity %.7g (float64 %.7g, %.2f ulp), used %d" % (m, k, got[0], perplexity, V.ulp_distance(got[0], perplexity), used))
    assert V.ulp_distance(got[0], perplexity) <= 1.0 and got[1] == used


@pytest.mark.parametrize("d,k,n,hw", [(3, 8192, 2, 300), (4, 16384, 1, 257), (8, 16384, 3, 100), (64, 300, 3, 259), (256, 1024, 2, 130), (4, 64, 2, 64)])
def test_gaussian_operands(hip_lib, d, k, n, hw):
    m = n * hw
    rows, E = V.gaussian_case(m, d, k, seed=23, uniform=(k == 64))
    layout = "nhwc" if d % 2 == 0 else "nchw"
    idx, zq, loss = assign(hip_lib, rows, E, n, hw, layout)
    bad, undecided = V.index_violations(rows, E, idx)
    print("D=%d K=%d M=%d: rule violations %d, mismatches against float64 %d, undecided share %.4f"
          % (d, k, m, len(bad), (idx != V.assign_f64(rows, E)).sum(), undecided))
    assert len(bad) == 0
    assert np.array_equal(bits(zq), bits(E[idx]))
    _, want_loss = V.quantize_f64(rows, E, idx, BETA)
    assert abs(loss - want_loss) <= 1.01 * V.U * abs(want_loss)
    rng = np.random.RandomState(d)
    gq = rng.standard_normal(rows.shape).astype(np.float32)
    for legacy in (True, False):
        gl = 1.5
        dz, de = backward(hip_lib, rows, E, idx, gq, gl, n, hw, layout, legacy=legacy)
        want_dz, want_de = V.backward_f64(rows, E, idx, gq, gl, BETA, legacy)
        ce = BETA if legacy else 1.0
        assert (np.abs(dz - want_dz) <= 3 * V.U * (np.abs(gq) + np.abs(want_dz - gq))).all()
        assert (np.abs(de - want_de) <= gl * (2.0 * ce / (m * d)) * V.dE_bound(rows, E, idx) + 1e-38).all()
        assert (de[np.bincount(idx, minlength=k) == 0] == 0).all()


def test_quantize_never_holds_a_distance_matrix(hip_lib):
    """vq-f8 at 256^2, B = 32: M = 32 768 rows against K = 16 384 codes of dimension 4.  The distance matrix alone would be 2 GB; forward and
    backward together may raise the allocator's peak by less than an eighth of it (the operands are about 1 MB)."""
    from odvae_amd import ops
    m_side, k, d = 32, 16384, 4
    g = torch.Generator().manual_seed(1)
    z = torch.randn(32, d, m_side, m_side, generator=g).to(DEV).requires_grad_(True)
    e = torch.randn(k, d, generator=g).to(DEV).requires_grad_(True)
    ops.vq_quantize(z.detach()[:1], e.detach(), BETA)      # (the shared workspace exists before the measurement starts; it grows inside it if it must)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    zq, loss, idx = ops.vq_quantize(z, e, BETA)
    (zq.sum() + loss).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    m = 32 * m_side * m_side
    print("peak rise %.1f MB against the M K 4 / 8 = %.1f MB allowed" % (rise / 2 ** 20, m * k * 4 / 8 / 2 ** 20))
    assert rise < m * k * 4 / 8
    assert idx.shape == (m,) and idx.dtype == torch.int64 and z.grad is not None and e.grad is not None
