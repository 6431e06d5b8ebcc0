"""Inputs, float64 references and the acceptance rule for the vector quantiser (csrc/vq_f32.hip); tests/test_vq_inputs.py holds them to
torch's f32 evaluation of upstream's expression and to planted faults, the GPU tests compare the kernels against them.

Rows are the positions of a [N, D, H, W] tensor taken as z[M, D] (M = N H W); E is the codebook [K, D].

    s_k = |e_k|^2 - 2 z . e_k        idx = argmin_k s_k, `s < best` from (+inf, 0): lowest k on ties, 0 for a row that holds NaN
    loss = (1 + beta) sum (z_q - z)^2 / (M D)
    dz = g_q + g_l (2 c_z / (M D)) (z - z_q)        dE[k] = g_l (2 c_e / (M D)) sum_{idx = k} (e_k - z_row)
    legacy: c_z = 1, c_e = beta; otherwise c_z = beta, c_e = 1

The rule for indices.  In f32 a score is D products summed in some order (fused or not), the same for |e_k|^2, and one subtraction: at
most n = D + 2 roundings on any path from an input to the score, so |s_f32 - s| <= gamma_n (|e_k|^2 + 2 sum_i |z_i e_ki|) with
gamma_n = n u / (1 - n u), u = 2^-24, whatever the order.  bound_row is the largest such bound over the codes of a row; an index passes
iff its exact score is within 2 bound_row of the best exact score.  A row whose best-to-second gap exceeds that must match exactly.
"""
import numpy as np

U = 2.0 ** -24
FAULTS = ["tie_highest", "no_norm", "skip_last", "skip_chunk_edge", "beta_wrong_term", "dE_no_2", "dE_with_gq", "dz_no_st", "loss_div_M"]
CHUNK = 64      # codes per LDS chunk of the search kernel (ops.vq_plan(...)["chunk"]; the GPU test checks that it still is)


def gamma(n):
    return n * U / (1.0 - n * U)


def scores_f64(z, E):
    z, E = np.asarray(z, dtype=np.float64), np.asarray(E, dtype=np.float64)
    return (E * E).sum(1)[None, :] - 2.0 * z @ E.T


def row_bound(z, E):
    z, E = np.asarray(z, dtype=np.float64), np.asarray(E, dtype=np.float64)
    mag = (E * E).sum(1)[None, :] + 2.0 * np.abs(z) @ np.abs(E).T
    with np.errstate(invalid="ignore"):
        return gamma(z.shape[1] + 2) * np.nanmax(np.where(np.isfinite(mag), mag, np.nan), axis=1, initial=0.0)


def assign_f64(z, E, fault=None):
    """argmin under the `s < best` rule in float64; NaN scores never win, a row with no score below +inf gets 0"""
    s = scores_f64(z, E)
    if fault == "no_norm":
        s = -2.0 * np.asarray(z, dtype=np.float64) @ np.asarray(E, dtype=np.float64).T
    s = np.where(np.isnan(s), np.inf, s)
    if fault == "skip_last":
        s[:, -1] = np.inf
    if fault == "skip_chunk_edge" and s.shape[1] > CHUNK:
        s[:, CHUNK] = np.inf
    if fault == "tie_highest":
        k = s.shape[1]
        return (k - 1 - np.argmin(s[:, ::-1], axis=1)).astype(np.int64)
    return np.argmin(s, axis=1).astype(np.int64)


def index_violations(z, E, idx):
    """(rows that break the rule, share of rows whose best-to-second gap is within 2 bound_row); rows holding NaN or inf must be 0 /
    in range and are judged by the caller"""
    s = scores_f64(z, E)
    idx = np.asarray(idx)
    ok_range = (idx >= 0) & (idx < E.shape[0])
    b = row_bound(z, E)
    best = s.min(axis=1)
    got = s[np.arange(len(idx)), np.clip(idx, 0, E.shape[0] - 1)]
    bad = ~ok_range | ~(got <= best + 2.0 * b)
    if s.shape[1] > 1:
        srt = np.partition(s, 1, axis=1)
        undecided = float(((srt[:, 1] - srt[:, 0]) <= 2.0 * b).mean())
    else:
        undecided = 0.0
    return np.nonzero(bad)[0], undecided


def quantize_f64(z, E, idx, beta, fault=None):
    z, E = np.asarray(z, dtype=np.float64), np.asarray(E, dtype=np.float64)
    zq = E[idx]
    m, d = z.shape
    denom = m if fault == "loss_div_M" else m * d
    return zq, (1.0 + float(beta)) * ((zq - z) ** 2).sum() / denom


def backward_f64(z, E, idx, gq, gl, beta, legacy, fault=None):
    """(dz [M, D], dE [K, D]) in float64, in the order of operations of the kernel (coef = gl * scale first)"""
    z, E = np.asarray(z, dtype=np.float64), np.asarray(E, dtype=np.float64)
    m, d = z.shape
    gq = np.zeros_like(z) if gq is None else np.asarray(gq, dtype=np.float64)
    beta = float(np.float32(beta))
    cz, ce = (1.0, beta) if legacy else (beta, 1.0)
    if fault == "beta_wrong_term":
        cz, ce = ce, cz
    md = float(m) * float(d)
    two_e = 1.0 if fault == "dE_no_2" else 2.0
    zq = E[idx]
    dz = (0.0 if fault == "dz_no_st" else gq) + (float(gl) * (2.0 * cz / md)) * (z - zq)
    dE = np.zeros_like(E)
    np.add.at(dE, idx, zq - z)
    dE = (float(gl) * (two_e * ce / md)) * dE
    if fault == "dE_with_gq":
        np.add.at(dE, idx, gq)
    return dz, dE


def dE_bound(z, E, idx):
    """gamma_{c_k + 3} sum |terms| per code: the f32-rounding budget the issue grants dE[k] before its scale"""
    z, E = np.asarray(z, dtype=np.float64), np.asarray(E, dtype=np.float64)
    mag = np.zeros_like(E)
    np.add.at(mag, idx, np.abs(E[idx] - z))
    counts = np.bincount(idx, minlength=E.shape[0]).astype(np.float64)
    return gamma(counts + 3.0)[:, None] * mag


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def exact_case(m, d, k, seed):
    """z [M, D], E [K, D] of whole numbers in [-8, 8] as f32: every product, every partial sum of a score (|s| <= 192 D < 2^24) and every
    difference e - z is exact in f32 in any order"""
    rng = np.random.RandomState(seed)
    z = rng.randint(-8, 9, size=(m, d)).astype(np.float32)
    E = rng.randint(-8, 9, size=(k, d)).astype(np.float32)
    assert 192 * d < 2 ** 24
    return z, E


def gaussian_case(m, d, k, seed, uniform=False):
    rng = np.random.RandomState(seed)
    if uniform:
        return (rng.uniform(-1.0 / k, 1.0 / k, size=(m, d)).astype(np.float32), rng.uniform(-1.0 / k, 1.0 / k, size=(k, d)).astype(np.float32))
    return rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((k, d)).astype(np.float32)


def plant_winner(z, E, row, code, dup=None):
    """make `code` the exact nearest code of `row` (its row of E becomes the row of z, distance 0, unique unless `dup` names a second code
    that gets the same row): the winner sits where the caller aims it"""
    E[code] = z[row]
    same = np.nonzero((E == z[row]).all(axis=1))[0]
    for j in same:
        if j != code and j != dup:
            E[j, 0] = E[j, 0] + (1.0 if E[j, 0] < 8 else -1.0)
    if dup is not None:
        E[dup] = z[row]
    return E


def to_nchw(rows, n, hw):
    """[M, D] rows -> [N, D, HW] (the NCHW tensor with H W flattened)"""
    m, d = rows.shape
    return np.ascontiguousarray(rows.reshape(n, hw, d).transpose(0, 2, 1))


def from_nchw(t):
    n, d, hw = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(n * hw, d)


def ulp_distance(got, ref64):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref64), 2.0 ** -126))) - 23)
    return np.where(np.isfinite(got), np.abs(got - ref64) / ulp, np.inf)


def usage_f64(idx, k):
    counts = np.bincount(np.asarray(idx), minlength=k)
    p = counts.astype(np.float64) / float(len(idx))
    return counts, float(np.exp(-(p * np.log(p + 1e-10)).sum())), int((counts > 0).sum())
