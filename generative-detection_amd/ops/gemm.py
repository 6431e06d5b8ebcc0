"""The f32 GEMM and the column sum (gemm_f32.hip): used by the 1x1 convs, attention, the PatchGAN convs and the pose MLPs."""
import torch

from .. import lib as _lib
from ._base import KERNEL_EVENTS, _L, _ws
from .precision import _sync_precision


# ------------------------------------------------------------------------------------------------------
# GEMM-backed ops
# ------------------------------------------------------------------------------------------------------
def gemm(ta, tb, m, n, k, alpha, a, lda, sa, b, ldb, sb, c, ldc, sc, bias=None, residual=None, batch=1):
    """Raw batched GEMM on device pointers held by tensors a, b, c (see gemm_f32.hip)."""
    L = _L()
    _sync_precision(L)      # float32_matmul_precision: deep plain products run on the bf16-split kernel
    need = L.odvae_gemm_f32_workspace_bytes(m, n, k, batch)
    wp, wn = _ws(need, c) if need else (None, 0)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_gemm_f32(int(ta), int(tb), m, n, k, float(alpha), a.data_ptr(), lda, sa, b.data_ptr(), ldb, sb,
                                c.data_ptr(), ldc, sc, _lib.ptr(bias), _lib.ptr(residual), batch, wp, wn,
                                _lib.stream_ptr()), "gemm_f32")
    KERNEL_EVENTS.end("gemm_f32", 2.0 * m * n * k * batch, tag, 4.0 * batch * (m * k + k * n + m * n))


def _colsum(x2d_ptr_tensor, rows, c):
    L = _L()
    out = torch.empty(c, dtype=torch.float32, device=x2d_ptr_tensor.device)
    need = L.odvae_colsum_workspace_bytes(rows, c)
    wp, wn = _ws(need, out)
    _lib.check(L.odvae_colsum_f32(x2d_ptr_tensor.data_ptr(), rows, c, out.data_ptr(), wp, wn, _lib.stream_ptr()), "colsum")
    return out
