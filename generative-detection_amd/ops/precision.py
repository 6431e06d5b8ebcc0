"""float32_matmul_precision: how many bf16 planes of each f32 operand the bf16-split GEMM (gemm_f32_split.hip) multiplies.

The reference's launcher calls torch.set_float32_matmul_precision('medium') (train.py:521); in its model that setting governs the
torch.bmm products of AttnBlock and the pose head's nn.Linear layers.  Here it governs every launch of the split kernel: the six
attention products where their gates open, and a 1x1 convolution's weight gradient where the GEMM sends it there (1 024 pixels; deeper
ones run split-K on the f32 kernel.  In the reference that product falls under cuDNN's TF32 allowance, on by default).  The pose head's dense layers stay on linear_f32.hip in exact f32 at every
level: they are under 0.1 % of the work.  The gates do not move with the level: a product on the f32 MFMA kernel stays there.

    highest (default)   hi + mid + lo, six products     within 2^-22 of sum |a| |b| of the f32 kernel
    high                hi + mid, three products        within 2^-14
    medium              hi, one product                 within 2^-6   (bf16 operands, f32 accumulation)
    torch               follow torch.get_float32_matmul_precision() at call time

The setting is FLOAT32_MATMUL_PRECISION in the switch table of ops/__init__.py; the library holds a process-global level
(odvae_gemm_select_precision), and `_sync_precision` pushes it there when it differs from what was pushed last."""
import torch

from .. import ops as _ops      # the package: the setting and the pushed level live in its table (ops/__init__.py)
from .. import lib as _lib

MATMUL_PRECISION_LEVELS = {"highest": 0, "high": 1, "medium": 2}      # name -> level of odvae_gemm_select_precision
MATMUL_PRECISION_VALUES = tuple(MATMUL_PRECISION_LEVELS) + ("torch",)


def _parse_matmul_precision(value):
    """A value of ODVAE_FLOAT32_MATMUL_PRECISION / set_float32_matmul_precision: one of MATMUL_PRECISION_VALUES (case and
    surrounding blanks ignored).  Anything else raises ValueError."""
    name = value.strip().lower() if isinstance(value, str) else None
    if name not in MATMUL_PRECISION_VALUES:
        raise ValueError("float32_matmul_precision must be one of %s, got %r" % (", ".join(MATMUL_PRECISION_VALUES), value))
    return name


def _matmul_level():
    """The level the current setting asks for (0..2); in `torch` mode from torch's own setting, read now."""
    mode = _ops.FLOAT32_MATMUL_PRECISION
    return MATMUL_PRECISION_LEVELS[torch.get_float32_matmul_precision() if mode == "torch" else mode]


def _sync_precision(L):
    """Called in front of every launch that may reach the split kernel: one compare; the library is told only where the level changes."""
    level = _matmul_level()
    if level != _ops._MATMUL_LEVEL_PUSHED:
        L.odvae_gemm_select_precision(level)
        _ops._MATMUL_LEVEL_PUSHED = level


def set_float32_matmul_precision(name):
    """highest | high | medium | torch (module docstring).  Process-global, like torch's.  A bad value raises ValueError and changes
    nothing.  Takes effect at once when the library is loaded, else at the first launch."""
    _ops.FLOAT32_MATMUL_PRECISION = _parse_matmul_precision(name)
    if _lib._lib is not None:
        _sync_precision(_lib._lib)


def get_float32_matmul_precision():
    """The setting as it was given: highest, high, medium or torch."""
    return _ops.FLOAT32_MATMUL_PRECISION
