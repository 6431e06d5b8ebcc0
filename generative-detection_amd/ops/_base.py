"""What every kernel family starts from: the library handle, NHWC views, workspace, tensor stamps, the HIP-event timer."""
import torch

from .. import lib as _lib


CL = torch.channels_last


def _L():
    return _lib.load()


BF16 = torch.bfloat16


def _cl(t, dtype=torch.float32):
    """NHWC-in-memory view of a logical NCHW tensor (copy only if the caller handed us another layout)."""
    _lib.require_device(t, dtypes=(dtype,))
    if t.dim() != 4:
        raise ValueError("expected a 4-d NCHW tensor, got shape %s" % (tuple(t.shape),))
    n, c, h, w = t.shape
    if t.stride() == (h * w * c, 1, w * c, c):
        return t
    out = torch.empty((n, c, h, w), dtype=t.dtype, device=t.device, memory_format=CL)
    out.copy_(t)
    if out.stride() != (h * w * c, 1, w * c, c):  # degenerate sizes: force the canonical NHWC strides
        out = out.as_strided((n, c, h, w), (h * w * c, 1, w * c, c))
    return out


def _new_cl(n, c, h, w, like, dtype=torch.float32):
    t = torch.empty((n, h, w, c), dtype=dtype, device=like.device)
    return t.permute(0, 3, 1, 2)


def _ws(nbytes, like):
    return _lib.workspace.get(nbytes, like.device)


def _stamp(t):
    """What identifies "this tensor, as it is now" for a result derived from its values: storage, version counter, shape.  Anything that
    writes to the tensor in between (an in-place op, a hook, a checkpoint wrapper's copy) changes it."""
    return (t.data_ptr(), t._version, tuple(t.shape))


def _stamped(t, stamp):
    """Is `t` still the tensor `stamp` was taken from?"""
    return stamp == _stamp(t)


class _KernelEvents:
    """HIP-event brackets around individual kernel launches on torch's current stream (bench.py's live roofline).
    Off by default; when on, every launch of a tagged kernel records (algorithmic flops, start, stop)."""

    def __init__(self):
        self.on = False
        self.extra = False    # also bracket the secondary kernel families (bench.py: one extra step after the timed region)
        self.rec = {}
        self.issued = 0.0
        self.sample, self._n = 1, 0

    def enable(self):
        self.on, self.rec, self.issued = True, {}, 0.0

    def count(self, issued_flops):
        """Multiply-add work actually issued to the MFMA pipe by one launch (Winograd: 16/36 of the direct form); host
        arithmetic only, summed over the timed steps for bench.py's whole-step MFMA fraction."""
        if self.on:
            self.issued += issued_flops

    def disable(self):
        self.on = False

    def begin(self, secondary=False):
        if not self.on or (secondary and not self.extra):
            return None
        if not secondary and self.sample > 1:   # bracket one launch in `sample` of the dominant family (see bench.py)
            self._n += 1
            if self._n % self.sample:
                return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, name, flops, ev0, nbytes=0.0, issued=None, variant=None):
        """flops = ALGORITHMIC work of the launch (direct form); issued = multiply-add work actually sent to the MFMA pipe
        (defaults to flops).  variant: which instantiation of the family's kernel ran (its epilogue); the same record is then also
        listed under "name|variant" (summary("name|variant"), variants(name)): the family figure aggregates kernels that do different
        amounts of non-matrix work per launch."""
        if self.on:
            self.issued += flops if issued is None else issued
        if ev0 is None:
            return
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        item = (flops, ev0, ev1, nbytes, flops if issued is None else issued)
        self.rec.setdefault(name, []).append(item)
        if variant is not None:
            self.rec.setdefault(name + "|" + variant, []).append(item)

    def variants(self, name):
        return sorted(k.split("|", 1)[1] for k in self.rec if k.startswith(name + "|"))

    def summary(self, name):
        torch.cuda.synchronize()
        items = self.rec.get(name, [])
        if not items:
            return None
        total_ms = sum(it[1].elapsed_time(it[2]) for it in items)
        flops = sum(it[0] for it in items)
        nbytes = sum(it[3] for it in items)
        issued = sum(it[4] for it in items)
        return {"launches": len(items), "total_ms": total_ms, "avg_ms": total_ms / len(items),
                "gflop_per_launch": flops / len(items) / 1e9, "tflops": flops / total_ms / 1e9,
                "issued_gflop_per_launch": issued / len(items) / 1e9, "issued_tflops": issued / total_ms / 1e9,
                "bytes_per_launch": nbytes / len(items), "tbytes_per_s": nbytes / total_ms / 1e9}


KERNEL_EVENTS = _KernelEvents()
