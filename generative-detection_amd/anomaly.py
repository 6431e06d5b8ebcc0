"""Anomaly detection for backward passes with the semantics of `torch.autograd.set_detect_anomaly(True)` -- what the reference's
`lightning.trainer.detect_anomaly: True` (yaml:138) switches on under PL 1.9 -- at a cost small enough to leave on.

torch's mode runs `isnan(output).any().item()` on every output of every backward node as it finishes: one host synchronisation
per output, ATen kernels on the product path and a traceback recorded per forward op.  Here:

- `watch(roots)` walks the autograd graph from `roots` and registers one post-hook on every node not seen in this optimizer phase;
- each firing of a hook takes the next sequence number (execution order; a node that runs twice under retain_graph=True gets two)
  and launches `anomaly_scan_kernel` (csrc/anomaly.hip) over the node's floating outputs, up to 8 per launch; the kernel keeps
  min((seq << 20) | output_index) over everything it flags in a one-word device record;
- the host keeps seq -> (node name, innermost nn.Module whose forward built the node) for the phase;
- `Detector.check()` waits once per optimizer phase for that word (a pinned copy and an event) after the backward, and the trainer
  raises `AnomalyError` before gradient clipping and the optimizer step.

So the first node torch would name, and its lowest offending output index, is what this reports -- one host wait per optimizer step
instead of one per node output.  Dense outputs of any stride order (the channels-last tensors of ops._new_cl included) are scanned in
place; anything else (non-dense views, dtypes other than f32 / bf16, host tensors) takes a small fallback that never synchronises the
device and is counted in `Detector.fallbacks`.  With the mode off none of this exists: no hook, no launch, no wait.
"""
import ctypes
import functools
import os
import time

import torch

from . import lib as _lib

CLEAN = (1 << 63) - 1         # ODVAE_ANOMALY_CLEAN: the record of a phase in which nothing was flagged
MAX_PER_LAUNCH = 8
MODES = {"nan": 0, "nonfinite": 1}
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


class AnomalyError(RuntimeError):
    """A backward node returned NaN (or, in "nonfinite" mode, NaN / Inf) values.  The message starts with torch's own sentence;
    `node`, `output_index`, `module`, `optimizer_idx`, `global_step` and `rank` carry the details."""

    def __init__(self, message, node=None, output_index=None, module=None, optimizer_idx=None, global_step=None, rank=None):
        super().__init__(message)
        self.node, self.output_index, self.module = node, output_index, module
        self.optimizer_idx, self.global_step, self.rank = optimizer_idx, global_step, rank


class _TensorDesc(ctypes.Structure):
    """OdvaeAnomalyTensor of include/odvae_hip.h."""
    _fields_ = [("ptr", ctypes.c_void_p), ("numel", ctypes.c_int64), ("dtype", ctypes.c_int32), ("output_index", ctypes.c_int32)]


def parse_mode(value):
    """Trainer(detect_anomaly=...) -> None (off), "nan" or "nonfinite".  False / True (= "nan", torch's semantics) / "nan" /
    "nonfinite"; None reads ODVAE_DETECT_ANOMALY (unset or 0 = off, 1 = nan, nonfinite)."""
    if value is None:
        value = os.environ.get("ODVAE_DETECT_ANOMALY", "")
    if isinstance(value, bool):
        return "nan" if value else None
    if isinstance(value, int):
        if value in (0, 1):
            return "nan" if value else None
        raise ValueError("detect_anomaly: %r (expected False, True, 'nan' or 'nonfinite')" % (value,))
    v = str(value).strip().lower()
    if v in ("", "0", "false", "off", "none"):
        return None
    if v in ("1", "true", "on", "nan"):
        return "nan"
    if v == "nonfinite":
        return "nonfinite"
    raise ValueError("detect_anomaly: %r (expected False, True, 'nan' or 'nonfinite')" % (value,))


def _tensors(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors(o)


def dense(t):
    """True when t's elements fill exactly numel() consecutive slots from data_ptr() (any stride order: at::is_non_overlapping_and_dense,
    which Python does not expose)."""
    if t.is_contiguous():
        return True
    expected = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if stride != expected:
            return False
        expected *= size
    return True


class _Record:
    """One device word (int64, read as unsigned by the kernel), its pinned host copy and the event that orders the two.
    Allocated once per device: no allocation in steady state."""

    def __init__(self, device):
        self.dev = torch.empty(1, dtype=torch.int64, device=device)
        self.host = torch.empty(1, dtype=torch.int64, pin_memory=True)
        self.event = torch.cuda.Event()


_records = {}


def record_for(device):
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    r = _records.get(key)
    if r is None:
        r = _records[key] = _Record(torch.device("cuda", key))
    return r


def reset(record):
    """Sets the device word to CLEAN on the current stream."""
    _lib.check(_lib.load().odvae_anomaly_reset(record.data_ptr(), _lib.stream_ptr()), "anomaly_reset")


def scan(items, seq, mode, record):
    """items: [(tensor, output_index)] of dense f32 / bf16 device tensors; one launch per 8."""
    L = _lib.load()
    code = MODES[mode]
    for s in range(0, len(items), MAX_PER_LAUNCH):
        chunk = items[s:s + MAX_PER_LAUNCH]
        descs = (_TensorDesc * len(chunk))(*[_TensorDesc(t.data_ptr(), t.numel(), _DTYPES[t.dtype], i) for t, i in chunk])
        _lib.check(L.odvae_anomaly_scan(descs, len(chunk), seq, code, record.data_ptr(), _lib.stream_ptr()), "anomaly_scan")


_active = None      # the Detector of the optimizer phase in progress, if any


def watch(roots):
    """Watch every backward node reachable from `roots` (tensors or nested lists of them) in the current phase; a no-op when anomaly
    mode is off.  PoseLoss calls it before its torch.autograd.grad passes, the trainer before the main backward."""
    d = _active
    if d is not None:
        d.watch(roots)


class Detector:
    """The per-trainer state: module tags, the hooks' sequence numbers and the seq -> node table of the current optimizer phase."""

    def __init__(self, mode, model=None):
        if mode not in MODES:
            raise ValueError("anomaly mode %r (expected one of %s)" % (mode, sorted(MODES)))
        self.mode = mode
        self.active = False
        self.gen = 0                # phase counter: hooks of an earlier phase (a graph kept alive) do nothing
        self.seq = 0
        self.table = {}             # seq -> (node name, module name or None)
        self.seen = {}              # node -> True: nodes of this phase that carry a hook (held until the phase ends)
        self.tags = {}              # node -> name of the innermost module whose forward created it (this phase)
        self.host_key = CLEAN       # findings on host tensors (fallback)
        self.fallbacks = 0          # outputs that were not scanned in place
        self.hook_seconds = 0.0     # host time spent in the hooks
        self.bytes_scanned = 0      # bytes handed to the scan kernel (from the shapes)
        self.last_watched = 0       # nodes watched in the last phase
        self.record = None
        self._module_hooks = []
        if model is not None:
            for name, m in model.named_modules():
                self._module_hooks.append(m.register_forward_hook(functools.partial(self._tag, name or type(m).__name__)))

    def remove(self):
        for h in self._module_hooks:
            h.remove()
        self._module_hooks = []

    # ---- module tags: forward hooks, innermost module first (its hook fires before its parent's) ------------------------------
    def _tag(self, name, module, args, output):
        if not self.active or torch._C._current_graph_task_id() != -1:     # no tags for recomputations inside a backward
            return
        stop = {t.grad_fn for t in _tensors(args) if t.grad_fn is not None}
        stack = [t.grad_fn for t in _tensors(output) if t.grad_fn is not None]
        tags = self.tags
        while stack:
            node = stack.pop()
            if node is None or node in tags or node in stop:
                continue
            nf = node.next_functions
            if not nf:              # AccumulateGrad: no outputs, outlives the phase
                continue
            tags[node] = name
            stack.extend(f for f, _ in nf)

    # ---- one optimizer phase ---------------------------------------------------------------------------------------------------
    def begin(self, device):
        """Start a phase: reset the device record (current stream) and the host table."""
        global _active
        self.record = record_for(device)
        reset(self.record.dev)
        self.gen += 1
        self.seq = 0
        self.table.clear()
        self.seen.clear()
        self.tags.clear()
        self.host_key = CLEAN
        self.active = True
        _active = self

    def end(self):
        """Leave the phase: drop every reference to the phase's graph."""
        global _active
        self.active = False
        if _active is self:
            _active = None
        if self.seen:
            self.last_watched = len(self.seen)
        self.seen.clear()
        self.tags.clear()

    def watch(self, roots):
        if not self.active:
            return
        seen, tags, gen = self.seen, self.tags, self.gen
        stack = [t.grad_fn for t in _tensors(roots) if t.grad_fn is not None]
        while stack:
            node = stack.pop()
            if node is None or node in seen:
                continue
            seen[node] = True
            nf = node.next_functions
            if not nf:
                continue
            # the hook holds names only, never the node: a node -> hook -> node cycle would keep the graph alive
            node.register_hook(functools.partial(self._fire, gen, node.name(), tags.get(node)))
            stack.extend(f for f, _ in nf)

    def _fire(self, gen, name, module, grad_inputs, grad_outputs):
        if gen != self.gen or not self.active:
            return
        t0 = time.perf_counter()
        seq = self.seq
        self.seq += 1
        self.table[seq] = (name, module)
        items = []
        for i, g in enumerate(grad_inputs):
            if g is None or not (g.is_floating_point() or g.is_complex()) or g.numel() == 0:
                continue
            if g.is_cuda and g.dtype in _DTYPES:
                if 0 in g.stride():         # a broadcast gradient (SumBackward, MeanBackward): its distinct elements are what counts
                    g = g.as_strided([1 if st == 0 else sz for sz, st in zip(g.shape, g.stride())], g.stride())
                if dense(g):
                    items.append((g, i))
                    continue
            self.fallbacks += 1
            if not g.is_cuda:                       # a host tensor: checked on the host, no device involved
                bad = torch.isnan(g) if self.mode == "nan" else ~torch.isfinite(g)
                if bool(bad.any()):
                    self.host_key = min(self.host_key, (seq << 20) | i)
                continue
            bad = (torch.isnan(g) if self.mode == "nan" else ~torch.isfinite(g)).any()
            items.append((torch.where(bad, float("nan"), 0.0).to(device=g.device, dtype=torch.float32).reshape(1), i))
        if items:
            self.bytes_scanned += sum(t.numel() * t.element_size() for t, _ in items)
            scan(items, seq, self.mode, self.record.dev)
        self.hook_seconds += time.perf_counter() - t0

    def check(self, group=None):
        """Wait for the phase's record (after an all-reduce MIN over `group` when given) and return None or
        (node name, output index, module name) of the earliest flagged output."""
        rec = self.record
        if self.host_key != CLEAN:
            rec.dev.clamp_(max=self.host_key)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(rec.dev, op=dist.ReduceOp.MIN, group=group)
        rec.host.copy_(rec.dev, non_blocking=True)
        rec.event.record()
        rec.event.synchronize()
        key = int(rec.host[0])
        if key == CLEAN:
            return None
        seq, index = key >> 20, key & 0xFFFFF
        name, module = self.table.get(seq, ("<unknown node #%d>" % seq, None))
        return name, index, module

    def stats(self):
        """Hook firings and watched nodes of the current / last phase, fallbacks and host hook time so far."""
        return {"firings": self.seq, "watched": len(self.seen) or self.last_watched, "fallbacks": self.fallbacks, "hook_seconds": self.hook_seconds,
                "bytes_scanned": self.bytes_scanned}

    def message(self, name, index, module):
        what = "nan" if self.mode == "nan" else "nan or inf"
        return "Function '%s' returned %s values in its %dth output." % (name, what, index) + \
            (" It was created in the forward of module '%s'." % module if module else " It was created outside any module's forward.")
