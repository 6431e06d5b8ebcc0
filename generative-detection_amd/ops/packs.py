"""Weight packs of the conv kernels and their cache (one pack per weight update, refilled in place)."""
import os
import weakref

import torch

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, _L


class _PackCache:
    """Weight packs keyed by (storage pointer, tensor version, optimizer epoch): a conv's forward and data-gradient packs
    are built together, once per weight update, instead of once per call.  FusedAdam updates parameters from a raw
    kernel (no torch version bump), so it advances `epoch` itself.
    A stale entry is REPACKED INTO ITS OWN BUFFERS (same weight object, same pack kind, hence same sizes): the per-step churn of
    ~180 small allocations and frees kept the caching allocator's small pool fragmenting, and a training step in steady state asked the
    driver for fresh 2 MB segments once or twice (hipMalloc: a device synchronisation -- DESIGN.md 4, the bf16 256x256 side run).
    A graph built before a weight update must not be back-propagated after it: its data-gradient pack now holds the NEW weights
    (torch would raise its "modified by an inplace operation" error there; `check_epoch` raises the same way)."""

    INPLACE = os.environ.get("ODVAE_PACK_INPLACE", "1") != "0"

    def __init__(self):
        self.epoch = 0
        self.generation = 0      # bumps that named no parameters (see bump)
        self._trainable = {}     # id -> weak reference (an id is reused once its tensor is gone: a frozen weight must not inherit it)
        self.store = {}
        self._tables = {}

    def bump(self, stepped=None):
        """Every pack tagged with the epoch is stale from here on.  stepped: the parameters an optimizer step has just written (FusedAdam);
        without it -- a load_state_dict, a broadcast -- any parameter may have changed.  The packs of kind "bf16v" are tagged per weight
        (`weight_tag`): they go stale only when their own weight was stepped, or on a bump that names no parameters."""
        self.epoch += 1
        if stepped is None:
            self.generation += 1
        else:
            for p in stepped:
                p._odvae_steps = getattr(p, "_odvae_steps", 0) + 1

    def weight_tag(self, weight):
        """What identifies the VALUES of this weight: storage, torch's version counter, the optimizer steps that wrote it, unnamed bumps"""
        return (weight.data_ptr(), weight._version, getattr(weight, "_odvae_steps", 0), self.generation)

    def _epoch_of(self, weight):
        """The optimizer epoch a pack of this weight is valid for, or -1 for a weight that has never been trainable while this cache saw it
        (a tensor whose requires_grad is only switched off for a while -- the discriminator during the generator phase -- is still updated
        by its optimizer without a version bump)."""
        if weight.requires_grad:
            seen = self._trainable.get(id(weight))
            if seen is None or seen() is not weight:
                trainable = self._trainable
                self._trainable[id(weight)] = weakref.ref(weight, lambda r, k=id(weight): trainable.pop(k, None) if trainable.get(k) is r else None)
            return self.epoch
        seen = self._trainable.get(id(weight))
        return self.epoch if (seen is not None and seen() is weight) else -1

    def _tag(self, weight, kind="direct"):
        if kind in _PER_WEIGHT_KINDS:      # tagged per weight: the discriminator's packs outlive the generator's optimizer step
            return self.weight_tag(weight)
        # (a frozen weight -- the LPIPS-style VGG stack -- is in no optimizer: its packs do not go stale with the optimizer epoch, only with a
        # write to the tensor itself (load_state_dict: version counter))
        return (weight.data_ptr(), weight._version, self._epoch_of(weight))

    def get(self, weight, want_dgrad, kind="direct"):
        key = (id(weight), kind)
        tag = self._tag(weight, kind)
        hit = self.store.get(key)
        same = hit is not None and hit[0]() is weight
        if same and hit[1] == tag and (hit[3] is not None or not want_dgrad):
            return hit[2], hit[3]
        reuse = None
        if same and self.INPLACE and hit[4] == (tuple(weight.shape), weight.device) and (hit[3] is not None or not want_dgrad):
            if self.BATCH and kind in _BATCH_KINDS and self._refresh_kind(kind, weight.device):
                hit = self.store.get(key)
                if hit is not None and hit[1] == tag:
                    return hit[2], hit[3]
            reuse = (hit[2], hit[3])          # refill the buffers this weight's packs already live in
            want_dgrad = hit[3] is not None
        fwd, dgr = _pack_conv3x3_now(weight, True, want_dgrad, kind, into=reuse)
        # An entry dies with its weight tensor.  AttnBlock builds its [3C, C] q/k/v weight with torch.cat on every forward: each of
        # those temporaries left its two packs behind (round 3 purged dead entries only past 4 096 of them), 14 per step in the bf16
        # path, 6-10 MB that the allocator had to find -- a few fresh hipMalloc calls per step, each a device synchronisation; the
        # f32 path never saw it because its 1x1 convs read the weight as it is.
        store = self.store
        ref = weakref.ref(weight, lambda r, k=key: store.pop(k, None) if (store.get(k) or (None,))[0] is r else None)
        store[key] = (ref, tag, fwd, dgr, (tuple(weight.shape), weight.device))
        return fwd, dgr

    # One launch per pack KIND instead of one per weight: the first stale hit after a weight update refills every stale entry of that
    # kind (the f32 training step repacks 64 Winograd weight packs after every optimizer step: 15-30 us launches, mostly overhead; 234.7 -> 234.4 ms).
    # The device table of (weight, pack, pack, Cout, Cin, taps) records is rebuilt only when the set of entries changes: parameters live
    # in the optimizer's arena and the packs are refilled in place, so the pointers are the same step after step.
    BATCH = os.environ.get("ODVAE_PACK_BATCH", "1") != "0"

    def _refresh_kind(self, kind, device):
        import numpy as np
        L = _L()
        live = []
        for key, ent in self.store.items():
            if key[1] != kind or ent[2] is None:
                continue
            w = ent[0]()
            if w is None or w.device != device or ent[4] != (tuple(w.shape), w.device) or not w.is_contiguous() or w.dtype != torch.float32:
                continue
            tag = self._tag(w)
            if ent[1] == tag or not _batchable(kind, w, L):
                continue
            live.append((key, ent, w, tag))
        if len(live) < 2:
            return False
        sig = tuple((k, e[2].data_ptr(), 0 if e[3] is None else e[3].data_ptr(), w.data_ptr()) for k, e, w, _ in live)
        cached = self._tables.get((kind, device))
        if cached is None or cached[0] != sig:
            rec = np.zeros(len(live), dtype=np.dtype([("w", "<u8"), ("fwd", "<u8"), ("dgr", "<u8"), ("cout", "<i4"), ("cin", "<i4"), ("taps", "<i4"), ("pad", "<i4")]))
            for i, (_, e, w, _) in enumerate(live):
                rec[i] = (w.data_ptr(), e[2].data_ptr(), 0 if e[3] is None else e[3].data_ptr(), w.shape[0], w.shape[1], w.shape[2] * w.shape[3], 0)
            table = _lib.upload(torch.from_numpy(rec.view(np.uint8).copy()), device)
            cached = self._tables[(kind, device)] = (sig, table)
        fn = {"wino": L.odvae_conv3x3_pack_wino_batch, "wino4": L.odvae_conv3x3_pack_wino4_batch}[kind]
        _lib.check(fn(cached[1].data_ptr(), len(live), _lib.stream_ptr()), "pack batch (%s)" % kind)
        for key, e, w, tag in live:
            self.store[key] = (e[0], tag, e[2], e[3], e[4])
        return True

    def check_epoch(self, epoch, what):
        if epoch != self.epoch:
            raise RuntimeError("%s: the weights were updated (optimizer step) between this graph's forward and its backward; the "
                               "cached weight packs now hold the new weights" % what)


_PER_WEIGHT_KINDS = ("bf16v", "c4x4s1", "c4x4s2")      # the PatchGAN's packs: bf16, and the f32 16-tap packs of a stride-1 / stride-2 conv
_BATCH_KINDS = ("wino", "wino4")      # (bf16 packs: batching measured 0.3-0.65 ms per step slower, see conv_bf16.hip)


def _batchable(kind, w, L):
    """Shapes the batched pack kernels take: the Winograd packs without padding in either direction (the single-weight launcher zero-fills
    padding with a memset first)."""
    cout, cin = w.shape[0], w.shape[1]
    if tuple(w.shape[2:]) != (3, 3):
        return False
    rp, op = ((L.odvae_conv3x3_wino_reduce_pad, L.odvae_conv3x3_wino_out_pad) if kind == "wino"
              else (L.odvae_conv3x3_wino4_reduce_pad, L.odvae_conv3x3_wino4_out_pad))
    return rp(cin) == cin and op(cout) == cout and rp(cout) == cout and op(cin) == cin


PACK_CACHE = _PackCache()


def _pack_conv3x3_now(weight, want_fwd=True, want_dgrad=False, kind="direct", into=None):
    """kind: "direct" (conv3x3_f32.hip, modes 0-3); "up": the 16-tap packs of an Upsample conv (taps that hit the same low-res pixel
    pre-summed, modes 5 / 6); "wino" / "wino4": the Winograd F(2x2,3x3) / F(4x4,3x3) packs U = G g G^T of a stride-1 conv
    (conv3x3_wino_f32.hip, conv3x3_wino4_f32.hip); "bf16": see below.
    into=(fwd, dgr): refill these pack tensors (of the same weight and kind) instead of allocating."""
    L = _L()
    ifwd, idgr = into if into is not None else (None, None)
    w = weight.detach().contiguous()
    _lib.require_device(w)
    cout, cin = w.shape[0], w.shape[1]
    if kind in ("bf16", "bf16v"):   # bf16 MFMA-fragment packs of a 3x3, 1x1 or 4x4 conv (conv_bf16.hip); master weights stay f32; "bf16v": tagged per weight
        taps = w.shape[2] * w.shape[3]
        fwd = (ifwd if ifwd is not None else torch.empty(L.odvae_conv_bf16_pack_elems(cin, cout, taps), dtype=BF16, device=w.device)) if want_fwd else None
        dgr = (idgr if idgr is not None else torch.empty(L.odvae_conv_bf16_pack_elems(cout, cin, taps), dtype=BF16, device=w.device)) if want_dgrad else None
        _lib.check(L.odvae_conv_pack_bf16(w.data_ptr(), cout, cin, taps, _lib.ptr(fwd), _lib.ptr(dgr), _lib.stream_ptr()), "conv_pack_bf16")
        return fwd, dgr
    if kind in ("c4x4s1", "c4x4s2"):   # f32 16-tap packs of Conv2d(k=4, pad=1) (odvae_conv4x4_f32); the data-gradient pack's order depends on the stride
        fwd = (ifwd if ifwd is not None else torch.empty(L.odvae_conv4x4_pack_floats(cin, cout), dtype=torch.float32, device=w.device)) if want_fwd else None
        dgr = (idgr if idgr is not None else torch.empty(L.odvae_conv4x4_pack_floats(cout, cin), dtype=torch.float32, device=w.device)) if want_dgrad else None
        _lib.check(L.odvae_conv4x4_pack_f32(w.data_ptr(), cout, cin, int(kind[-1]), _lib.ptr(fwd), _lib.ptr(dgr), _lib.stream_ptr()), "conv4x4_pack")
        return fwd, dgr
    floats, pack = {"direct": (L.odvae_conv3x3_pack_floats, L.odvae_conv3x3_pack_f32),
                    "up": (L.odvae_conv3x3_up_pack_floats, L.odvae_conv3x3_pack_up_f32),
                    "wino": (L.odvae_conv3x3_wino_pack_floats, L.odvae_conv3x3_pack_wino_f32),
                    "wino4": (L.odvae_conv3x3_wino4_pack_floats, L.odvae_conv3x3_pack_wino4_f32)}[kind]
    fwd = dgr = None
    if want_fwd:
        fwd = ifwd if ifwd is not None else torch.empty(floats(cin, cout), dtype=torch.float32, device=w.device)
    if want_dgrad:
        dgr = idgr if idgr is not None else torch.empty(floats(cout, cin), dtype=torch.float32, device=w.device)
    _lib.check(pack(w.data_ptr(), cout, cin, _lib.ptr(fwd), _lib.ptr(dgr), _lib.stream_ptr()), "conv3x3_pack")
    return fwd, dgr


def pack_conv3x3(weight, want_fwd=True, want_dgrad=False, kind="direct"):
    """OIHW parameter -> kernel packs of one kind (_pack_conv3x3_now), cached per weight update."""
    fwd, dgr = _ops.PACK_CACHE.get(weight, want_dgrad, kind)
    return (fwd if want_fwd else None), (dgr if want_dgrad else None)
