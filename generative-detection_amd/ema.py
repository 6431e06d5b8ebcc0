"""Exponential moving average of the trainable weights: [UPSTREAM] ldm.modules.ema.LitEma on the flat arenas of optim.FusedAdam.

Buffers, names and arithmetic are upstream's (a checkpoint's `model_ema.*` keys load here and the reverse):
  decay        f32 scalar
  num_updates  int32 scalar, 0 at the start; -1 with use_num_upates=False (the misspelt keyword is upstream's)
  one buffer per parameter that requires a gradient at construction, named by the parameter's name without its dots, a clone of it
One update (forward): num_updates += 1; d = min(decay, (1 + num_updates) / (10 + num_updates)) in f32; every shadow s of a parameter p
becomes s - (1 - d) * (s - p) by three separately rounded f32 operations.

Upstream walks named_parameters() from Python (three small kernels per parameter) and reads the counter on the host.  Here the counter
and the schedule stay on the device (ops.ema_tick) and, once `materialize` has laid the shadows out like the optimizers' parameter
arenas, an update is one tick, one streaming launch per arena (ops.ema_update) and one per parameter that lives in no arena.  `swap`
exchanges parameters and shadows in one pass per arena (ops.ema_swap): entering and leaving AutoencoderKL.ema_scope costs one launch per
arena each way, and leaving restores the exact bits.  Building, `.to()`, state_dict and load_state_dict work on the CPU; an update or a
swap needs a HIP device (lib.HipLibraryError otherwise, like every op)."""
import weakref

import torch
import torch.nn as nn

from . import lib as _lib
from . import ops


class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.m_name2s_name = {}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0, dtype=torch.int) if use_num_upates else torch.tensor(-1, dtype=torch.int))
        for name, p in model.named_parameters():
            if p.requires_grad:
                s_name = name.replace(".", "")      # a buffer name may hold no "."
                self.m_name2s_name[name] = s_name
                self.register_buffer(s_name, p.clone().detach().data)
        self.collected_params = []
        self._state = None        # device [1 - d, d] of the last tick
        self._plan = None         # [(parameter storage, shadow storage, floats)] once materialised
        self._plan_key = None
        self._pairs_of = None     # (weak reference to the model, its [(parameter, shadow buffer name)])
        self.arenas = []          # [(parameter arena, shadow arena, floats)] per FusedAdam arena, once materialised

    def __getstate__(self):
        """A copy or a pickle takes the buffers, not the launch plan: that is rebuilt on the next update"""
        state = self.__dict__.copy()
        state.update(_state=None, _plan=None, _plan_key=None, _pairs_of=None, arenas=[])
        return state

    def reset_num_updates(self):
        del self.num_updates
        self.register_buffer("num_updates", torch.tensor(0, dtype=torch.int))

    # ---- layout ---------------------------------------------------------------------------------------------------------------------
    def _pairs(self, model=None):
        """[(parameter, shadow buffer)] of every shadowed parameter, in named_parameters() order; model=None: the model of the last call"""
        if model is None or (self._pairs_of is not None and self._pairs_of[0]() is model):
            if self._pairs_of is None or self._pairs_of[0]() is None:
                raise RuntimeError("LitEma: no model seen yet; call forward(model) / materialize(optimizers, model) first")
            return [(p, self._buffers[n]) for p, n in self._pairs_of[1]]
        out = []
        for name, p in model.named_parameters():
            s_name = self.m_name2s_name.get(name)
            if s_name is not None:
                out.append((p, s_name))
            elif p.requires_grad:
                raise KeyError("LitEma: %s requires a gradient and has no shadow (it did not when the average was built)" % name)
        self._pairs_of = (weakref.ref(model), out)      # (Parameter objects outlive `.to()`; buffers are replaced by it, hence looked up by name)
        return [(p, self._buffers[n]) for p, n in out]

    def materialize(self, optimizers, model=None):
        """Lay the shadows out like the parameter arenas: for each materialised FusedAdam whose parameters are all shadowed, one shadow arena
        with the same offsets, the buffers re-pointed at views of it (their values kept), the way FusedAdam.materialize re-points parameters.
        Shadowed parameters in no such arena keep a buffer each.  Call after the optimizers have materialised, with the model on its device."""
        pairs = self._pairs(model)
        shadow_of = {id(p): s for p, s in pairs}
        arenas, taken = [], set()
        for opt in optimizers:
            flat = getattr(opt, "_flat", None)
            if flat is None or not all(id(p) in shadow_of for p in flat["params"]):
                continue
            arena = torch.zeros_like(flat["p"])
            for p, off in zip(flat["params"], flat["offsets"]):
                s = shadow_of[id(p)]
                view = arena[off:off + p.numel()].view(p.shape)
                view.copy_(s.data)
                s.data = view
                taken.add(id(p))
            arenas.append((flat["p"], arena, flat["total"]))
        self.arenas = arenas
        self._plan = arenas + [(p.data, s.data, p.numel()) for p, s in pairs if id(p) not in taken]
        self._plan_key = self._key(pairs)
        return self

    @staticmethod
    def _key(pairs):
        return tuple((p.data_ptr(), s.data_ptr()) for p, s in pairs)

    def _launches(self, model=None):
        """[(parameter storage, shadow storage, floats)]: the arenas and the strays once materialised, else one entry per parameter.  The plan
        holds the live storage; it is dropped for the per-parameter form when a parameter or a shadow has moved since (a later `.to()`)."""
        pairs = self._pairs(model)
        key = self._key(pairs)
        if self._plan is None or self._plan_key != key:
            self._plan = [(p.data, s.data, p.numel()) for p, s in pairs]
            self._plan_key = key
            self.arenas = []
        return self._plan

    def shadow_storages(self, model=None):
        """The tensors that hold every shadow (arenas, then strays): what a data-parallel run broadcasts from rank 0"""
        return [s for _, s, _ in self._launches(model)]

    # ---- the update -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, model):
        plan = self._launches(model)
        _lib.require_device(self.decay)
        if self._state is None or self._state.device != self.decay.device:
            self._state = torch.zeros(2, dtype=torch.float32, device=self.decay.device)
        ops.ema_tick(self.decay, self.num_updates, self._state)
        for p, s, n in plan:
            ops.ema_update(p, s, self._state, n)

    @torch.no_grad()
    def swap(self, model):
        """Parameters <-> shadows, one launch per arena and stray parameter.  The parameters change behind torch's version counters: the
        caller bumps ops.PACK_CACHE."""
        for p, s, n in self._launches(model):
            ops.ema_swap(p, s, n)

    # ---- upstream's interface ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def copy_to(self, model):
        for p, s in self._pairs(model):
            p.data.copy_(s.data)

    def store(self, parameters):
        self.collected_params = [p.clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        for c, p in zip(self.collected_params, parameters):
            p.data.copy_(c.data)
        self.collected_params = []
