"""Minimal training loop with the semantics of the reference's PL-1.9 Trainer for this model.

Per batch, for optimizer_idx in (0, 1): toggle_optimizer -> training_step -> zero_grad -> backward (DDP buckets fire)
-> clip_grad_norm_(gradient_clip_val) -> optimizer.step -> untoggle; global_step advances once per optimizer step,
i.e. by 2 per batch (every `global_step` threshold in the model and the loss depends on that).
`accumulate_grad_batches = N` stretches zero_grad ... step over a window of N batches (backward of loss / N each, no exchange before the last).
`fit` takes any iterable of batch dicts; `validate` drives `validation_step` (src/models/autoencoder.py:332-363) over a loader with
the epoch mean and the `sync_dist` rank mean of `val/rec_loss`; `save_checkpoint` / `load_checkpoint` write and read the
Lightning-1.9 checkpoint layout the reference's `ModelCheckpoint` produces (train.py:228-249), so a run of this trainer resumes
under the reference and the reverse.  The rest of train.py (CLI, loggers) is out of scope.
"""
import os

import torch

from . import anomaly
from .anomaly import AnomalyError  # noqa: F401  (raised by training_batch; importable from here)
from .parallel import GradReducer


class DeviceHealthError(RuntimeError):
    """A HIP kernel reported, through the library's device-side health counters, that it produced wrong numbers."""


class _TrainerHandle:
    """What `model.trainer` exposes to the module (the optimizer list drives PL-style toggling)."""

    def __init__(self, optimizers):
        self.optimizers = optimizers


class Trainer:
    def __init__(self, model, gradient_clip_val=None, optimizer_indices=(0, 1), process_group=None, bucket_mb=None, precision=None,
                 distributed=None, comm_dtype=None, callbacks=(), logger=None, comm_f32_accumulate=False,
                 detect_anomaly=None, accumulate_grad_batches=1, perceptual_precision=None, discriminator_precision=None,
                 sync_batchnorm=False, float32_matmul_precision=None, gradient_clip_algorithm=None, track_grad_norm=-1):
        """optimizer_indices: which of the model's optimizers run each batch; (0,) is the "rec+KL only" benchmark
        configuration (discriminator off, optimizer 1 skipped -- SURVEY.md 8(d)).
        comm_dtype: dtype of the gradient buckets on the wire; None = f32 in every precision -- what the reference's `strategy: ddp`
        all-reduces under `precision: bf16` too (autocast leaves parameters and their gradients f32).  torch.bfloat16 is an opt-in:
        half the bytes per link, ~2^-9 relative rounding on every summed gradient element (deliberate deviations).
        bucket_mb: f32 megabytes of gradient arena per all-reduce; None = 32, or 16 with bf16 buckets (8 MB on the wire: ~18
        collectives inside the bf16 step's ~50 ms backward).
        distributed: None = data-parallel exactly when a process group is given or the default group has more than one rank
        (what `strategy: ddp` amounts to, yaml:137); False = never (a single-process reference run inside a rank).
        detect_anomaly: lightning.trainer.detect_anomaly of the yaml (:138).  False = off; True or "nan" = torch's anomaly mode semantics
        (the first backward node that returns a NaN output raises AnomalyError before clipping and the optimizer step); "nonfinite" also
        flags +-Inf; None reads ODVAE_DETECT_ANOMALY (unset / 0 = off, 1 = nan, nonfinite).  The checks run on the device
        (anomaly.py): one host wait per optimizer step.
        accumulate_grad_batches: lightning.trainer.accumulate_grad_batches of the yaml (:134), PL-1.9 automatic optimisation: N consecutive
        batches form a window; every batch back-propagates loss / N into gradients that are zeroed only before the window's first backward; clip,
        optimizer.step() and the global_step increment happen on the window's last batch only.  1 = a step after
        every batch.
        perceptual_precision: 32 or "bf16" for the loss's LPIPS-style net (AutoencoderKL.set_precision); None leaves it alone.
        discriminator_precision: the same for the loss's PatchGAN discriminator (NLayerDiscriminator.set_precision).
        sync_batchnorm: lightning.trainer.sync_batchnorm of the yaml / `--sync_batchnorm True` (PL 1.9 runs
        torch.nn.SyncBatchNorm.convert_sync_batchnorm over the module; its only BatchNorm layers are the discriminator's three).  True in a
        data-parallel run over more than one rank: those layers take their training statistics and backward sums over this trainer's
        process group (gan.BatchNormLReLU.dist_group).  Not data-parallel, one rank, or use_actnorm: nothing changes.
        float32_matmul_precision: "highest", "high", "medium" or "torch" -- what the reference's launcher sets with
        torch.set_float32_matmul_precision (train.py:521: 'medium'); ops/precision.py.  Process-global, like torch's, and not
        restored when the trainer goes away.  None leaves the setting (ODVAE_FLOAT32_MATMUL_PRECISION, default highest) alone.
        gradient_clip_algorithm: the PL-1.9 Trainer argument.  None or "norm": gradient_clip_val is the global L2 bound of
        clip_grad_norm_ (today's path, bit for bit).  "value": gradient_clip_val is an element-wise bound, torch.nn.utils.clip_grad_value_
        (FusedAdam clamps inside the Adam kernel and leaves `.grad` unclipped, as its norm clipping does); it needs a gradient_clip_val.
        Anything else raises ValueError.
        track_grad_norm: the PL-1.9 Trainer argument.  -1 = off; a number > 0, 'inf' or float('inf') = on every stepping batch, after the
        backward, the reducer's finish() and the anomaly check and BEFORE clipping, the p-norm of the gradient of every parameter of
        the optimizer being stepped that the backward reached, and their total, go through `model.log_dict` under
        "grad_<p>_norm/<name>" and "grad_<p>_norm_total" (<p> = float(p): 2.0, inf; <name> from model.named_parameters()).  The values
        are 0-d views of one device vector (FusedAdam.grad_norms: no host wait); `self.grad_norms[optimizer_idx] = (names, vector)`
        keeps each optimizer's last vector, total last.  Data-parallel: the norms of the reduced gradients, the same on every rank.
        Inside an accumulation window nothing is tracked before the window's last batch; then the norms are of the summed gradients.
        Tracking changes no bit of the run.  Deviation from PL (restated, not pinned against it: pytorch_lightning is not available to
        the build): PL walks every named parameter with a non-None `.grad`, stale gradients of the untoggled optimizer included; this
        trainer tracks the stepped optimizer's parameters only.  An optimizer that is not a FusedAdam (CPU, gloo) takes p.grad.norm(p) of its
        parameters whose `.grad` is not None (PL's rule; the gradient reducer hands every parameter a slice of its bucket, so an unreached one
        reads 0 there) and torch.nn.utils.clip_grad_value_.  bool, 0, other negatives, NaN and other strings raise ValueError."""
        if gradient_clip_algorithm not in (None, "norm", "value"):
            raise ValueError("gradient_clip_algorithm must be None, 'norm' or 'value', got %r" % (gradient_clip_algorithm,))
        if gradient_clip_algorithm == "value" and not gradient_clip_val:
            raise ValueError("gradient_clip_algorithm='value' needs a gradient_clip_val, got %r" % (gradient_clip_val,))
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.track_grad_norm = parse_track_grad_norm(track_grad_norm)      # None = off, else a float (inf for 'inf')
        self.grad_norms = {}              # optimizer_idx -> (names, device vector [len(names) + 1], total last) of its last tracked step
        self._param_names = None
        self._norm_picks = {}             # (optimizer_idx, reached parameters) -> device index vector, when not every parameter was reached
        if float32_matmul_precision is not None:
            from . import ops
            ops.set_float32_matmul_precision(float32_matmul_precision)      # (a bad name raises before anything else is touched)
        if not isinstance(sync_batchnorm, bool):
            raise ValueError("sync_batchnorm must be True or False, got %r" % (sync_batchnorm,))
        self.sync_batchnorm = sync_batchnorm
        if isinstance(accumulate_grad_batches, bool) or not isinstance(accumulate_grad_batches, int) or accumulate_grad_batches < 1:
            raise ValueError("accumulate_grad_batches must be an integer >= 1, got %r" % (accumulate_grad_batches,))
        self.accumulate_grad_batches = accumulate_grad_batches
        self._window_pos = 0              # micro-batches already in the open accumulation window (0 = closed)
        self.model = model
        # callbacks: objects with the pytorch_lightning.Callback hooks used by the reference's yaml (callbacks.ImageLogger, ...);
        # `on_train_batch_end` runs after the last optimizer step of a batch, as under PL's automatic optimisation.  logger: anything
        # with a `save_dir` (ImageLogger writes <save_dir>/images/<split>/...); it becomes `model.logger`.
        self.callbacks = list(callbacks)
        if logger is not None:
            try:
                model.logger = logger
            except AttributeError:      # a real pytorch_lightning.LightningModule: `logger` is a read-only property of its Trainer
                model._odvae_logger = logger
        if precision is not None:   # lightning.trainer.precision of the yaml (:139): 32 or "bf16"
            extra = {}
            if perceptual_precision is not None:
                extra["perceptual_precision"] = perceptual_precision
            if discriminator_precision is not None:
                extra["discriminator_precision"] = discriminator_precision
            model.set_precision(precision, **extra)
        else:
            if perceptual_precision is not None:
                model.loss.perceptual_loss.set_precision(perceptual_precision)
            if discriminator_precision is not None:
                disc = getattr(model.loss, "discriminator", None)
                if not hasattr(disc, "set_precision"):
                    raise ValueError("discriminator_precision=%r: the loss has no discriminator" % (discriminator_precision,))
                disc.set_precision(discriminator_precision)
        self.clip = gradient_clip_val
        self.detect_anomaly = anomaly.parse_mode(detect_anomaly)
        self.anomaly = anomaly.Detector(self.detect_anomaly, model) if self.detect_anomaly else None
        self.optimizer_indices = tuple(optimizer_indices)
        opts, _ = model.configure_optimizers()
        self.optimizers = opts
        for o in opts:
            if hasattr(o, "materialize"):
                o.materialize()
        # model.params.ema_decay: the shadows of the weights take the layout of the parameter arenas (one update launch per arena)
        ema = getattr(model, "model_ema", None) if getattr(model, "use_ema", False) else None
        if ema is not None and hasattr(ema, "materialize") and _device_of(model).type == "cuda":
            ema.materialize(opts, model)
        model.trainer = _TrainerHandle(opts)
        self.current_epoch = 0           # completed passes over the training loader (PL: trainer.current_epoch)
        # device-side health counters as of the last check_device_health(): GroupNorm team-barrier timeouts (fatal) and exact-softmax
        # fallbacks of the folded attention softmax (correct, slower; reported)
        self.device_health = {"gn_barrier_timeouts": 0, "attn_softmax_fallbacks": 0, "gn_recentred": 0}
        self.callback_metrics = {}        # name -> 0-d CPU tensor: the last validate()'s epoch means (what ModelCheckpoint monitors)
        self.reducers = None
        if distributed is None:
            distributed = process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                                        and torch.distributed.get_world_size() > 1)
        if distributed:
            # the mean over ranks rides in the loss scale (training_batch), not in a pass over the gradient arena
            if bucket_mb is None:
                bucket_mb = 16.0 if comm_dtype == torch.bfloat16 else 32.0
            self.reducers = [GradReducer(o, process_group=process_group, bucket_mb=bucket_mb, prescaled=True, comm_dtype=comm_dtype, f32_accumulate=comm_f32_accumulate)
                             for o in opts]
            self.reducers[0].broadcast_parameters(model)
            if hasattr(model, "noise_rank"):      # device_noise: the rank goes into the Philox key, so the ranks draw different noise
                model.noise_rank = torch.distributed.get_rank(process_group)
            if ema is not None:
                # rank 0's average everywhere, once, as whole arenas: from here on every rank computes the same bits from the same
                # parameters, with no communication
                with torch.no_grad():
                    for t in ema.shadow_storages(model) + [ema.decay.data, ema.num_updates.data]:
                        torch.distributed.broadcast(t, src=0, group=process_group)
            # ActNorm layers initialise from data on their first training forward: rank 0's values then go to every rank (parallel.broadcast_actnorm)
            for m in model.modules():
                if hasattr(m, "dist_group") and hasattr(m, "refresh_initialized"):
                    m.dist_group = process_group if process_group is not None else torch.distributed.group.WORLD
                    m.refresh_initialized()
        # sync_batchnorm: the discriminator's BatchNorm layers get this trainer's group, or lose one a former Trainer gave them
        group = None
        if distributed and sync_batchnorm:
            group = process_group if process_group is not None else torch.distributed.group.WORLD
            if torch.distributed.get_world_size(group) < 2:
                group = None
        for m in model.modules():
            if hasattr(m, "batchnorm_layers"):
                for bn in m.batchnorm_layers():
                    bn.dist_group = group

    # PL-1.9 toggle_optimizer: parameters owned by the *other* optimizers stop requiring grad; parameters in no
    # optimizer (loss.logvar, the frozen LPIPS net) are left alone
    def _toggle(self, idx):
        mine = {id(p) for g in self.optimizers[idx].param_groups for p in g["params"]}
        saved = {}
        for j, opt in enumerate(self.optimizers):
            if j == idx:
                continue
            for g in opt.param_groups:
                for p in g["params"]:
                    if id(p) not in mine and id(p) not in saved:
                        saved[id(p)] = (p, p.requires_grad)
                        p.requires_grad = False
        return saved

    @staticmethod
    def _untoggle(saved):
        for p, rg in saved.values():
            p.requires_grad = rg

    @property
    def accumulation_index(self):
        """Micro-batches in the open gradient-accumulation window; 0 when no window is open."""
        return self._window_pos

    def _discard_window(self):
        self._window_pos = 0
        for o in self.optimizers:
            if hasattr(o, "discard_window"):
                o.discard_window()

    def training_batch(self, batch, batch_idx=0, last_in_epoch=False):
        """One batch = one step of each scheduled optimizer.  Returns the list of loss tensors (device, not synced).
        With accumulate_grad_batches = N > 1 one batch is one micro-batch of a window: each scheduled optimizer still gets its toggle,
        training_step and backward (of loss / N), but it is stepped -- clip, step, global_step + 1 -- only on the window's last batch, the N-th
        or the one flagged `last_in_epoch` (the divisor stays N).  The returned losses are unscaled."""
        model = self.model
        losses = []
        n_acc = self.accumulate_grad_batches
        first = self._window_pos == 0
        final = self._window_pos + 1 >= n_acc or bool(last_in_epoch)
        try:
            for idx in self.optimizer_indices:
                opt = self.optimizers[idx]
                saved = self._toggle(idx)
                an = self.anomaly
                try:
                    if an is not None:
                        an.begin(_device_of(model))      # before training_step: PoseLoss's torch.autograd.grad passes are checked too
                    loss = model.training_step(batch, batch_idx, idx)
                    if first:
                        opt.zero_grad(set_to_none=True)   # FusedAdam: gradients are gathered into its arena after the backward (optim.gather_grads)
                    elif hasattr(opt, "begin_microbatch"):
                        opt.begin_microbatch()            # FusedAdam: the arena keeps the sums, the backward hands over fresh kernel outputs again
                    root = loss if n_acc == 1 else loss / n_acc
                    red = self.reducers[idx] if self.reducers else None
                    if red is not None:
                        if n_acc == 1:
                            red.prepare_for_backward()
                        else:                             # DDP no_sync until the window's last backward, which exchanges the accumulated sums
                            red.prepare_for_backward(first=first, sync=final)
                        root = root * red.inv_world       # sum over ranks of grad(loss / world) = DDP's mean gradient
                        if an is not None:
                            an.watch(root)
                        root.backward()
                        red.finish()
                    else:
                        if an is not None:
                            an.watch(root)
                        root.backward()
                    if an is not None:
                        self._check_anomaly(an, idx, red)
                    if final:
                        # (FusedAdam inside a window: clip_grad_norm_ / step add whatever this backward left fresh to the arena's sums first)
                        if self.track_grad_norm is not None:
                            self._track_grad_norms(idx, opt)      # the unclipped gradients, as in PL
                        if self.clip:
                            if self.gradient_clip_algorithm == "value":
                                if hasattr(opt, "clip_grad_value_"):
                                    opt.clip_grad_value_(self.clip)
                                else:
                                    torch.nn.utils.clip_grad_value_([p for g in opt.param_groups for p in g["params"]], self.clip)
                            elif hasattr(opt, "clip_grad_norm_"):
                                opt.clip_grad_norm_(self.clip)
                            else:
                                torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], self.clip)
                        opt.step()
                    elif hasattr(opt, "gather_grads"):
                        opt.gather_grads(accumulate=not first)   # one multi-tensor copy (window start) or add (later) into the arena
                finally:
                    self._untoggle(saved)
                    if an is not None:
                        an.end()
                if final:
                    model._global_step += 1
                losses.append(loss.detach())
        except AnomalyError:
            if n_acc > 1:
                self._discard_window()    # the next batch starts a new window
            raise
        self._window_pos = 0 if final else self._window_pos + 1
        for cb in self.callbacks:
            cb.on_train_batch_end(self, model, losses, batch, batch_idx)
        # PL 1.9: the callbacks' hook first, then the module's own (AutoencoderKL: one update of the weight average per batch, also inside an
        # accumulation window).  A batch that ended in AnomalyError has left above and makes no update.
        hook = getattr(model, "on_train_batch_end", None)
        if hook is not None:
            hook(losses, batch, batch_idx)
        return losses

    def _track_grad_norms(self, idx, opt):
        """track_grad_norm for the optimizer about to be stepped: names, one vector, log_dict (the constructor's docstring)."""
        p = self.track_grad_norm
        if self._param_names is None:
            self._param_names = {id(q): name for name, q in self.model.named_parameters()}
        names = self._param_names
        params = [q for g in opt.param_groups for q in g["params"]]
        if hasattr(opt, "grad_norms"):
            reached = [i for i in sorted(opt._touched) if id(params[i]) in names]      # (read before grad_norms: a host set)
            vec = opt.grad_norms(p)
            if len(reached) != len(params):      # some parameters had no gradient: their entries leave the vector (index cached per set)
                key = (idx, tuple(reached))
                pick = self._norm_picks.get(key)
                if pick is None:
                    if len(self._norm_picks) >= 16:
                        self._norm_picks.clear()
                    pick = self._norm_picks[key] = torch.tensor(reached + [len(params)], dtype=torch.long, device=vec.device)
                vec = vec.index_select(0, pick)
            logged = [names[id(params[i])] for i in reached]
            picked = vec
            values = vec.unbind(0)      # 0-d views of the one vector
            total = values[-1]
        else:
            keep = [q for q in params if q.grad is not None and id(q) in names]
            logged = [names[id(q)] for q in keep]
            with torch.no_grad():
                values = [q.grad.detach().norm(p) for q in keep]
                total = torch.stack(values).norm(p) if values else torch.zeros(())
                picked = torch.stack(values + [total])
        self.grad_norms[idx] = (logged, picked)
        d = {"grad_%s_norm/%s" % (p, name): v for name, v in zip(logged, values)}
        d["grad_%s_norm_total" % p] = total
        self.model.log_dict(d, prog_bar=False, logger=True, on_step=True, on_epoch=False)

    def _check_anomaly(self, an, idx, red):
        """One host wait for the phase's anomaly record (all-reduced MIN over the ranks when data-parallel, so every rank raises);
        AnomalyError before clip / step / the global_step increment: no parameter, moment or step count takes in the bad step."""
        group = None
        if red is not None:
            import torch.distributed as dist
            group = red.group if red.group is not None else dist.group.WORLD
        found = an.check(group)
        if found is None:
            return
        name, index, module = found
        rank, world = _rank(), _world()
        gs = int(self.model.global_step)
        raise AnomalyError("%s (optimizer %d, global_step %d, rank %d of %d)" % (an.message(name, index, module), idx, gs, rank, world),
                           node=name, output_index=index, module=module, optimizer_idx=idx, global_step=gs, rank=rank)

    def check_device_health(self, where=""):
        """Reads the library's device-side counters (odvae_device_health, odvae_groupnorm_recentred: device synchronisations, so it is called only where the
        host waits anyway -- validation, checkpoint save, the end of fit).  A GroupNorm backward whose team barrier gave up has written
        WRONG gradients (csrc/groupnorm.hip: the opt-in team mode, odvae_groupnorm_select_backward(1)): DeviceHealthError, and no
        checkpoint is written from such a state.  Fallbacks of the folded attention softmax are exact; new ones since the last check are
        reported once through `warnings` and to the logger's `log_metrics` when it has one; so are GroupNorm statistics that had to be
        recentred (csrc/gn_finalize.h), through `warnings`.  Returns the counters."""
        import ctypes
        import warnings
        from . import lib as _lib
        if not torch.cuda.is_available():
            return dict(self.device_health)
        L = _lib.load()
        gn, at = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(L.odvae_device_health(ctypes.byref(gn), ctypes.byref(at), 0, 0), "device_health")
        prev = self.device_health
        rc = int(L.odvae_groupnorm_recentred(0))
        if rc < 0:
            raise _lib.HipLibraryError("device_health: cannot read the GroupNorm recentring counter")
        self.device_health = {"gn_barrier_timeouts": int(gn.value), "attn_softmax_fallbacks": int(at.value), "gn_recentred": rc}
        if gn.value > prev["gn_barrier_timeouts"]:
            raise DeviceHealthError(
                "%d GroupNorm team-barrier wait(s) gave up on the device%s (global_step %d): the gradients of those launches are wrong. "
                "The team mode is opt-in (odvae_groupnorm_select_backward(1)); the default never waits across blocks."
                % (gn.value - prev["gn_barrier_timeouts"], (" before " + where) if where else "", int(self.model.global_step)))
        if at.value > prev["attn_softmax_fallbacks"]:
            new = at.value - prev["attn_softmax_fallbacks"]
            warnings.warn("%d attention block(s) took the exact-softmax fallback since the last check (global_step %d): a row's Cauchy-Schwarz "
                          "bound underflowed in f32; results are exact, each fallback costs three extra passes over its T x T scores"
                          % (new, int(self.model.global_step)), RuntimeWarning, stacklevel=2)
            logger = getattr(self.model, "logger", None) or getattr(self.model, "_odvae_logger", None)
            log = getattr(logger, "log_metrics", None)
            if log is not None:
                log({"device/attn_softmax_fallbacks": float(at.value)}, step=int(self.model.global_step))
        if rc > prev.get("gn_recentred", 0):
            warnings.warn("%d GroupNorm (sample, group) statistics were taken from centred sums since the last check (global_step %d): "
                          "|mean| / std of those groups exceeded 8; results are exact, each one costs a second read of its group by one wavefront"
                          % (rc - prev.get("gn_recentred", 0), int(self.model.global_step)), RuntimeWarning, stacklevel=2)
        return dict(self.device_health)

    def fit(self, batches, max_batches=None, val_batches=None, max_epochs=1):
        """`max_epochs` passes over `batches` (re-iterated per epoch; at most `max_batches` each).  With `val_batches` every epoch
        ends as PL's does: validation over the whole loader, `on_validation_end` (ModelCheckpoint saves here), then the epoch counter
        advances.  Returns the per-batch loss lists of every epoch, flattened."""
        out = []
        for _ in range(max_epochs):
            self.model.train()
            if self.accumulate_grad_batches == 1:
                for i, batch in enumerate(batches):
                    if max_batches is not None and i >= max_batches:
                        break
                    out.append(self.training_batch(batch, i))
            else:       # one batch of look-ahead: the epoch's last batch (or the `max_batches` cut) closes the accumulation window
                it, end = iter(batches), object()
                nxt, i = next(it, end), 0
                while nxt is not end and (max_batches is None or i < max_batches):
                    batch, nxt = nxt, next(it, end)
                    last = nxt is end or (max_batches is not None and i + 1 >= max_batches)
                    out.append(self.training_batch(batch, i, last_in_epoch=last))
                    i += 1
            if val_batches is not None:
                self.validate(val_batches)
            self._set_epoch(self.current_epoch + 1)
        self.check_device_health("the end of fit")
        return out

    def _set_epoch(self, epoch):
        self.current_epoch = int(epoch)
        try:
            self.model.current_epoch = self.current_epoch
        except AttributeError:      # a real LightningModule: read-only, its own Trainer owns the counter
            pass

    # ---- validation (src/models/autoencoder.py:332-363; [PL-1.9] evaluation loop) -----------------------------------------------
    @torch.no_grad()
    def validate(self, batches, max_batches=None):
        """model.eval(), `validation_step` per batch under no_grad, every logged scalar averaged over the epoch the way [PL-1.9] does it
        for `self.log(..., on_epoch=True)` inside validation_step: the mean WEIGHTED BY BATCH SIZE (ResultMetric: value * batch_size
        summed, divided by the cumulated batch size; the batch size is the first dimension of the first tensor in the batch,
        `extract_batch_size`) -- with a ragged last batch this is what the reference's ModelCheckpoint(monitor) sees;
        `val/rec_loss` is logged with `sync_dist=True` (:359), so each batch value already is the mean over the ranks.  The epoch means land in
        `self.callback_metrics` (and are returned); callbacks see `on_validation_batch_end` per batch and `on_validation_end` once.
        The model's training mode is restored."""
        model = self.model
        was_training = model.training
        model.eval()
        sums, counts = {}, {}
        try:
            for i, batch in enumerate(batches):
                if max_batches is not None and i >= max_batches:
                    break
                logged = getattr(model, "_logged", None)
                if logged is not None:
                    logged.clear()
                out = model.validation_step(batch, i)
                bs = _batch_size(batch)
                for k, v in (getattr(model, "logged_metrics", None) or {}).items():
                    if torch.is_tensor(v):
                        if v.numel() != 1:
                            continue
                        v = v.detach().double().reshape(())
                    else:
                        v = torch.tensor(float(v), dtype=torch.float64)
                    v = v * bs
                    sums[k] = v if k not in sums else sums[k] + v.to(sums[k].device)      # stays on the device: no sync per batch
                    counts[k] = counts.get(k, 0) + bs
                for cb in self.callbacks:
                    cb.on_validation_batch_end(self, model, out, batch, i)
        finally:
            model.train(was_training)
        metrics = {k: (sums[k] / counts[k]).float().cpu() for k in sums}      # (the host waits for the device here anyway)
        self.check_device_health("validation ended")
        self.callback_metrics.update(metrics)
        for cb in self.callbacks:
            hook = getattr(cb, "on_validation_end", None)
            if hook is not None:
                hook(self, model)
        return metrics

    # ---- checkpoints: the Lightning-1.9 layout (train.py:228-249 ModelCheckpoint; [PL-1.9] CheckpointConnector.dump_checkpoint) --
    def dump_checkpoint(self, weights_only=False):
        """{"epoch", "global_step", "pytorch-lightning_version", "state_dict"} and, unless `weights_only` (the reference's default,
        train.py:236), {"optimizer_states", "lr_schedulers", "callbacks"}: optimizer_states[i] is optimizer i's `state_dict()` in
        torch.optim.Adam's layout (optim.FusedAdam writes exactly that), lr_schedulers is empty (configure_optimizers returns none,
        autoencoder.py:377).  `state_dict` keys / shapes / dtypes are the reference module tree's (OIHW f32); every
        tensor is copied to the host.  No "loops" entry: PL-1.9 then restores `global_step` and `epoch` from the top-level keys (its
        path for pre-1.6 checkpoints) instead of from a progress-tracker tree this trainer does not keep.
        RuntimeError inside an open gradient-accumulation window: the layout carries no gradients, the window's sums would be lost silently."""
        self._no_open_window("dump_checkpoint")
        model = self.model
        ckpt = {"epoch": self.current_epoch, "global_step": int(model.global_step), "pytorch-lightning_version": "1.9.0",
                "state_dict": {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()}}
        if not weights_only:
            def host(o):
                if torch.is_tensor(o):
                    return o.detach().to("cpu", copy=True)
                if isinstance(o, dict):
                    return {k: host(v) for k, v in o.items()}
                if isinstance(o, (list, tuple)):
                    return type(o)(host(v) for v in o)
                return o
            ckpt["optimizer_states"] = [host(o.state_dict()) for o in self.optimizers]
            ckpt["lr_schedulers"] = []
            ckpt["callbacks"] = {}
            for cb in self.callbacks:
                sd = getattr(cb, "state_dict", None)
                if sd is not None:
                    ckpt["callbacks"][getattr(cb, "state_key", type(cb).__qualname__)] = sd()
        return ckpt

    def _no_open_window(self, what):
        if self._window_pos:
            raise RuntimeError("%s inside an open gradient-accumulation window (%d of %d micro-batches): a Lightning checkpoint carries no "
                               "gradients; finish the window first" % (what, self._window_pos, self.accumulate_grad_batches))

    def save_checkpoint(self, path, weights_only=False):
        """Rank 0 writes `path` (atomically: temporary file + rename); every rank returns the path."""
        self._no_open_window("save_checkpoint")
        self.check_device_health("writing %s" % os.path.basename(path))      # never a checkpoint of weights stepped with wrong gradients
        if _rank() == 0:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            tmp = "%s.part" % path
            torch.save(self.dump_checkpoint(weights_only=weights_only), tmp)
            os.replace(tmp, path)
        return path

    def load_checkpoint(self, path, strict=True, trusted=False):
        """Resume from a checkpoint in that layout -- one of this trainer's or one Lightning wrote for the reference model: weights
        (strict by default), `global_step`, `epoch`, and the optimizer states when present (a weights-only file leaves the
        optimizers fresh, as Lightning does).  The file is read with torch's restricted unpickler (`weights_only=True`: tensors, numbers,
        strings, containers).  A real Lightning checkpoint may also carry arbitrary Python objects (`hyper_parameters` as an OmegaConf
        DictConfig, callback state with timedelta / Path): unpickling those executes code, so it happens only with `trusted=True`."""
        import pickle
        try:
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as e:
            if not trusted:
                raise pickle.UnpicklingError(
                    "%s holds objects torch's restricted unpickler refuses (%s). If the file comes from a source you trust -- a Lightning "
                    "checkpoint with hyper_parameters / callback state -- call load_checkpoint(path, trusted=True)." % (path, str(e).splitlines()[0])) from e
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
        res = self.model.load_state_dict(ckpt["state_dict"], strict=strict)
        if self._window_pos:
            self._discard_window()      # a resume starts at a window boundary
        from . import ops
        ops.PACK_CACHE.bump()           # load_state_dict copies into .data of the arena views: no version bump the pack cache could see
        self.model._global_step = int(ckpt.get("global_step", 0))
        self._set_epoch(ckpt.get("epoch", 0))
        states = ckpt.get("optimizer_states")
        if states is not None:
            if len(states) != len(self.optimizers):
                raise ValueError("checkpoint holds %d optimizer states, the model configures %d optimizers" % (len(states), len(self.optimizers)))
            for o, sd in zip(self.optimizers, states):
                o.load_state_dict(sd)
        return res


def parse_track_grad_norm(value):
    """PL-1.9's Trainer(track_grad_norm=...): -1 -> None (off); a number > 0, 'inf' or float('inf') -> that norm as a float."""
    if isinstance(value, str):
        if value == "inf":
            return float("inf")
    elif not isinstance(value, bool) and isinstance(value, (int, float)):
        if value == -1:
            return None
        if value > 0:       # (NaN fails the comparison)
            return float(value)
    raise ValueError("track_grad_norm must be -1 (off), a number > 0 or 'inf', got %r" % (value,))


def _batch_size(batch):
    """[PL-1.9] extract_batch_size: the first dimension of the first tensor found in the batch (dicts / sequences walked in order); 1 if none."""
    if torch.is_tensor(batch):
        return int(batch.shape[0]) if batch.dim() > 0 else 1
    if isinstance(batch, dict):
        batch = list(batch.values())
    if isinstance(batch, (list, tuple)):
        for v in batch:
            if torch.is_tensor(v):
                return int(v.shape[0]) if v.dim() > 0 else 1
            if isinstance(v, (dict, list, tuple)) and any(torch.is_tensor(x) for x in (v.values() if isinstance(v, dict) else v)):
                return _batch_size(v)
    return 1


def _device_of(model):
    for p in model.parameters():
        return p.device
    return torch.device("cuda", torch.cuda.current_device())


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
