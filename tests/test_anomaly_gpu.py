"""Anomaly mode on the device (anomaly.py, csrc/anomaly.hip): the scan kernel on bit patterns, sizes and views; parity with
torch.autograd.set_detect_anomaly(True) on the product path (same node, same output index); the state after AnomalyError; clean runs
bit-identical with the mode on and off; no host synchronisation in the hooks; no steady-state memory growth."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
GAN = dict(perceptual_weight=1.0, disc_factor=1.0, disc_start=0)

F32_NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000]   # +-qNaN, +-sNaN, payloads
F32_INFS = [0x7F800000, 0xFF800000]
BF16_NANS = [0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF]
BF16_INFS = [0x7F80, 0xFF80]


def _i32(bits):
    return int(np.array([bits], dtype=np.uint32).view(np.int32)[0])


def _i16(bits):
    return int(np.array([bits], dtype=np.uint16).view(np.int16)[0])


def _poke(t, k, bits):
    """Write the raw bit pattern `bits` into element k of the flat contiguous tensor t."""
    if t.dtype == torch.float32:
        t.view(torch.int32)[k] = _i32(bits)
    else:
        t.view(torch.int16)[k] = _i16(bits)


def _record():
    return torch.empty(1, dtype=torch.int64, device="cuda:0")


def _read(rec):
    torch.cuda.synchronize()
    return int(rec.item())


def _key(seq, idx):
    return (seq << 20) | idx


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 4096 + 5, 64 * 1024 * 1024 + 3])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_scan_finds_nan_at_first_middle_last(hip_lib, dtype, n, offset):
    from odvae_amd import anomaly
    base = torch.randn(n + offset, device="cuda:0").to(dtype)
    x = base[offset:]                          # a view at an odd element offset: scalar head, vector body, scalar tail
    rec = _record()
    nans = F32_NANS if dtype == torch.float32 else BF16_NANS
    anomaly.reset(rec)
    anomaly.scan([(x, 0)], 1, "nan", rec)
    anomaly.scan([(x, 1)], 2, "nonfinite", rec)
    assert _read(rec) == anomaly.CLEAN
    for j, k in enumerate(sorted({0, n // 2, n - 1})):
        for pat in (nans if n < 10000 else nans[:2]):
            y = x.clone()
            _poke(y, k, pat)
            z = base.clone()
            _poke(z, offset + k, pat)
            for t in (y, z[offset:]):
                anomaly.reset(rec)
                anomaly.scan([(t, 3)], 7 + j, "nan", rec)
                assert _read(rec) == _key(7 + j, 3), (k, hex(pat))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 4096 + 5])
def test_inf_is_flagged_only_in_nonfinite_mode(hip_lib, dtype, n):
    from odvae_amd import anomaly
    rec = _record()
    infs = F32_INFS if dtype == torch.float32 else BF16_INFS
    big = torch.tensor([3.0e38 if dtype == torch.float32 else 3.0e38], device="cuda:0").to(dtype)   # largest-exponent finite values
    for k in sorted({0, n // 2, n - 1}):
        for pat in infs:
            x = torch.randn(n, device="cuda:0").to(dtype)
            x[0] = big[0]
            _poke(x, k, pat)
            anomaly.reset(rec)
            anomaly.scan([(x, 0)], 4, "nan", rec)
            assert _read(rec) == anomaly.CLEAN
            anomaly.scan([(x, 2)], 4, "nonfinite", rec)
            assert _read(rec) == _key(4, 2)


def test_lowest_node_and_lowest_output_win(hip_lib):
    from odvae_amd import anomaly
    rec = _record()
    bad = torch.randn(1000, device="cuda:0")
    bad[500] = float("nan")
    good = torch.randn(1000, device="cuda:0")
    anomaly.reset(rec)
    anomaly.scan([(bad, 1)], 5, "nan", rec)
    anomaly.scan([(bad, 4)], 3, "nan", rec)
    anomaly.scan([(bad, 0)], 9, "nan", rec)
    assert _read(rec) == _key(3, 4)
    # within one node: output indices 6 and 2 bad, 0 and 4 clean -> 2; across two launches of one node (10 outputs)
    anomaly.reset(rec)
    anomaly.scan([(good, 0), (bad, 6), (good, 4), (bad, 2)], 11, "nan", rec)
    assert _read(rec) == _key(11, 2)
    anomaly.reset(rec)
    items = [(good, i) for i in range(9)] + [(bad.bfloat16(), 9)]
    anomaly.scan(items, 12, "nan", rec)
    assert _read(rec) == _key(12, 9)
    anomaly.scan([(bad, 17)], 12, "nan", rec)
    assert _read(rec) == _key(12, 9)


def test_clean_data_leaves_the_record_untouched(hip_lib):
    from odvae_amd import anomaly
    rec = _record()
    rec.fill_(_key(42, 1))                   # whatever was there stays
    xs = [(torch.randn(s, device="cuda:0").to(dt), i) for i, (s, dt) in
          enumerate([(1, torch.float32), (7, torch.bfloat16), (4101, torch.float32), (1 << 20, torch.bfloat16)])]
    anomaly.scan(xs, 1, "nonfinite", rec)
    anomaly.scan(xs, 2, "nan", rec)
    assert _read(rec) == _key(42, 1)


def test_channels_last_outputs_scan_in_place(hip_lib):
    from odvae_amd import anomaly, ops
    rec = _record()
    x = torch.randn(2, 8, 5, 3, device="cuda:0")
    t = ops._new_cl(2, 8, 5, 3, x)
    t.copy_(x)
    t[1, 7, 4, 2] = float("nan")
    assert anomaly.dense(t) and not t.is_contiguous()
    anomaly.reset(rec)
    anomaly.scan([(t, 0)], 0, "nan", rec)
    assert _read(rec) == _key(0, 0)


# ---- the product path against torch's own anomaly mode ----------------------------------------------------------------------------
class _InjectInf(torch.autograd.Function):
    """Test-only identity whose backward writes one +Inf into the gradient it passes on (when armed)."""
    armed = True

    @staticmethod
    def forward(ctx, x):
        return x.clone(memory_format=torch.preserve_format)

    @staticmethod
    def backward(ctx, g):
        if not _InjectInf.armed:
            return g
        g = g.clone(memory_format=torch.preserve_format)
        g[(0,) * g.dim()] = float("inf")
        return g


def _inject(model, name):
    mod = dict(model.named_modules())[name]
    return mod.register_forward_hook(lambda m, a, out: _InjectInf.apply(out))


def _model(gan=False, precision=None, ckpt=False, seed=23):
    from odvae_amd import synthetic
    torch.manual_seed(seed)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, **(GAN if gan else {})).to("cuda:0").train()
    if ckpt:
        model.decoder.activation_checkpoint = ckpt
    model._global_step = 1
    return model


def _batch(seed=23):
    from odvae_amd import synthetic
    batch = synthetic.make_batch(2, 64, seed=seed)
    return {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in batch.items()}


def _fresh(batch):
    b = dict(batch)
    b["pose_6d"] = batch["pose_6d"].clone()
    return b


PARITY = [(False, None, False, "decoder.up.1.block.0.norm2"), (False, "bf16", False, "decoder.up.1.block.0.norm2"),
          (False, "bf16", "unit", "decoder.up.1.block.1.norm2"), (True, None, False, "loss.discriminator.main.3")]


@pytest.mark.parametrize("gan,precision,ckpt,where", PARITY, ids=["rec+KL", "bf16", "bf16-unit-ckpt", "gan-discriminator"])
def test_same_node_and_output_as_torch_anomaly_mode(hip_lib, gan, precision, ckpt, where):
    import warnings
    from odvae_amd.trainer import AnomalyError, Trainer
    batch = _batch()
    got = {}
    for mode in ("torch", "device"):
        model = _model(gan, precision, ckpt)
        h = _inject(model, where)
        trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1) if gan else (0,), precision=precision,
                          detect_anomaly=(mode == "device"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if mode == "torch":
                with torch.autograd.set_detect_anomaly(True):
                    with pytest.raises(RuntimeError) as e:
                        trainer.training_batch(_fresh(batch), 0)
                m = re.search(r"Function '(\w+)' returned nan values in its (\d+)th output\.", str(e.value))
                assert m, str(e.value)
                got[mode] = (m.group(1), int(m.group(2)))
            else:
                with pytest.raises(AnomalyError) as e:
                    trainer.training_batch(_fresh(batch), 0)
                assert str(e.value).startswith("Function '%s' returned nan values in its %dth output." % (e.value.node, e.value.output_index))
                assert e.value.optimizer_idx == 0 and e.value.global_step == 1 and e.value.rank == 0
                got[mode] = (e.value.node, e.value.output_index)
                assert e.value.module and e.value.module.startswith(where.rsplit(".", 1)[0]), e.value.module
        h.remove()
        assert model.global_step == 1
        del trainer, model
    assert got["torch"] == got["device"], got
    assert got["torch"][0] != "_InjectInfBackward"
    from odvae_amd import ops
    assert hasattr(ops, got["torch"][0][:-len("Backward")]), got          # a product Function (ops.py) made the first NaN


def test_state_is_untouched_after_anomaly(hip_lib, tmp_path):
    import copy
    import warnings
    from odvae_amd.trainer import AnomalyError, Trainer
    model = _model(gan=True)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), detect_anomaly=True)
    batch = _batch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer.training_batch(_fresh(batch), 0)             # clean: Adam moments and step counts exist
        torch.cuda.synchronize()
        # parameters, not buffers: the failing phase's forward has updated BatchNorm running statistics, as it does under torch's mode
        params = {k: v.detach().clone() for k, v in model.named_parameters()}
        opts = [copy.deepcopy(trainer.dump_checkpoint()["optimizer_states"])]
        step = model.global_step
        h = _inject(model, "decoder.up.1.block.0.norm2")
        with pytest.raises(AnomalyError):
            trainer.training_batch(_fresh(batch), 1)
        h.remove()
    torch.cuda.synchronize()
    assert model.global_step == step
    for k, v in model.named_parameters():
        assert torch.equal(v, params[k]), k
    after = trainer.dump_checkpoint()["optimizer_states"]

    def same(a, b):
        if torch.is_tensor(a):
            return torch.equal(a, b)
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return a == b
    assert same(opts[0], after)
    path = trainer.save_checkpoint(os.path.join(tmp_path, "after_anomaly.ckpt"))
    assert os.path.exists(path)


@pytest.mark.parametrize("gan,precision", [(False, None), (False, "bf16"), (True, None)], ids=["rec+KL", "bf16", "gan"])
def test_clean_runs_are_bit_identical_with_the_mode_on(hip_lib, gan, precision):
    import warnings
    from odvae_amd.trainer import Trainer
    batch = _batch()
    runs = {}
    for on in (False, True):
        model = _model(gan, precision)
        trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1) if gan else (0,), precision=precision, detect_anomaly=on)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            losses = [[l.item() for l in trainer.training_batch(_fresh(batch), i)] for i in range(3)]
        if on:
            st = trainer.anomaly.stats()
            assert st["firings"] > 20 and st["watched"] > 20, st        # (the last phase's: the discriminator's with the GAN on)
        runs[on] = (losses, {k: v.detach().cpu() for k, v in model.state_dict().items()})
        del trainer, model
    assert runs[False][0] == runs[True][0]
    for k, v in runs[False][1].items():
        assert torch.equal(v, runs[True][1][k]), k


def test_hooks_and_scans_do_not_synchronise(hip_lib):
    import warnings
    from odvae_amd.trainer import Trainer
    model = _model()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), detect_anomaly=True)
    batch = _batch()
    an = trainer.anomaly
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(2):
            trainer.training_batch(_fresh(batch), i)
        torch.cuda.synchronize()
        opt = trainer.optimizers[0]
        saved = trainer._toggle(0)
        try:
            an.begin(torch.device("cuda:0"))
            torch.cuda.set_sync_debug_mode("error")
            try:
                loss = model.training_step(_fresh(batch), 2, 0)
                opt.zero_grad(set_to_none=True)
                an.watch(loss)
                loss.backward()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert an.seq > 50
            assert an.check() is None                   # the one wait, after the backward
        finally:
            an.end()
            trainer._untoggle(saved)


@pytest.mark.parametrize("gan", [False, True], ids=["rec+KL", "gan"])
def test_steady_state_memory_with_the_mode_on(hip_lib, gan):
    import gc
    import warnings
    from odvae_amd import ops
    from odvae_amd.trainer import Trainer
    model = _model(gan)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1) if gan else (0,), detect_anomaly=True)
    batch = _batch()

    def held():
        torch.cuda.synchronize()
        st = torch.cuda.memory_stats()
        return st["allocated_bytes.all.current"], st["allocation.all.current"], len(ops.PACK_CACHE.store)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(3):
            trainer.training_batch(_fresh(batch), i)
        gc.collect()
        base = held()
        seen = []
        for i in range(3, 9):
            trainer.training_batch(_fresh(batch), i)
            gc.collect()
            seen.append(held())
    assert all(s == base for s in seen), (base, seen)
    assert not trainer.anomaly.seen and not trainer.anomaly.tags
