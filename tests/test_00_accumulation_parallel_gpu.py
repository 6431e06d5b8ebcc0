"""Gradient accumulation under data parallelism on device tensors: real PoseAutoencoder + FusedAdam + GradReducer + Trainer(accumulate_grad_batches=2).

1. two ranks share the one GPU over **gloo** (as in tests/test_00_parallel_gpu.py): the first micro-batch of a window launches no bucket (DDP
   `no_sync`), the last one exchanges the accumulated local sums -- both ranks then hold the same arena, which is the arena of ONE process
   accumulating the four shards (mean over ranks of window means = a window of four), in the VAE phase and in the encoder-pretraining phase of the
   untouched yaml, where the decoder gets no gradient and buckets are only partly touched;
2. one rank over **nccl** (= RCCL): N = 2 over four batches through real collectives is bit-identical to the non-distributed N = 2 run.

Every case spawns its ranks BEFORE this pytest process touches the GPU, which is why the file name sorts first."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
OWNED = ("encoder", "decoder", "quant", "post_quant", "pose_")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _shard(rank, step=0):
    """One rank's micro-batch, as in tests/test_00_parallel_gpu.py: every sample carries a pixel at 0 and one at 1."""
    from odvae_amd import synthetic
    batch = synthetic.make_batch(2, 64, seed=50 + 10 * step + rank)
    batch["patch"][:, :, 0, 0] = 0.0
    batch["patch"][:, :, 0, 1] = 1.0
    return batch, synthetic.make_noise(2, 4, seed=70 + 10 * step + rank)


def _arena(trainer):
    torch.cuda.synchronize()
    return trainer.optimizers[0].flat_grad.detach().cpu().clone()


def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    out = {}
    for phase in ("asis", "vae"):
        torch.manual_seed(1000 + rank)       # different initial weights per rank: the broadcast aligns them
        model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, phase=phase)
        model.learning_rate = 0.0            # lr = 0, no clip: the gradient arena survives the optimizer step
        model = model.to("cuda:0").train()
        trainer = Trainer(model, gradient_clip_val=None, optimizer_indices=(0,), bucket_mb=1.0, accumulate_grad_batches=2)
        red = trainer.reducers[0]
        gs = model._global_step = 1 if phase == "vae" else 0      # "asis": 0 < encoder_pretrain_steps -> the decoder is skipped
        res = {"nbuckets": len(red.buckets)}
        for m in range(2):
            batch, noise = _shard(rank, m)
            model.injected_noise = noise
            trainer.training_batch(batch, m)
            res["order%d" % m] = list(red.launch_order)
            res["arena%d" % m] = _arena(trainer)
            res["index%d" % m] = trainer.accumulation_index
        res["global_step"] = model._global_step - gs
        if rank == 0:                        # one process, the same weights, a window over the four shards
            single = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, phase=phase)
            single.load_state_dict(model.state_dict())
            single.learning_rate = 0.0
            single = single.to("cuda:0").train()
            t1 = Trainer(single, gradient_clip_val=None, optimizer_indices=(0,), distributed=False, accumulate_grad_batches=4)
            assert t1.reducers is None
            single._global_step = gs
            for j, (m, r) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
                batch, noise = _shard(r, m)
                single.injected_noise = noise
                t1.training_batch(batch, j)
            assert t1.accumulation_index == 0
            res["arena_full"] = _arena(t1)
            name_of = {id(p): n for n, p in single.named_parameters()}
            res["names"] = [(name_of[id(p)], off, cnt) for p, off, cnt in t1.optimizers[0].param_slices()]
            del single, t1
        out[phase] = res
        del model, trainer
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def _nccl_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    runs = {}
    for mode in ("rccl", "single"):
        torch.manual_seed(23)
        model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32).to("cuda:0").train()
        if mode == "rccl":
            trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), process_group=dist.group.WORLD, bucket_mb=1.0,
                              accumulate_grad_batches=2)
            assert trainer.reducers is not None and dist.get_backend() == "nccl"
        else:
            trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), distributed=False, accumulate_grad_batches=2)
            assert trainer.reducers is None
        model._global_step = 1
        losses, orders = [], []
        for step in range(4):
            batch, noise = _shard(0, step)
            model.injected_noise = noise
            losses.append(trainer.training_batch(batch, step)[0].item())
            if mode == "rccl":
                orders.append(list(trainer.reducers[0].launch_order))
        torch.cuda.synchronize()
        runs[mode] = {"sd": {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith(OWNED)}, "losses": losses,
                      "global_step": model._global_step, "orders": orders, "calls": trainer.optimizers[0].accumulate_calls}
        if mode == "rccl":
            runs[mode]["nbuckets"] = len(trainer.reducers[0].buckets)
        del model, trainer
    torch.save(runs, os.path.join(out_dir, "nccl.pt"))
    dist.destroy_process_group()


def _spawnable():
    if torch.cuda.device_count() < 1:
        pytest.skip("no HIP device")
    if torch.cuda.is_initialized():
        pytest.skip("GPU already initialised in this process; run this file in its own pytest invocation")


def test_two_ranks_exchange_the_accumulated_sums_once_per_window(tmp_path):
    _spawnable()
    world, port = 2, _free_port()
    mp.spawn(_gloo_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    for phase in ("asis", "vae"):
        a, b = r0[phase], r1[phase]
        # first micro-batch: no bucket launched, the ranks hold their own gradients, the window is open
        assert a["order0"] == [] and b["order0"] == [] and a["index0"] == b["index0"] == 1
        assert not torch.equal(a["arena0"], b["arena0"])
        # end of the window: one exchange, identical arenas, one optimizer step
        assert a["nbuckets"] >= 2 and len(a["order1"]) >= 1 and a["order1"] == b["order1"]
        assert a["index1"] == b["index1"] == 0 and a["global_step"] == b["global_step"] == 1
        assert torch.equal(a["arena1"], b["arena1"]), phase
        got, full = a["arena1"].double(), a["arena_full"].double()
        gmax = full.abs().max().item()
        assert gmax > 0
        worst = 0.0
        for name, off, n in a["names"]:
            ref = full[off:off + n]
            err = (got[off:off + n] - ref).abs().max().item()
            scale = max(ref.abs().max().item(), 1e-3 * gmax)
            worst = max(worst, err / scale)
            assert err <= 2e-3 * scale, "%s %s: %.3e vs scale %.3e" % (phase, name, err, scale)
        print("phase %s: worst per-parameter deviation from the one-process window of four: %.2e of its scale" % (phase, worst))
    asis = r0["asis"]
    dec = [(o, n) for name, o, n in asis["names"] if name.startswith("decoder.")]
    assert dec and all(float(asis["arena_full"][o:o + n].abs().max()) == 0.0 for o, n in dec)
    assert len(asis["order1"]) <= asis["nbuckets"] and sorted(r0["vae"]["order1"]) == list(range(r0["vae"]["nbuckets"]))


def test_rccl_world1_window_is_bit_identical_to_single_process(tmp_path):
    _spawnable()
    mp.spawn(_nccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    runs = torch.load(os.path.join(tmp_path, "nccl.pt"))
    a, b = runs["rccl"], runs["single"]
    assert a["orders"][0] == [] and a["orders"][2] == []
    assert sorted(a["orders"][1]) == sorted(a["orders"][3]) == list(range(a["nbuckets"])) and a["nbuckets"] >= 2
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    assert a["global_step"] == b["global_step"] == 3
    assert a["calls"] >= 2 and b["calls"] >= 2      # each window's second micro-batch went through the accumulate kernel
    for k in b["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), k
