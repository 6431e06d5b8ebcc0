"""Anomaly mode under data parallelism: two gloo ranks on one GPU (the pattern of test_00_parallel_gpu.py), the NaN source on rank 1
only.  The record is all-reduced (MIN) before the host reads it, so BOTH ranks raise AnomalyError naming the same node, before either
steps its optimizer.  The ranks must join within a time limit: a rank left waiting in a collective fails the test instead of hanging it.
Spawned before this pytest process touches the GPU, hence the file name."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import warnings
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd import synthetic
    from odvae_amd.trainer import AnomalyError, Trainer

    class Inject(torch.autograd.Function):
        """Identity on both ranks (same graph, same node numbering); its backward writes +Inf on rank 1 only."""
        @staticmethod
        def forward(ctx, x):
            return x.clone(memory_format=torch.preserve_format)

        @staticmethod
        def backward(ctx, g):
            if rank == 1:
                g = g.clone(memory_format=torch.preserve_format)
                g[(0,) * g.dim()] = float("inf")
            return g

    torch.manual_seed(1000 + rank)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32).to("cuda:0").train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,), bucket_mb=1.0, detect_anomaly=True)
    assert trainer.reducers is not None
    batch = synthetic.make_batch(2, 64, seed=50 + rank)
    model.injected_noise = synthetic.make_noise(2, 4, seed=70 + rank)
    losses = [trainer.training_batch(dict(batch, pose_6d=batch["pose_6d"].clone()), 0)[0].item()]     # clean step first
    before = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    dict(model.named_modules())["decoder.up.1.block.0.norm2"].register_forward_hook(lambda m, a, out: Inject.apply(out))
    res = {"losses": losses, "raised": False}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            trainer.training_batch(dict(batch, pose_6d=batch["pose_6d"].clone()), 1)
        except AnomalyError as e:
            res.update(raised=True, node=e.node, index=e.output_index, module=e.module, rank=e.rank, msg=str(e))
    torch.cuda.synchronize()
    res["global_step"] = model.global_step
    res["unchanged"] = all(torch.equal(v.detach().cpu(), before[k]) for k, v in model.named_parameters())
    torch.save(res, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_both_ranks_raise_when_one_rank_makes_a_nan(tmp_path):
    if torch.cuda.device_count() < 1:
        pytest.skip("no HIP device")
    if torch.cuda.is_initialized():
        pytest.skip("GPU already initialised in this process; run this file in its own pytest invocation")
    world, port = 2, _free_port()
    ctx = mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=False, start_method="spawn")
    deadline = time.time() + 600
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                pytest.fail("the ranks did not finish within 600 s (a rank waiting in a collective?)")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
                p.join(10)
    r = [torch.load(os.path.join(tmp_path, "rank%d.pt" % i)) for i in range(world)]
    for i, ri in enumerate(r):
        assert ri["raised"], i
        assert ri["rank"] == i and ri["global_step"] == 2 and ri["unchanged"], ri
        assert ri["msg"].startswith("Function '%s' returned nan values in its %dth output." % (ri["node"], ri["index"]))
        assert "rank %d of 2" % i in ri["msg"]
    assert (r[0]["node"], r[0]["index"], r[0]["module"]) == (r[1]["node"], r[1]["index"], r[1]["module"])
    assert r[0]["node"] != "Inject" + "Backward" and r[0]["module"].startswith("decoder.up.1.block.0")
