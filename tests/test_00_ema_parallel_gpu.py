"""model.params.ema_decay under data parallelism: two ranks share the one GPU over gloo, exactly as tests/test_00_syncbn_parallel_gpu.py
runs them.  The ranks build the plain model from different seeds, so before the Trainer their weights and shadows differ; constructing
the Trainer broadcasts rank 0's parameters and then rank 0's shadow arenas, stray shadows, decay and num_updates.  From there every rank
computes its average from the same parameters with no communication: after two batches (different images per rank) the shadows and
num_updates of the two ranks hold the same bits.

The ranks are spawned BEFORE this pytest process touches the GPU (hence the file name), results come back through files, the parent
joins with a time limit and terminates the ranks when it passes; nothing is retried."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_plain.yaml")
SMALL = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
         "model.params.ddconfig.resolution=32", "model.params.ddconfig.z_channels=4", "model.params.embed_dim=4",
         "model.params.lossconfig.params.disc_start=0", "model.params.lossconfig.params.kl_weight=0.01", "model.params.ema_decay=0.999"]
WORLD = 2
JOIN_SECONDS = 180


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ema_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.model_ema.state_dict().items()}


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import warnings
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd import synthetic
    from odvae_amd.config import Config, instantiate_from_config
    from odvae_amd.trainer import Trainer
    config = Config.merge(Config.load(YAML), Config.from_dotlist(SMALL))
    torch.manual_seed(1000 + rank)       # different initial weights per rank: the broadcasts align them
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = instantiate_from_config(config.model)
    model.learning_rate = 2 * config.model.base_learning_rate
    model = model.to("cuda:0").train()
    if rank == 1:                        # and a counter that is not rank 0's
        model.model_ema.num_updates.fill_(5)
    out = {"built": _ema_state(model)}
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), bucket_mb=1.0)
    assert trainer.reducers is not None and len(model.model_ema.arenas) == 2
    out["constructed"] = _ema_state(model)
    out["params0"] = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if n in model.model_ema.m_name2s_name}
    losses = []
    for step in range(2):
        g = torch.Generator().manual_seed(500 + 10 * step + rank)
        model.injected_noise = {"posterior_eps": torch.randn(2, 4, 16, 16, generator=g)}
        losses.append([l.item() for l in trainer.training_batch(synthetic.make_image_batch(2, 32, seed=50 + 10 * step + rank), step)])
    torch.cuda.synchronize()
    out["losses"] = losses
    out["trained"] = _ema_state(model)
    out["params2"] = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if n in model.model_ema.m_name2s_name}
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """One two-rank run for every test of this file: [rank 0's results, rank 1's]"""
    if torch.cuda.device_count() < 1:
        pytest.skip("no HIP device")
    if torch.cuda.is_initialized():
        pytest.skip("GPU already initialised in this process; run this file in its own pytest invocation")
    out_dir = str(tmp_path_factory.mktemp("ema_parallel"))
    ctx = mp.spawn(_worker, args=(WORLD, _free_port(), out_dir), nprocs=WORLD, join=False)
    deadline = time.monotonic() + JOIN_SECONDS
    while not ctx.join(timeout=5):          # raises when a rank failed (and terminates the other)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            for p in ctx.processes:
                p.join(10)
            pytest.fail("the two ranks did not finish within %d s: terminated, not retried" % JOIN_SECONDS)
    return [torch.load(os.path.join(out_dir, "rank%d.pt" % r)) for r in range(WORLD)]


def _bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_the_ranks_start_apart(ranks):
    b0, b1 = ranks[0]["built"], ranks[1]["built"]
    assert set(b0) == set(b1) and len(b0) > 50
    assert not torch.equal(b0["encoderconv_inweight"], b1["encoderconv_inweight"])
    assert int(b0["num_updates"]) == 0 and int(b1["num_updates"]) == 5


def test_construction_gives_every_rank_rank_0s_average(ranks):
    c0, c1, built = ranks[0]["constructed"], ranks[1]["constructed"], ranks[0]["built"]
    for k in c0:
        assert _bits(c0[k], c1[k]), "model_ema.%s differs between the ranks after Trainer construction" % k
        assert _bits(c0[k], built[k]), "model_ema.%s is not what rank 0 built" % k
    assert int(c1["num_updates"]) == 0
    assert all(_bits(ranks[0]["params0"][n], ranks[1]["params0"][n]) for n in ranks[0]["params0"])


def test_two_batches_keep_the_averages_bit_identical(ranks):
    t0, t1 = ranks[0]["trained"], ranks[1]["trained"]
    assert ranks[0]["losses"] != ranks[1]["losses"]                        # different images per rank
    assert all(torch.isfinite(torch.tensor(r["losses"])).all() for r in ranks)
    for k in t0:
        assert _bits(t0[k], t1[k]), "model_ema.%s differs between the ranks after two batches" % k
    assert int(t0["num_updates"]) == 2 == int(t1["num_updates"])
    assert all(_bits(ranks[0]["params2"][n], ranks[1]["params2"][n]) for n in ranks[0]["params2"])
    moved = [k for k in t0 if k not in ("decay", "num_updates") and not torch.equal(t0[k], ranks[0]["constructed"][k])]
    assert len(moved) > 50
    import ema_ref as E
    assert not torch.equal(t0["encoderconv_inweight"], ranks[0]["params2"]["encoder.conv_in.weight"]) and E.shadow_name("encoder.conv_in.weight") in t0
