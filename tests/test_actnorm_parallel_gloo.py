"""ActNorm across data-parallel ranks, on the host: two gloo ranks hold ActNorm layers with different loc / scale, rank 0 "initialised"
and rank 1 not; after `parallel.broadcast_actnorm` both hold rank 0's loc, scale and initialized = 1 (the buffer and its host-side
mirror).  Upstream initialises per rank and never reconciles the replicas: DESIGN.md 6."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd.gan import ActNormLReLU
    from odvae_amd.parallel import broadcast_actnorm
    g = torch.Generator().manual_seed(50 + rank)
    layers = [ActNormLReLU(8), ActNormLReLU(4)]
    with torch.no_grad():
        for m in layers:
            m.loc.copy_(torch.randn(m.loc.shape, generator=g))
            m.scale.copy_(torch.rand(m.scale.shape, generator=g) + 0.5)
            if rank == 0:
                m.initialized.fill_(1)
            m.refresh_initialized()
    before = [(m.loc.detach().clone(), m.scale.detach().clone(), int(m.initialized), m._initialized_host) for m in layers]
    broadcast_actnorm(layers, dist.group.WORLD)
    after = [(m.loc.detach().clone(), m.scale.detach().clone(), int(m.initialized), m._initialized_host) for m in layers]
    torch.save({"before": before, "after": after}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_broadcast_gives_every_rank_rank_zeros_actnorm(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    for k in range(2):
        b0, b1, a0, a1 = r0["before"][k], r1["before"][k], r0["after"][k], r1["after"][k]
        assert not torch.equal(b0[0], b1[0]) and not torch.equal(b0[1], b1[1])
        assert (b0[2], b0[3], b1[2], b1[3]) == (1, True, 0, False)
        for a in (a0, a1):
            assert torch.equal(a[0], b0[0]) and torch.equal(a[1], b0[1]) and a[2] == 1 and a[3] is True


def test_broadcast_is_a_no_op_without_a_process_group():
    from odvae_amd.gan import ActNormLReLU
    from odvae_amd.parallel import broadcast_actnorm
    m = ActNormLReLU(4)
    broadcast_actnorm([m], None)
    assert int(m.initialized) == 0 and not m._initialized_host
