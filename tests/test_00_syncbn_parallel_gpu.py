"""sync_batchnorm under data parallelism: two ranks share the one GPU over gloo, exactly as tests/test_00_parallel_gpu.py runs them.

Rank 0 sees bright patches and rank 1 dark ones, so a rank's own BatchNorm statistics and those of the two together differ by far more
than any tolerance here.  The reference is the float64 oracle discriminator (oracle.losses.NLayerDiscriminator) on the CONCATENATED batch.

(a) the discriminator alone, f32 and bf16: logits and input gradient of each rank's rows, and the rank-summed parameter gradients, by
    the tolerances of the single-process discriminator tests (tests/test_gan_lpips_gpu.py: 1e-3 / 5e-3 of the reference's largest value;
    bf16: twice the CPU-autocast oracle's distance plus the floors of tests/test_disc_bf16_gpu.py).  The same run with the switch off has
    to fall outside them: the inputs tell the two apart.
(b) after that forward running_mean, running_var and num_batches_tracked hold the same bits on both ranks, and the oracle's values on
    the concatenated batch within gn_offset_inputs.FLOOR_FWD (bf16 activations: the 2e-2 of tests/test_disc_bf16_gpu.py).
(c) Trainer(optimizer_indices=(0, 1), sync_batchnorm=True), disc_factor 1, disc_start 0: the discriminator optimizer's gradient arena
    equals the arena of one process on the concatenated batch (rank 0 builds that twin), by the rule test_00_parallel_gpu.py has for
    the generator's; after two batches every discriminator parameter and buffer is bit-identical across the ranks.
(d) uneven shards, B = 3 and B = 1: merged statistics and logits match the concatenated batch (no gradient claim: DDP makes none).

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
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
BF = torch.bfloat16
WORLD = 2
JOIN_SECONDS = 240
SIZES = {"even": (2, 2), "uneven": (3, 1)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _images(rank, n, seed=0):
    """[n, 3, 64, 64] in [-1, 1]: rank 0 bright (0.4 .. 1), rank 1 dark (-1 .. -0.4)"""
    u = torch.rand(n, 3, 64, 64, generator=torch.Generator().manual_seed(900 + 10 * seed + rank))
    return (0.4 + 0.6 * u) if rank == 0 else (-1.0 + 0.6 * u)


def _logit_grads(sizes):
    g = torch.Generator().manual_seed(77)
    return list(torch.split(torch.randn(sum(sizes), 1, 6, 6, generator=g), list(sizes), 0))


def _oracle_disc():
    from odvae_amd.gan import weights_init
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(5)
    return RefD().apply(weights_init).train()


def _shard(rank, step=0):
    """tests/test_00_parallel_gpu.py's shard (a pixel at 0 and one at 1 per sample keeps `_rescale`'s batch min / max equal on a shard and
    on the concatenated batch), brightened on rank 0 and darkened on rank 1"""
    from odvae_amd import synthetic
    batch = synthetic.make_batch(2, 64, seed=50 + 10 * step + rank)
    p = batch["patch"]
    batch["patch"] = (0.6 + 0.4 * p) if rank == 0 else 0.4 * p
    batch["patch"][:, :, 0, 0] = 0.0
    batch["patch"][:, :, 0, 1] = 1.0
    return batch, synthetic.make_noise(2, 4, seed=70 + 10 * step + rank)


def _concat(parts):
    out = {}
    for k in parts[0]:
        v = [p[k] for p in parts]
        out[k] = torch.cat(v, 0) if torch.is_tensor(v[0]) else sum(v, [])
    return out


def _disc_arena(model, trainer, batch, noise):
    """Optimizer 1's training_step -> backward (-> bucketed all-reduce) as Trainer.training_batch does it, stopping before clip / step"""
    opt = trainer.optimizers[1]
    red = trainer.reducers[1] if trainer.reducers else None
    saved = trainer._toggle(1)
    try:
        model.injected_noise = noise
        loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 1)
        opt.zero_grad(set_to_none=True)
        if red is not None:
            red.prepare_for_backward()
            (loss * red.inv_world).backward()
            red.finish()
        else:
            loss.backward()
        opt.gather_grads()
    finally:
        trainer._untoggle(saved)
    torch.cuda.synchronize()
    return opt.flat_grad.detach().cpu().clone()


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd import synthetic
    from odvae_amd.gan import NLayerDiscriminator
    from odvae_amd.trainer import Trainer
    dev = "cuda:0"
    out = {}
    ref_state = _oracle_disc().state_dict()
    # ---- (a), (b), (d): the discriminator alone ---------------------------------------------------------------------------------
    for split, sizes in SIZES.items():
        gy = _logit_grads(sizes)[rank]
        for precision in ("f32", "bf16"):
            for switch in ((True, False) if split == "even" else (True,)):
                net = NLayerDiscriminator()
                net.load_state_dict(ref_state, strict=True)
                net = net.to(dev).train()
                if precision == "bf16":
                    net.set_precision("bf16")
                if switch:
                    for m in net.batchnorm_layers():
                        m.dist_group = dist.group.WORLD
                x = _images(rank, sizes[rank]).to(dev).requires_grad_(True)
                y = net(x)
                buffers = {k: v.detach().cpu().clone() for k, v in net.named_buffers()}
                res = {"y": y.detach().float().cpu(), "buffers": buffers}
                if split == "even":
                    y.backward(gy.to(dev))
                    res["dx"] = x.grad.detach().float().cpu()
                    res["grads"] = {k: p.grad.detach().float().cpu() for k, p in net.named_parameters()}
                out[(split, precision, switch)] = res
                del net
    # ---- (c): the trainer ----------------------------------------------------------------------------------------------------------
    build = lambda: synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=1.0, disc_factor=1.0, disc_start=0)
    torch.manual_seed(1000 + rank)       # different initial weights per rank: the broadcast aligns them
    model = build().to(dev).train()
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), sync_batchnorm=True, bucket_mb=1.0)
    layers = model.loss.discriminator.batchnorm_layers()
    assert len(layers) == 3 and all(m.dist_group is dist.group.WORLD for m in layers)
    model._global_step = 1
    if rank == 0:
        single = build()
        single.load_state_dict(model.state_dict())
        single = single.to(dev).train()
        t1 = Trainer(single, gradient_clip_val=1.0, optimizer_indices=(0, 1), distributed=False, sync_batchnorm=True)
        assert t1.reducers is None and all(m.dist_group is None for m in single.loss.discriminator.batchnorm_layers())
        single._global_step = 1
    batch, noise = _shard(rank)
    res = {"arena": _disc_arena(model, trainer, batch, noise)}
    if rank == 0:
        shards = [_shard(r) for r in range(world)]
        full_noise = {k: torch.cat([s[1][k] for s in shards], 0) for k in shards[0][1]}
        res["arena_full"] = _disc_arena(single, t1, _concat([s[0] for s in shards]), full_noise)
        name_of = {id(p): n for n, p in single.named_parameters()}
        res["names"] = [(name_of[id(p)], off, cnt) for p, off, cnt in t1.optimizers[1].param_slices()]
        del single, t1
    # two whole batches: both optimizers step; the ranks' discriminators must stay the same bits
    losses = []
    for step in range(2):
        batch, noise = _shard(rank, step)
        model.injected_noise = noise
        losses.append([l.item() for l in trainer.training_batch(batch, step)])
    torch.cuda.synchronize()
    res["losses"] = losses
    res["disc"] = {k: v.detach().cpu().clone() for k, v in model.loss.discriminator.state_dict().items()}
    out["trainer"] = res
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def _spawnable():
    if torch.cuda.device_count() < 1:
        pytest.skip("no HIP device")
    if torch.cuda.is_initialized():
        pytest.skip("GPU already initialised in this process; run this file in its own pytest invocation")


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """One two-rank run for every test of this file: [rank 0's results, rank 1's]"""
    _spawnable()
    out_dir = str(tmp_path_factory.mktemp("syncbn"))
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


# ---- the float64 oracle on the concatenated batch, once per split -----------------------------------------------------------------------
_ORACLE = {}


def _oracle(split):
    if split not in _ORACLE:
        import copy
        sizes = SIZES[split]
        x = torch.cat([_images(r, sizes[r]) for r in range(WORLD)], 0)
        gy = torch.cat(_logit_grads(sizes), 0)
        res = {}
        for kind in ("f64", "autocast"):
            net = copy.deepcopy(_oracle_disc())
            net = net.double() if kind == "f64" else net
            xr = x.to(torch.float64 if kind == "f64" else torch.float32).clone().requires_grad_(True)
            if kind == "autocast":
                with torch.autocast("cpu", dtype=BF):
                    y = net(xr)
            else:
                y = net(xr)
            y.float().backward(gy) if kind == "autocast" else y.backward(gy.double())
            res[kind] = {"y": y.detach().double(), "dx": xr.grad.detach().double(),
                         "grads": {k: p.grad.detach().double() for k, p in net.named_parameters()},
                         "buffers": {k: b.detach().clone() for k, b in net.named_buffers()}}
        _ORACLE[split] = res
    return _ORACLE[split]


def _gathered(ranks, key, split="even"):
    """the two ranks' results put together as the concatenated batch has them: rows concatenated, parameter gradients summed"""
    r0, r1 = ranks[0][key], ranks[1][key]
    out = {"y": torch.cat([r0["y"], r1["y"]], 0)}
    if "dx" in r0:
        out["dx"] = torch.cat([r0["dx"], r1["dx"]], 0)
        out["grads"] = {k: r0["grads"][k].double() + r1["grads"][k].double() for k in r0["grads"]}
    return out


def _failures(got, precision, split="even"):
    """names of the quantities outside the single-process discriminator tests' tolerances against the float64 oracle"""
    from test_bf16_model_gpu import rel
    ref, ac = _oracle(split)["f64"], _oracle(split)["autocast"]
    items = [("logits", got["y"], ref["y"], ac["y"], 1e-3, 2e-2)]
    if "dx" in got:
        items.append(("input gradient", got["dx"], ref["dx"], ac["dx"], 5e-3, 5e-2))
        items += [("grad " + k, got["grads"][k], ref["grads"][k], ac["grads"][k], 5e-3, 5e-2) for k in sorted(ref["grads"])]
    bad = []
    for name, g, want, autocast, tol32, floor16 in items:
        assert torch.isfinite(g).all(), name
        e = rel(g, want)
        bound = tol32 if precision == "f32" else 2 * rel(autocast, want) + floor16
        print("%-22s %s err %.3e bound %.3e" % (name, precision, e, bound))
        if not e <= bound:
            bad.append(name)
    return bad


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_discriminator_matches_float64_on_the_concatenated_batch(ranks, precision):
    on = _failures(_gathered(ranks, ("even", precision, True)), precision)
    assert not on, "sync_batchnorm on, outside the tolerances: %s" % on
    off = _failures(_gathered(ranks, ("even", precision, False)), precision)
    assert "logits" in off and "input gradient" in off and any(n.startswith("grad ") for n in off), \
        "with the switch off the run stays inside the tolerances (%s outside): these inputs do not tell the two apart" % off


@pytest.mark.parametrize("split", ["even", "uneven"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_running_statistics_are_the_same_bits_on_both_ranks_and_the_oracles(ranks, precision, split):
    import gn_offset_inputs as G
    from test_bf16_model_gpu import rel
    b0, b1 = (r[(split, precision, True)]["buffers"] for r in ranks)
    want = _oracle(split)["f64"]["buffers"]
    assert set(b0) == set(want) and len(b0) == 9
    for k in sorted(b0):
        assert b0[k].dtype == b1[k].dtype and torch.equal(b0[k], b1[k]), "%s differs between the ranks" % k
        if k.endswith("num_batches_tracked"):
            assert int(b0[k]) == 1 == int(want[k])
        elif precision == "f32":
            err, bound = G.maxerr(b0[k], want[k]), G.FLOOR_FWD * max(1.0, G.maxabs(want[k]))
            print("%s %s: err %.3e bound %.3e" % (split, k, err, bound))
            assert err <= bound, "%s: %.3e > %.3e" % (k, err, bound)
        else:
            assert rel(b0[k], want[k]) <= 2e-2, "%s: %.3e" % (k, rel(b0[k], want[k]))
    if split == "even":      # and without the switch each rank keeps its own: the inputs do differ
        o0, o1 = (r[(split, precision, False)]["buffers"] for r in ranks)
        assert not torch.equal(o0["main.3.running_mean"], o1["main.3.running_mean"])


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_uneven_shards_give_the_logits_of_the_concatenated_batch(ranks, precision):
    assert tuple(ranks[0][("uneven", precision, True)]["y"].shape) == (3, 1, 6, 6) and tuple(ranks[1][("uneven", precision, True)]["y"].shape) == (1, 1, 6, 6)
    bad = _failures(_gathered(ranks, ("uneven", precision, True), "uneven"), precision, "uneven")
    assert not bad, bad


def test_trainer_discriminator_arena_equals_one_process_on_the_concatenated_batch(ranks):
    t0, t1 = ranks[0]["trainer"], ranks[1]["trainer"]
    a0, a1, full = t0["arena"].double(), t1["arena"].double(), t0["arena_full"].double()
    assert torch.equal(a0, a1)                       # both ranks hold the same reduced arena
    gmax = full.abs().max().item()
    assert gmax > 0 and len(t0["names"]) == 13 and all(n.startswith("loss.discriminator.") for n, _, _ in t0["names"])
    worst = 0.0
    for name, off, n in t0["names"]:                 # the rule of tests/test_00_parallel_gpu.py (b)
        ref = full[off:off + n]
        err = (a0[off:off + n] - ref).abs().max().item()
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err / scale)
        assert err <= 2e-3 * scale, "%s: %.3e vs scale %.3e" % (name, err, scale)
    print("worst per-parameter deviation of the discriminator's arena: %.2e of its scale" % worst)


def test_trainer_keeps_the_ranks_discriminators_bit_identical(ranks):
    t0, t1 = ranks[0]["trainer"], ranks[1]["trainer"]
    assert t0["losses"] != t1["losses"] and all(torch.isfinite(torch.tensor(t["losses"])).all() for t in (t0, t1))
    assert len(t0["disc"]) == 22
    for k in t0["disc"]:
        assert torch.equal(t0["disc"][k], t1["disc"][k]), "loss.discriminator.%s differs between the ranks after two batches" % k
    assert int(t0["disc"]["main.3.num_batches_tracked"]) > 1
