"""lightning.trainer.accumulate_grad_batches = N (PL-1.9 automatic optimisation, two optimizers) on CPU: the Trainer and the GradReducer are
device-agnostic, so a small two-optimizer torch module with torch.optim.Adam drives them here, as in tests/test_parallel_gloo.py.
Window = N batches; zero_grad before the window's first backward only; every backward runs on loss / N; clip + step + global_step on the last
batch of the window (or of the epoch); no gradient exchange before the window's last backward, which carries the accumulated local sums of every
bucket touched anywhere in the window."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class TinyNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(8, 64)
        self.b = nn.Linear(64, 64)
        self.c = nn.Linear(64, 64)
        self.d = nn.Linear(64, 4)

    def forward(self, x):
        return self.d(torch.tanh(self.c(torch.tanh(self.b(torch.tanh(self.a(x)))))))


class TinyLightning(nn.Module):
    """Two-optimizer module with the surface Trainer uses.  `side` (in the generator's optimizer) joins the loss only while
    `side_batches` contains the batch index: a parameter that only some micro-batches of a window reach."""

    def __init__(self, side_batches=()):
        super().__init__()
        self.gen, self.disc = TinyNet(), TinyNet()
        self.side = nn.Linear(8, 4)
        self.side_batches = tuple(side_batches)
        self._global_step = 0
        self.learning_rate = 1e-2
        self.seen_global_steps = []

    @property
    def global_step(self):
        return self._global_step

    def training_step(self, batch, batch_idx, optimizer_idx):
        x, y = batch
        self.seen_global_steps.append((batch_idx, optimizer_idx, self._global_step))
        if optimizer_idx == 0:
            out = self.gen(x)
            if batch_idx in self.side_batches:
                out = out + self.side(x)
            return ((out - y) ** 2).mean()
        return (self.disc(x) ** 2).mean()

    def configure_optimizers(self):
        return [torch.optim.Adam(list(self.gen.parameters()) + list(self.side.parameters()), lr=self.learning_rate, betas=(0.5, 0.9)),
                torch.optim.Adam(self.disc.parameters(), lr=self.learning_rate, betas=(0.5, 0.9))], []


def _batches(n, seed=5, rows=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 8, generator=g), torch.randn(rows, 4, generator=g)) for _ in range(n)]


def _hand_loop(model, batches, n_acc, clip=1.0, closes=None):
    """The PL-1.9 loop written out: per batch and optimizer index training_step, zero_grad at the window start, (loss / N).backward(), and on the
    window's last batch clip_grad_norm_ + step + global_step.  `closes`: batch indices that end a window early (the epoch's last batch)."""
    opts, _ = model.configure_optimizers()
    losses, pos = [], 0
    for i, batch in enumerate(batches):
        final = pos + 1 == n_acc or (closes is not None and i in closes)
        row = []
        for idx in (0, 1):
            other = [p for g in opts[1 - idx].param_groups for p in g["params"]]
            for p in other:
                p.requires_grad = False
            loss = model.training_step(batch, i, idx)
            if pos == 0:
                opts[idx].zero_grad(set_to_none=True)
            (loss if n_acc == 1 else loss / n_acc).backward()
            if final:
                torch.nn.utils.clip_grad_norm_([p for g in opts[idx].param_groups for p in g["params"]], clip)
                opts[idx].step()
                model._global_step += 1
            for p in other:
                p.requires_grad = True
            row.append(loss.detach())
        losses.append(row)
        pos = 0 if final else pos + 1
    return losses


def _pair(**kw):
    torch.manual_seed(11)
    a = TinyLightning(**kw)
    b = TinyLightning(**kw)
    b.load_state_dict(a.state_dict())
    return a, b


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_window_of_two_is_the_hand_written_pl_loop():
    from odvae_amd.trainer import Trainer
    model, ref = _pair(side_batches=(0, 3))      # `side` is reached by the first micro-batch of window 0 and the last of window 1 only
    batches = _batches(4)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), accumulate_grad_batches=2, distributed=False)
    want = _hand_loop(ref, batches, 2)
    got = []
    for i, b in enumerate(batches):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        got.append(trainer.training_batch(b, i))
        changed = any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
        assert changed == (i in (1, 3)), i                      # nothing moves after batches 0 and 2
        assert trainer.accumulation_index == (1 if i in (0, 2) else 0)
    assert _same(model, ref)
    assert model._global_step == ref._global_step == 4
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))      # unscaled losses
    # every micro-batch of a window sees the window's global_step (optimizer 1 of the closing batch sees optimizer 0's step, as in PL)
    assert model.seen_global_steps == ref.seen_global_steps
    assert [s for (_, idx, s) in model.seen_global_steps if idx == 0] == [0, 0, 2, 2]


def test_fit_closes_a_partial_window_at_the_end_of_the_epoch(tmp_path):
    from odvae_amd.trainer import Trainer
    model, ref = _pair()
    batches = _batches(3)
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), accumulate_grad_batches=2, distributed=False)
    out = trainer.fit(batches)
    want = _hand_loop(ref, batches, 2, closes={2})               # the second step: one micro-batch, still scaled by 1/2
    assert len(out) == 3 and model._global_step == ref._global_step == 4      # two steps of each optimizer
    assert _same(model, ref)
    assert all(torch.equal(a, b) for g, w in zip(out, want) for a, b in zip(g, w))
    assert trainer.accumulation_index == 0
    # the max_batches cut closes the window too
    model2, ref2 = _pair()
    t2 = Trainer(model2, gradient_clip_val=1.0, optimizer_indices=(0, 1), accumulate_grad_batches=2, distributed=False)
    t2.fit(_batches(5), max_batches=3)
    _hand_loop(ref2, _batches(5)[:3], 2, closes={2})
    assert _same(model2, ref2) and t2.accumulation_index == 0
    # a checkpoint inside an open window would silently drop its gradients
    trainer.training_batch(batches[0], 0)
    assert trainer.accumulation_index == 1
    with pytest.raises(RuntimeError, match="window"):
        trainer.save_checkpoint(str(tmp_path / "open.ckpt"))
    with pytest.raises(RuntimeError, match="window"):
        trainer.dump_checkpoint()
    trainer.training_batch(batches[1], 1)
    trainer.save_checkpoint(str(tmp_path / "closed.ckpt"))
    trainer.training_batch(batches[2], 2)
    trainer.load_checkpoint(str(tmp_path / "closed.ckpt"))       # closes the window
    assert trainer.accumulation_index == 0


@pytest.mark.parametrize("explicit", [False, True])
def test_default_is_a_step_after_every_batch(explicit):
    from odvae_amd.trainer import Trainer
    model, ref = _pair()
    batches = _batches(3)
    kw = {"accumulate_grad_batches": 1} if explicit else {}
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), distributed=False, **kw)
    got = [trainer.training_batch(b, i) for i, b in enumerate(batches)]
    want = _hand_loop(ref, batches, 1)
    assert _same(model, ref) and model._global_step == 6
    assert all(torch.equal(a, b) for g, w in zip(got, want) for a, b in zip(g, w))
    assert trainer.accumulation_index == 0


@pytest.mark.parametrize("bad", [0, -1, 2.5])
def test_accumulate_grad_batches_must_be_a_positive_integer(bad):
    from odvae_amd.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(TinyLightning(), accumulate_grad_batches=bad, distributed=False)


def test_runner_maps_the_yaml_key():
    from odvae_amd import run
    from odvae_amd.config import Config, configure_learning_rate

    class M:
        pass
    config = Config.load(YAML)
    tc = config.lightning.trainer
    assert run.trainer_kwargs(tc) == {"gradient_clip_val": 1.0, "precision": 32, "detect_anomaly": True}      # the untouched yaml: no accumulation key
    lr1 = configure_learning_rate(config, M(), tc, ngpu=1).learning_rate
    assert run.trainer_kwargs(tc) == {"gradient_clip_val": 1.0, "precision": 32, "detect_anomaly": True}
    config4 = Config.merge(Config.load(YAML), Config.from_dotlist(["lightning.trainer.accumulate_grad_batches=4"]))
    tc4 = config4.lightning.trainer
    kw = run.trainer_kwargs(tc4)
    assert kw["accumulate_grad_batches"] == 4 and isinstance(kw["accumulate_grad_batches"], int)
    assert {k: v for k, v in kw.items() if k != "accumulate_grad_batches"} == run.trainer_kwargs(tc)
    lr4 = configure_learning_rate(config4, M(), tc4, ngpu=1).learning_rate
    assert lr4 == 4 * lr1 > 0


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------------
def _shards():
    """Four shards: (window micro-batch m, rank r) -> index 2 * m + r."""
    return _batches(4, seed=9)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd.trainer import Trainer
    torch.manual_seed(100 + rank)            # different init per rank: the broadcast aligns them
    model = TinyLightning(side_batches=(0,))                     # `side`: reached by the window's FIRST micro-batch only
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), bucket_mb=0.02, accumulate_grad_batches=2)
    reds = trainer.reducers
    assert reds is not None and len(reds[0].buckets) >= 2
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    shards = _shards()
    trainer.training_batch(shards[0 + rank], 0)
    out = {"sd0": sd0, "order_mid": [list(r.launch_order) for r in reds],
           "grads_mid": {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
           "unchanged_mid": all(torch.equal(sd0[k], v) for k, v in model.state_dict().items()), "index_mid": trainer.accumulation_index}
    trainer.training_batch(shards[2 + rank], 1)
    side_bucket = reds[0].param_bucket[[i for i, (p, _, _) in enumerate(reds[0].slices) if p is model.side.weight][0]]
    out.update({"sd": {k: v.clone() for k, v in model.state_dict().items()}, "order_end": [list(r.launch_order) for r in reds],
                "nbuckets": [len(r.buckets) for r in reds], "side_bucket": side_bucket, "global_step": model._global_step,
                "side_grad": model.side.weight.grad.clone(), "index_end": trainer.accumulation_index})
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_two_gloo_ranks_exchange_once_per_window(tmp_path):
    from odvae_amd.trainer import Trainer
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    for k in r0["sd0"]:
        assert torch.equal(r0["sd0"][k], r1["sd0"][k]), k
    # non-final micro-batch: nothing exchanged, nothing stepped, the ranks hold their own (different) gradients
    for r in (r0, r1):
        assert r["order_mid"] == [[], []] and r["unchanged_mid"] and r["index_mid"] == 1
    assert any(not torch.equal(r0["grads_mid"][n], r1["grads_mid"][n]) for n in r0["grads_mid"])
    assert "side.weight" in r0["grads_mid"]
    # end of the window: every bucket touched in the window travelled -- the one of `side` too, which the last backward did not reach
    for r in (r0, r1):
        assert [sorted(o) for o in r["order_end"]] == [list(range(n)) for n in r["nbuckets"]]
        assert r["side_bucket"] in r["order_end"][0] and r["global_step"] == 2 and r["index_end"] == 0
    assert torch.equal(r0["side_grad"], r1["side_grad"]) and r0["side_grad"].abs().max() > 0
    for k in r0["sd"]:
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k
    assert not torch.equal(r0["sd"]["side.weight"], r0["sd0"]["side.weight"])
    # one process accumulating all four shards: mean over ranks of the per-rank window means = 1/4 of the sum of the shard gradients
    ref = TinyLightning(side_batches=(0,))
    ref.load_state_dict(r0["sd0"])
    single = Trainer(ref, gradient_clip_val=1.0, optimizer_indices=(0, 1), accumulate_grad_batches=4, distributed=False)
    shards = _shards()
    for j, (i, b) in enumerate([(0, shards[0]), (0, shards[1]), (1, shards[2]), (1, shards[3])]):
        single.training_batch(b, i)
    assert ref._global_step == 2
    sd = ref.state_dict()
    for k in sd:
        # 1e-6 relative to the tensor's scale (its largest entry): an Adam step moves every weight by about lr whatever its size, so the f32
        # rounding of the update is not proportional to the single element
        assert (r0["sd"][k] - sd[k]).abs().max().item() <= 1e-6 * sd[k].abs().max().item(), k
