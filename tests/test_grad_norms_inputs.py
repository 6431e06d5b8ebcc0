"""track_grad_norm / gradient_clip_algorithm on the CPU: the float64 reference and the host model of the segmented-norm kernel agree on the
cases the GPU tests run, every planted fault is rejected by one of those cases, both Trainer arguments are validated, the runner passes the
yaml keys on only when they are set, and the torch fallback path (torch.optim.Adam: p.grad.norm, clip_grad_value_) logs the right keys
and values -- alone, over two gloo ranks and over an accumulation window."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import grad_norms_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
NORMS = [1, 2, "inf", 0.5, 3]


def _edge_case(seed=1):
    lengths = gi.EDGE_LENGTHS
    offs, total = gi.layout(lengths, lead=64)
    return lengths, offs, gi.fill(lengths, offs, total, gi.whole_numbers(seed))


# ---- reference and host model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", NORMS)
def test_host_model_is_the_reference_on_the_edge_lengths(p):
    lengths, offs, arena = _edge_case()
    counts = [i % 3 != 1 for i in range(len(lengths))]
    want = gi.reference(arena, offs, lengths, counts, p)
    got = gi.host_model(arena, offs, lengths, counts, p)
    assert np.isfinite(want).all()                                   # no canary reached any result
    if p in (1, 2, "inf"):
        assert gi.same_bits(got[:-1], want[:-1])
        assert gi.ulps(got[-1:], want[-1:]).max() <= (1 if p == 2 else 0)
    else:
        assert gi.ulps(got, want).max() <= 2
    # the torch spelling of the same thing
    t = torch.from_numpy(arena)
    norm = float("inf") if p == "inf" else p
    per = torch.stack([t[o:o + n].double().norm(norm).float() for o, n in zip(offs, lengths)])
    assert gi.ulps(per.numpy(), want[:-1]).max() <= (0 if p in (1, "inf") else 2)
    tot = per[torch.tensor(counts)].double().norm(norm).float()
    assert gi.ulps(tot.numpy().reshape(1), want[-1:]).max() <= 2


@pytest.mark.parametrize("n_seg", [1, 129, 357])
def test_host_model_crosses_launch_tables(n_seg):
    rng = np.random.RandomState(n_seg)
    lengths = [int(v) for v in rng.choice(gi.EDGE_LENGTHS[:8] + [257, 1000], size=n_seg)]
    offs, total = gi.layout(lengths, gap=0)
    arena = gi.fill(lengths, offs, total, gi.whole_numbers(n_seg))
    for p in (1, 2, "inf"):
        want = gi.reference(arena, offs, lengths, None, p)
        assert gi.same_bits(gi.host_model(arena, offs, lengths, None, p)[:-1], want[:-1])
        assert gi.same_bits(gi.host_model(arena, offs, lengths, None, p, segs_per_launch=7)[:-1], want[:-1])      # any table size


def test_l2_total_is_exact_on_perfect_squares():
    lengths = [1, 3, 64, 65, 4097]
    offs, total = gi.layout(lengths)
    arena = gi.fill(lengths, offs, total, lambda i, n: gi.perfect_square_segment(n, i + 1))
    want = gi.reference(arena, offs, lengths, None, 2)
    assert list(want[:-1]) == [1.0, 10.0, 15.0, 20.0, 25.0]
    assert want[-1] == np.float32(np.sqrt(1 + 100 + 225 + 400 + 625.0))
    assert gi.same_bits(gi.host_model(arena, offs, lengths, None, 2), want)


# ---- planted faults: each is rejected by a case the GPU test runs ----------------------------------------------------------------------------
def _fault_cases():
    """fault -> (arena, offs, lengths, counts, p) on which the faulty model must leave the reference."""
    cases = {}
    big = (1 << 24) + 8
    offs, total = gi.layout([big])
    cases["f32_accumulate"] = (gi.fill([big], offs, total, lambda i, n: np.ones(n, dtype=np.float32)), offs, [big], None, 1)
    lengths, offs, arena = _edge_case()
    cases["read_padding"] = (arena, offs, lengths, None, 2)          # NaN canaries in every gap
    cases["one_short"] = (np.where(np.isnan(arena), arena, np.float32(1.0)).astype(np.float32), offs, lengths, None, 1)
    nan_arena = arena.copy()
    nan_arena[offs[4] + 17] = np.nan
    nan_arena[offs[4] + 18] = 100.0                                  # a larger value after the NaN: fmax forgets it
    cases["max_drops_nan"] = (nan_arena, offs, lengths, None, "inf")
    l2, o2 = [2, 1], [0, 64]
    a2 = np.zeros(256, dtype=np.float32)
    a2[0], a2[1], a2[64] = 16777216.0, 1.0, 1.0                      # L1: f32(16777217) + 1 rounds to 2^24, 16777218 does not
    cases["total_unrounded"] = (a2, o2, l2, None, 1)
    cases["noncounting_in_total"] = (nan_arena, offs, lengths, [i != 4 for i in range(len(lengths))], 2)
    return cases


@pytest.mark.parametrize("fault", gi.FAULTS)
def test_planted_fault_is_rejected(fault):
    arena, offs, lengths, counts, p = _fault_cases()[fault]
    want = gi.reference(arena, offs, lengths, counts, p)
    assert gi.same_bits(gi.host_model(arena, offs, lengths, counts, p), want)
    assert not gi.same_bits(gi.host_model(arena, offs, lengths, counts, p, fault=fault), want)


def test_f32_running_sum_misses_the_big_segment_and_float64_does_not():
    arena, offs, lengths, _, _ = _fault_cases()["f32_accumulate"]
    assert gi.reference(arena, offs, lengths, None, 1)[0] == np.float32(16777224.0)
    assert gi.host_model(arena, offs, lengths, None, 1, fault="f32_accumulate")[0] == np.float32(16777216.0)


def test_nonfinite_rules_of_the_reference():
    lengths, offs, arena = _edge_case()
    a = arena.copy()
    a[offs[3] + 2] = np.nan
    a[offs[5] + 7] = np.inf
    a[offs[6] + 7] = -np.inf
    a[offs[7]:offs[7] + lengths[7]] = 0.0
    for p in NORMS:
        r = gi.reference(a, offs, lengths, None, p)
        assert np.isnan(r[3]) and np.isnan(r[-1]) and r[5] == np.inf and r[6] == np.inf and r[7] == 0.0
        assert np.isfinite(np.delete(r[:-1], [3, 5, 6])).all()
        assert gi.ulps(gi.host_model(a, offs, lengths, None, p), r).max() <= 2
        quiet = gi.reference(a, offs, lengths, [i not in (3, 5, 6) for i in range(len(lengths))], p)
        assert np.isfinite(quiet[-1]) and np.isnan(quiet[3])
    assert torch.isnan(torch.tensor([float("nan"), 1.0, -3.0]).norm(float("inf")))


def test_clamp_model_is_torch_clamp_and_the_fmin_fmax_fault_is_rejected():
    c = 0.75
    for n in (1, 3, 4, 5, 1023, 1025):
        for seed in range(4):
            g = gi.clamp_inputs(n, seed, c)
            want = torch.clamp(torch.from_numpy(g), -c, c).numpy()
            assert gi.same_bits(gi.clamp_model(g, c), want)
            assert np.array_equal(np.signbit(gi.clamp_model(g, c)), np.signbit(want)) or np.isnan(g).any()
    g = gi.clamp_inputs(1025, 0, c)
    assert np.isnan(g).any() and np.isinf(g).any() and (np.abs(g[g != 0]) < 1e-38).any()
    want = torch.clamp(torch.from_numpy(g), -c, c).numpy()
    assert np.isnan(want).sum() == np.isnan(g).sum() and np.abs(want[~np.isnan(want)]).max() == np.float32(c)
    assert not gi.same_bits(gi.clamp_model(g, c, fault="nan_to_c"), want)
    z = torch.clamp(torch.tensor([-0.0]), -c, c)
    assert z.item() == 0.0 and np.signbit(z.numpy())[0]


# ---- Trainer arguments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [True, False, 0, 0.0, -2, -0.5, float("nan"), "2", "INF", "max", None, [2]])
def test_track_grad_norm_is_validated(bad):
    from odvae_amd.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(gi.TinyLightning(), track_grad_norm=bad, distributed=False)


@pytest.mark.parametrize("good, want", [(-1, None), (-1.0, None), (2, 2.0), (1, 1.0), (0.5, 0.5), (3.0, 3.0), ("inf", float("inf")),
                                        (float("inf"), float("inf"))])
def test_track_grad_norm_values(good, want):
    from odvae_amd.trainer import Trainer
    assert Trainer(gi.TinyLightning(), track_grad_norm=good, distributed=False).track_grad_norm == want


def test_gradient_clip_algorithm_is_validated():
    from odvae_amd.trainer import Trainer
    for bad in ("Value", "clamp", "", 1, True):
        with pytest.raises(ValueError):
            Trainer(gi.TinyLightning(), gradient_clip_val=1.0, gradient_clip_algorithm=bad, distributed=False)
    for clip in (None, 0, 0.0):
        with pytest.raises(ValueError):
            Trainer(gi.TinyLightning(), gradient_clip_val=clip, gradient_clip_algorithm="value", distributed=False)
    for ok in (None, "norm", "value"):
        assert Trainer(gi.TinyLightning(), gradient_clip_val=1.0, gradient_clip_algorithm=ok, distributed=False).gradient_clip_algorithm == ok
    import inspect
    names = list(inspect.signature(Trainer.__init__).parameters)
    assert names[-2:] == ["gradient_clip_algorithm", "track_grad_norm"]      # last: positional callers are unaffected


def test_runner_passes_the_keys_on_only_when_the_yaml_sets_them():
    from odvae_amd import run
    from odvae_amd.config import Config
    tc = Config.load(YAML).lightning.trainer
    assert run.trainer_kwargs(tc) == {"gradient_clip_val": 1.0, "precision": 32, "detect_anomaly": True}
    for dot, key, want in [("lightning.trainer.track_grad_norm=2", "track_grad_norm", 2),
                           ("lightning.trainer.track_grad_norm=inf", "track_grad_norm", float("inf")),
                           ("lightning.trainer.track_grad_norm=-1", "track_grad_norm", -1),
                           ("lightning.trainer.gradient_clip_algorithm=value", "gradient_clip_algorithm", "value"),
                           ("lightning.trainer.gradient_clip_algorithm=norm", "gradient_clip_algorithm", "norm")]:
        cfg = Config.merge(Config.load(YAML), Config.from_dotlist([dot]))
        kw = run.trainer_kwargs(cfg.lightning.trainer)
        assert kw[key] == want or (key == "track_grad_norm" and kw[key] == "inf"), (dot, kw)
        assert {k: v for k, v in kw.items() if k != key} == run.trainer_kwargs(tc)
        from odvae_amd.trainer import Trainer
        t = Trainer(gi.TinyLightning(), distributed=False, gradient_clip_val=kw["gradient_clip_val"],
                    **{k: v for k, v in kw.items() if k in ("track_grad_norm", "gradient_clip_algorithm")})      # and the Trainer takes what comes out
        if key == "track_grad_norm":
            assert t.track_grad_norm == (None if want == -1 else float(want))
    both = Config.merge(Config.load(YAML), Config.from_dotlist(["lightning.trainer.track_grad_norm=2", "lightning.trainer.gradient_clip_algorithm=value"]))
    assert set(run.trainer_kwargs(both.lightning.trainer)) == {"gradient_clip_val", "precision", "detect_anomaly", "track_grad_norm", "gradient_clip_algorithm"}


# ---- the torch fallback path -------------------------------------------------------------------------------------------------------------
def _hand_norms(model, opt, p):
    names = {id(q): n for n, q in model.named_parameters()}
    ps = [q for g in opt.param_groups for q in g["params"] if q.grad is not None]
    vals = [q.grad.detach().norm(p) for q in ps]
    d = {"grad_%s_norm/%s" % (float(p), names[id(q)]): v for q, v in zip(ps, vals)}
    d["grad_%s_norm_total" % float(p)] = torch.stack(vals).norm(p)
    return d


@pytest.mark.parametrize("p", [2, "inf", 1])
def test_fallback_path_logs_the_reached_parameters_of_the_stepped_optimizer(p):
    from odvae_amd.trainer import Trainer
    torch.manual_seed(3)
    model = gi.TinyLightning(side_batches=(1,))
    trainer = Trainer(model, gradient_clip_val=1e-3, track_grad_norm=p, distributed=False)
    pf = float(p)
    batches = gi.tiny_batches(2)
    trainer.training_batch(batches[0], 0)
    assert len(model.logs) == 2                                       # one log_dict per optimizer step
    gen = ["gen.0.weight", "gen.0.bias", "gen.2.weight", "gen.2.bias"]
    disc = ["disc.0.weight", "disc.0.bias", "disc.2.weight", "disc.2.bias"]
    assert list(model.logs[0]) == ["grad_%s_norm/%s" % (pf, n) for n in gen] + ["grad_%s_norm_total" % pf]      # no side.*, no idle.*, no disc.*
    assert list(model.logs[1]) == ["grad_%s_norm/%s" % (pf, n) for n in disc] + ["grad_%s_norm_total" % pf]
    assert {2: "grad_2.0_norm/gen.0.weight", "inf": "grad_inf_norm_total", 1: "grad_1.0_norm_total"}[p] in model.logs[0]      # the spelling, literally
    # the values are the UNCLIPPED norms: the gradients left in .grad were clipped to 1e-3 afterwards, so recompute from a twin
    torch.manual_seed(3)
    twin = gi.TinyLightning(side_batches=(1,))
    opts, _ = twin.configure_optimizers()
    for idx in (0, 1):
        for q in twin.parameters():
            q.grad = None
        other = [q for g in opts[1 - idx].param_groups for q in g["params"]]
        for q in other:
            q.requires_grad = False                                   # PL's toggle_optimizer
        twin.training_step(batches[0], 0, idx).backward()
        for q in other:
            q.requires_grad = True
        want = _hand_norms(twin, opts[idx], pf)
        assert list(want) == list(model.logs[idx])
        for k in want:
            assert torch.equal(want[k], model.logs[idx][k]), k
        assert float(want["grad_%s_norm_total" % pf]) > 1e-3            # above the clip: a clipped norm would read 1e-3
    names, vec = trainer.grad_norms[1]
    assert names == disc and vec.shape == (5,) and torch.equal(vec[-1], model.logs[1]["grad_%s_norm_total" % pf])
    assert trainer.grad_norms[0][0] == gen                           # optimizer 1 did not overwrite optimizer 0's
    trainer.training_batch(batches[1], 1)                             # batch 1 reaches `side`
    assert "grad_%s_norm/side.weight" % pf in model.logs[2] and "grad_%s_norm/side.bias" % pf in model.logs[2]
    assert not any("idle" in k for k in model.logs[2])


def test_tracking_changes_no_bit_and_off_logs_nothing():
    from odvae_amd.trainer import Trainer
    sds = []
    for track in (-1, 2):
        torch.manual_seed(4)
        model = gi.TinyLightning()
        trainer = Trainer(model, gradient_clip_val=1.0, track_grad_norm=track, distributed=False)
        for i, b in enumerate(gi.tiny_batches(3)):
            trainer.training_batch(b, i)
        assert len(model.logs) == (0 if track == -1 else 6)
        sds.append(model.state_dict())
    assert all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])


def test_value_clipping_on_the_fallback_path_is_clip_grad_value():
    from odvae_amd.trainer import Trainer
    c = 2e-2
    torch.manual_seed(5)
    model = gi.TinyLightning()
    torch.manual_seed(5)
    ref = gi.TinyLightning()
    trainer = Trainer(model, gradient_clip_val=c, gradient_clip_algorithm="value", track_grad_norm="inf", distributed=False)
    batches = gi.tiny_batches(2)
    for i, b in enumerate(batches):
        trainer.training_batch(b, i)
    opts, _ = ref.configure_optimizers()
    for i, b in enumerate(batches):
        for idx in (0, 1):
            other = [q for g in opts[1 - idx].param_groups for q in g["params"]]
            for q in other:
                q.requires_grad = False
            loss = ref.training_step(b, i, idx)
            opts[idx].zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_value_([q for g in opts[idx].param_groups for q in g["params"]], c)
            opts[idx].step()
            for q in other:
                q.requires_grad = True
    a, b = model.state_dict(), ref.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert max(float(d["grad_inf_norm_total"]) for d in model.logs) > c      # the clamp did bite, and the log shows the unclipped maximum


def test_accumulation_window_of_three_logs_once_on_the_sums():
    from odvae_amd.trainer import Trainer
    torch.manual_seed(6)
    model = gi.TinyLightning(side_batches=(0,))
    torch.manual_seed(6)
    twin = gi.TinyLightning(side_batches=(0,))
    trainer = Trainer(model, track_grad_norm=2, accumulate_grad_batches=3, distributed=False)
    batches = gi.tiny_batches(3)
    for i, b in enumerate(batches[:2]):
        trainer.training_batch(b, i)
        assert model.logs == [] and trainer.grad_norms == {}
    trainer.training_batch(batches[2], 2)
    assert len(model.logs) == 2
    for q in twin.parameters():
        q.grad = None
    for i, b in enumerate(batches):
        (twin.training_step(b, i, 0) / 3).backward()
    for k, v in model.logs[0].items():
        if "/" in k:
            assert torch.equal(v, twin.get_parameter(k.split("/", 1)[1]).grad.norm(2.0)), k
    assert "grad_2.0_norm/side.weight" in model.logs[0]               # reached by the window's first micro-batch only: still in the sums


# ---- two gloo ranks: the norms are of the reduced gradients -------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from odvae_amd.trainer import Trainer
    torch.manual_seed(100 + rank)
    model = gi.TinyLightning()
    trainer = Trainer(model, gradient_clip_val=1.0, track_grad_norm=2, bucket_mb=0.02)
    trainer.training_batch(gi.tiny_batches(2, seed=9)[rank], 0)
    torch.save({"logs": model.logs, "vec": [trainer.grad_norms[i][1] for i in (0, 1)],
                "grads": {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_two_gloo_ranks_log_identical_norms_of_the_reduced_gradients(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    assert len(r0["logs"]) == 2 and [list(d) for d in r0["logs"]] == [list(d) for d in r1["logs"]]
    for d0, d1 in zip(r0["logs"], r1["logs"]):
        for k in d0:
            assert torch.equal(d0[k], d1[k]), k
            # (the reducer hands every parameter of its optimizer a slice of the reduced bucket, so `side` and `idle`, which no
            # backward reached, pass PL's `p.grad is not None` rule here and read 0)
            assert (float(d0[k]) > 0) != ("side" in k or "idle" in k), k
    for v0, v1 in zip(r0["vec"], r1["vec"]):
        assert torch.equal(v0, v1)
    # the ranks saw different batches: what they logged is the norm of the MEAN gradient both of them hold after the exchange
    for n in r0["grads"]:
        assert torch.equal(r0["grads"][n], r1["grads"][n]), n
