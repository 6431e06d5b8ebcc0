"""Cost of the ResnetBlock dropout inside the GroupNorm (+ swish) kernels, against the plain kernels in the same process.

Kernels (default): 128 channels at 256 x 256, B = 32 (the 1 GiB-class f32 tensor), f32 and bf16 -- the forward apply pass
(odvae_groupnorm_apply_* / _apply_drop_*) and the two-kernel backward (odvae_groupnorm_bwd_* with the read-once form off / _bwd_drop_*).
HIP events around 20 back-to-back launches after 3 warm-up launches, no synchronisation inside the timed run, plain and dropout forms
alternated over three rounds; the minimum per form is printed with the ratio.

--step: one f32 training step of the headline geometry (ch = 128, 256 x 256, B = 32) with ddconfig.dropout 0.0 and 0.1 (events around
5 steps after 3 warm-up steps each): what bypassing the conv data gradient's GroupNorm-backward sums and the read-once kernel on the
norm2 layers costs, beside the mask's own cost above.
usage: python tools/gn_drop_time.py [--step] [--batch N]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
P, SEED = 0.1, 0x1234567890ABCDEF


def timed(call, launches=20, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernels(batch):
    from odvae_amd import lib as _lib, ops
    L = _lib.load()
    dev = torch.device("cuda:0")
    n, c, h, w = batch, 128, 256, 256
    for bf16 in (False, True):
        dt, esz, sfx = (torch.bfloat16, 2, "_bf16") if bf16 else (torch.float32, 4, "_f32")
        x = (torch.randn(n, h, w, c, device=dev) * 2 + 0.5).to(dt)
        dy = torch.randn(n, h, w, c, device=dev).to(dt)
        out = torch.empty_like(x)
        gamma, beta = torch.randn(c, device=dev), torch.randn(c, device=dev)
        xg = x.float().reshape(n, h * w, 32, c // 32)
        mean = xg.mean(dim=(1, 3)).contiguous()
        rstd = (1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-6)).contiguous()
        del xg
        dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        wsf = L.odvae_groupnorm_bf16_workspace_bytes if bf16 else L.odvae_groupnorm_workspace_bytes
        wp, wn = ops._ws(wsf(n, h * w, c, 32), x)
        st = _lib.stream_ptr()
        stats = (gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1)

        def fwd(drop):
            if drop:
                _lib.check(getattr(L, "odvae_groupnorm_apply_drop" + sfx)(x.data_ptr(), n, h * w, c, 32, *stats, P, SEED, out.data_ptr(), st), "apply_drop")
            else:
                _lib.check(getattr(L, "odvae_groupnorm_apply" + sfx)(x.data_ptr(), n, h * w, c, 32, *stats, out.data_ptr(), st), "apply")

        def bwd(drop):
            tail = (out.data_ptr(), dg.data_ptr(), db.data_ptr(), None, wp, wn, st)
            if drop:
                _lib.check(getattr(L, "odvae_groupnorm_bwd_drop" + sfx)(x.data_ptr(), dy.data_ptr(), n, h * w, c, 32, *stats, P, SEED, *tail), "bwd_drop")
            else:
                _lib.check(getattr(L, "odvae_groupnorm_bwd" + sfx)(x.data_ptr(), dy.data_ptr(), n, h * w, c, 32, *stats, *tail), "bwd")

        prev = L.odvae_groupnorm_select_backward(0)
        try:
            for name, fn, passes in (("forward apply", fwd, 2), ("backward (reduce + apply)", bwd, 5)):
                best = {False: float("inf"), True: float("inf")}
                for _ in range(3):
                    for drop in (False, True):
                        best[drop] = min(best[drop], timed(lambda: fn(drop)))
                nbytes = passes * n * h * w * c * esz      # bytes the kernels move: x (+ dy) read per pass, one tensor written
                print("%s N=%d C=%d %dx%d %s: plain %.3f ms (%.2f TB/s) | dropout p=%.1f %.3f ms (%.2f TB/s) | x%.3f"
                      % ("bf16" if bf16 else "f32", n, c, h, w, name, best[False], nbytes / best[False] / 1e9, P, best[True],
                         nbytes / best[True] / 1e9, best[True] / best[False]), flush=True)
        finally:
            L.odvae_groupnorm_select_backward(prev)
        del x, dy, out


def step(batch):
    from odvae_amd import ops, synthetic
    from odvae_amd.config import instantiate_from_config
    from odvae_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    data = synthetic.make_batch(batch, 256, seed=23)
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}
    for p in (0.0, 0.1):
        torch.manual_seed(23)
        mcfg, cfg = synthetic.model_config(YAML, latent_hw=16)
        mcfg.params.ddconfig["dropout"] = p
        model = instantiate_from_config(mcfg)
        model.learning_rate = 12 * cfg.model.base_learning_rate
        model = model.to(dev).train()
        model._global_step = 1
        trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0,))
        i = [0]

        def one():
            b = dict(data)
            b["pose_6d"] = data["pose_6d"].clone()
            trainer.training_batch(b, i[0])
            i[0] += 1

        hits = ops.GN_FUSED_BWD_HITS
        ms = timed(one, launches=5, warm=3)
        print("f32 step B=%d 256x256 ddconfig.dropout=%.1f: %.1f ms per step (GroupNorm backwards fed by a conv epilogue: %d per step)"
              % (batch, p, ms, (ops.GN_FUSED_BWD_HITS - hits) // 8), flush=True)
        del trainer, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    nb = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 32
    if "--step" in sys.argv:
        step(nb)
    else:
        kernels(nb)
