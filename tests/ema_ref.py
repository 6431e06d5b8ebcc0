"""Plain-torch restatement of [UPSTREAM] ldm.modules.ema.LitEma, run on the CPU in f32: the oracle of tests/test_ema_ref.py and
tests/test_ema_gpu.py (the role tests/actnorm_ref.py has for ActNorm).

  buffers   decay (f32 scalar), num_updates (int32 scalar: 0, or -1 with use_num_upates=False), one clone per parameter that requires a
            gradient, named by the parameter's name without its dots
  update    num_updates >= 0:  num_updates += 1;  q = (1 + num_updates) / (10 + num_updates)  -- two int32 tensors, torch's true division:
            both converted to f32, one correctly rounded division;  d = min(decay, q).   Otherwise d = decay.
            omd = 1 - d (f32);  every shadow:  s.sub_(omd * (s - p))  -- three f32 operations, three roundings, no fused multiply-add

Everything below is written with tensor operations only, so that what rounds where is torch's and not Python's (a Python float is a double).
"""
import torch


def schedule(decay, num_updates):
    """One counter step.  decay: f32 0-d tensor, num_updates: int32 0-d tensor -> (num_updates after the step, d, 1 - d), f32 0-d tensors"""
    assert decay.dtype == torch.float32 and num_updates.dtype == torch.int32
    n = num_updates.clone()
    d = decay.clone()
    if int(n) >= 0:
        n += 1
        q = (1 + n) / (10 + n)
        assert q.dtype == torch.float32
        d = torch.min(decay, q)
    omd = 1 - d
    assert omd.dtype == torch.float32
    return n, d, omd


def update_(shadow, param, omd):
    """shadow <- shadow - omd * (shadow - param), in place, as upstream writes it"""
    assert shadow.dtype == param.dtype == torch.float32 and shadow.device.type == "cpu"
    shadow.sub_(omd * (shadow - param))
    return shadow


def shadow_name(param_name):
    return param_name.replace(".", "")


class LitEmaRef:
    """The whole class on a dict of named CPU tensors"""

    def __init__(self, named_params, decay, use_num_upates=True):
        self.decay = torch.tensor(decay, dtype=torch.float32)
        self.num_updates = torch.tensor(0 if use_num_upates else -1, dtype=torch.int32)
        self.shadow = {shadow_name(k): v.detach().cpu().float().clone() for k, v in named_params.items()}

    def __call__(self, named_params):
        self.num_updates, d, omd = schedule(self.decay, self.num_updates)
        for k, v in named_params.items():
            update_(self.shadow[shadow_name(k)], v.detach().cpu(), omd)
        return d, omd

    def state_dict(self, prefix="model_ema."):
        out = {prefix + "decay": self.decay, prefix + "num_updates": self.num_updates}
        out.update({prefix + k: v for k, v in self.shadow.items()})
        return out
