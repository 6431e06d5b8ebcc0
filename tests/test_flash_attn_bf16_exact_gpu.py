"""bf16 flash attention (csrc/flash_attn_bf16.hip) on inputs with closed-form answers: tests/attn_exact_inputs.py builds queries that
SELECT a key, a tie group, everything, or a two-level group; o, dv (and dq = dk = 0) must then agree bit for bit, the rest per element
under a bound derived from the number formats (2^-7 of the element's own sum of |terms| plus the f32 cancellation floor).  The plain
forward / dQ / dK-dV kernels (C = 64, 512) and the wave-pair kernels (C = 128, 256) are called through the C ABI so that lse2 and the
raw dqkv are seen; one case per C goes through ops.attention_qkv autograd to tie the wrapper's layout to the same answers.
tests/test_attn_exact_inputs.py shows on the host which planted faults these rules reject; tests/test_bf16_gpu.py keeps the Gaussian
parity tests.  Recipes, bound and observed margins: profiles/flash_attn_exact.md."""
import pytest
import torch

import attn_exact_inputs as ax

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def run_kernels(hip_lib, case):
    """forward and backward through the C ABI; everything back on the host: o, dq, dk, dv bf16 [n, t, c], lse2 f32 [n, t]"""
    from odvae_amd import lib
    n, t, c = case["n"], case["t"], case["c"]
    scale = ax.scale_of(c)
    qkv = ax.pack_qkv(case).to(DEV).contiguous()
    do = case["do"].float().to(BF).to(DEV).contiguous()
    o = torch.full((n, t, c), float("nan"), dtype=BF, device=DEV)             # every element must be written
    lse2 = torch.full((n, t), float("nan"), dtype=torch.float32, device=DEV)
    dqkv = torch.full((n, t, 3 * c), float("nan"), dtype=BF, device=DEV)
    delta = torch.empty(n * t, dtype=torch.float32, device=DEV)
    assert hip_lib.odvae_flash_attn_supported(n, t, c) == 1
    lib.check(hip_lib.odvae_flash_attn_fwd_bf16(qkv.data_ptr(), n, t, c, scale, o.data_ptr(), lse2.data_ptr(), lib.stream_ptr()), "flash_attn_fwd")
    lib.check(hip_lib.odvae_flash_attn_bwd_bf16(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(), n, t, c, scale, dqkv.data_ptr(),
                                                delta.data_ptr(), lib.stream_ptr()), "flash_attn_bwd")
    torch.cuda.synchronize()
    dqkv = dqkv.cpu()
    return {"o": o.cpu(), "lse2": lse2.cpu(), "dq": dqkv[:, :, :c].contiguous(), "dk": dqkv[:, :, c:2 * c].contiguous(), "dv": dqkv[:, :, 2 * c:].contiguous()}


def check(hip_lib, kw):
    case = ax.make_case(**kw)
    ax.assert_preconditions(case)
    margins = ax.check_case(case, run_kernels(hip_lib, case))
    print("MARGIN %s C=%d T=%d N=%d %s" % (kw["family"], kw["c"], kw["t"], kw["n"], " ".join("%s=%.3f" % kv for kv in sorted(margins.items()))))


@pytest.mark.parametrize("c,t", ax.grid())
def test_flash_attention_exact(hip_lib, c, t):
    """Every family of one (C, T): all of o, lse2, dq, dk, dv, every element.  T = 1 ... 300 covers 1 ... 10 key tiles, fewer tiles than
    ring stages, ragged last tiles and 1 ... 3 query blocks; T = 4100 (selector only) a long ring run; N rotates over 1, 3, 8."""
    for kw in ax.cases_for(c, t):
        check(hip_lib, kw)


@pytest.mark.parametrize("c", ax.CS)
def test_attention_qkv_autograd_exact(hip_lib, c):
    """ops.attention_qkv on channels-last [N, 3C, H, W]: the wrapper's layout and its autograd hand the kernels the same problem"""
    from odvae_amd import ops
    h, w = 5, 9
    case = ax.make_case("B", 3, h * w, c, group=4)
    ax.assert_preconditions(case)

    def nchw(x):      # [n, t, ch] -> channels-last [n, ch, h, w]
        return x.float().to(BF).to(DEV).reshape(case["n"], h, w, -1).permute(0, 3, 1, 2)

    def ntc(x):
        return x.detach().permute(0, 2, 3, 1).reshape(case["n"], h * w, -1).cpu().contiguous()

    qkv = nchw(torch.cat([case["q"], case["k"], case["v"]], 2)).requires_grad_(True)
    o = ops.attention_qkv(qkv)
    assert o.dtype == BF
    o.backward(nchw(case["do"]))
    g = ntc(qkv.grad)
    got = {"o": ntc(o), "dq": g[:, :, :c].contiguous(), "dk": g[:, :, c:2 * c].contiguous(), "dv": g[:, :, 2 * c:].contiguous()}
    raw = run_kernels(hip_lib, case)
    for name in got:
        ax.assert_bits_equal(got[name], raw[name], "attention_qkv %s against the C ABI" % name)
    got["lse2"] = raw["lse2"]
    ax.check_case(case, got)
