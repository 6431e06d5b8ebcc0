"""Fused f32 attention (csrc/flash_attn_f32.hip) on inputs with closed-form answers: tests/attn_exact_inputs.py builds queries that
SELECT a key, a tie group, everything, or a two-level group.  The forward's o must then agree bit for bit (families A and B, C at
T = 2^n; C elsewhere within one f32 ulp), dq = dk = 0 of a selector bit for bit, and everything else -- lse2, dv, the other dq / dk, all
of family D -- per element under bounds counted in f32 roundings (attn_exact_inputs' docstring, "f32 routes").  The three kernels are
called through the C ABI so that lse2 and the raw dqkv are seen, into NaN-filled buffers with canaries behind them (the kernels store
float4 rows: a write past T or a row left out shows); one case per C goes through ops.attention_qkv autograd with ATTN_F32_FUSED on.
tests/test_attn_f32_exact_inputs.py shows on the host which planted faults these rules reject; tests/test_flash_attn_f32_gpu.py keeps
the Gaussian parity tests.  Recipes, bounds and observed margins: profiles/attn_f32_exact.md."""
import pytest
import torch

import attn_exact_inputs as ax
from canary_buffers import assert_canary, out_buf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def run_kernels(hip_lib, case):
    """forward and backward through the C ABI; everything back on the host: o, dq, dk, dv f32 [n, t, c], lse2 f32 [n, t]"""
    from odvae_amd import lib
    n, t, c = case["n"], case["t"], case["c"]
    scale = ax.scale_of(c)
    qkv = ax.pack_qkv(case, F32).to(DEV).contiguous()
    do = case["do"].float().to(DEV).contiguous()
    qkv0, do0 = qkv.clone(), do.clone()
    o_buf, o = out_buf(n * t * c)
    lse_buf, lse2 = out_buf(n * t)
    dqkv_buf, dqkv = out_buf(n * t * 3 * c)
    delta_buf, delta = out_buf(n * t)
    assert hip_lib.odvae_flash_attn_f32_supported(n, t, c) == 1
    lib.check(hip_lib.odvae_flash_attn_fwd_f32(qkv.data_ptr(), n, t, c, scale, o.data_ptr(), lse2.data_ptr(), lib.stream_ptr()), "flash_attn_fwd_f32")
    lib.check(hip_lib.odvae_flash_attn_bwd_f32(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(), n, t, c, scale, dqkv.data_ptr(),
                                               delta.data_ptr(), lib.stream_ptr()), "flash_attn_bwd_f32")
    torch.cuda.synchronize()
    assert_canary(o_buf, lse_buf, dqkv_buf, delta_buf)
    assert torch.equal(qkv, qkv0) and torch.equal(do, do0), "a kernel wrote into its inputs"
    dqkv = dqkv.view(n, t, 3 * c).cpu()
    return {"o": o.view(n, t, c).cpu(), "lse2": lse2.view(n, t).cpu(), "dq": dqkv[:, :, :c].contiguous(), "dk": dqkv[:, :, c:2 * c].contiguous(),
            "dv": dqkv[:, :, 2 * c:].contiguous()}


def check(hip_lib, kw):
    case = ax.make_case(**kw)
    ax.assert_preconditions(case, dtype=F32)
    margins = ax.check_case_f32(case, run_kernels(hip_lib, case), "fused")
    print("MARGIN fused %s C=%d T=%d N=%d %s" % (kw["family"], kw["c"], kw["t"], kw["n"], " ".join("%s=%.3f" % kv for kv in sorted(margins.items()))))


@pytest.mark.parametrize("c,t", ax.grid_f32())
def test_flash_attention_f32_exact(hip_lib, c, t):
    """Every family of one (C, T): all of o, lse2, dq, dk, dv, every element.  T = 1 ... 300 puts the edges of a wave's 16 rows, a tile's
    32 keys and a block's 64 rows on both sides, one to five blocks; T = 4100 (selector only) a long run of tiles; N rotates over 1, 3, 8.
    C = 512: dK and dV come from two launches of one template."""
    for kw in ax.cases_for_f32(c, t):
        check(hip_lib, kw)


@pytest.mark.parametrize("c", ax.CS)
def test_attention_qkv_autograd_exact(hip_lib, monkeypatch, c):
    """ops.attention_qkv on channels-last [N, 3C, H, W] with ATTN_F32_FUSED on: the wrapper's layout and its autograd hand the kernels
    the same problem -- bit-equal to the C ABI"""
    from odvae_amd import ops
    monkeypatch.setattr(ops, "ATTN_F32_FUSED", True)
    h, w = 5, 9
    case = ax.make_case("B", 3, h * w, c, group=4)
    ax.assert_preconditions(case, dtype=F32)

    def nchw(x):      # [n, t, ch] -> channels-last [n, ch, h, w]
        return x.float().to(DEV).reshape(case["n"], h, w, -1).permute(0, 3, 1, 2)

    def ntc(x):
        return x.detach().permute(0, 2, 3, 1).reshape(case["n"], h * w, -1).cpu().contiguous()

    qkv = nchw(torch.cat([case["q"], case["k"], case["v"]], 2)).requires_grad_(True)
    o = ops.attention_qkv(qkv)
    assert o.dtype == F32 and type(o.grad_fn).__name__ == "_FlashAttentionF32Backward"
    o.backward(nchw(case["do"]))
    g = ntc(qkv.grad)
    got = {"o": ntc(o), "dq": g[:, :, :c].contiguous(), "dk": g[:, :, c:2 * c].contiguous(), "dv": g[:, :, 2 * c:].contiguous()}
    raw = run_kernels(hip_lib, case)
    for name in got:
        ax.assert_bits_equal_f32(got[name], raw[name], "attention_qkv %s against the C ABI" % name)
    got["lse2"] = raw["lse2"]
    ax.check_case_f32(case, got, "fused")
