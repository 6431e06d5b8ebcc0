"""Linear attention, host side (no device): the refused config key constructs, the module tree is the reference's, and the acceptance
rule of tests/linattn_ref.py admits host f32 at every case the GPU tests run and rejects the faults a kernel of this design can have."""
import pytest
import torch

import linattn_ref as R

DD = dict(double_z=True, z_channels=4, resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
          attn_resolutions=[8], dropout=0.0)
CORE_CASES = [(n, c, t) for n in (1, 3) for c in (32, 96, 128) for t in (1, 35, 256)]


def test_make_attn_linear_constructs():
    from odvae_amd import modules
    blk = modules.make_attn(64, "linear")
    assert isinstance(blk, modules.LinAttnBlock)
    for gone in ("norm", "q", "k", "v", "proj_out"):
        assert not hasattr(blk, gone), gone
    assert isinstance(modules.make_attn(64, "none"), torch.nn.Identity)
    assert isinstance(modules.make_attn(64, "vanilla"), modules.AttnBlock)
    with pytest.raises(NotImplementedError):
        modules.make_attn(64, "vanilla-xformers")


@pytest.mark.parametrize("which", ["Encoder", "Decoder"])
def test_use_linear_attn_constructs_with_the_counterparts_state_dict(which):
    from odvae_amd import modules
    from oracle import ldm_model
    net = getattr(modules, which)(use_linear_attn=True, **DD)
    ref = R.linearize(getattr(ldm_model, which)(**DD))
    assert isinstance(net.mid.attn_1, modules.LinAttnBlock)
    stages = net.down if which == "Encoder" else net.up
    assert sum(isinstance(a, modules.LinAttnBlock) for s in stages for a in s.attn) == (1 if which == "Encoder" else 2)
    sd, sd_ref = net.state_dict(), ref.state_dict()
    assert set(sd) == set(sd_ref)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in sd_ref.items()}
    assert tuple(sd["mid.attn_1.to_qkv.weight"].shape) == (3 * 64, 64, 1, 1)
    assert "mid.attn_1.to_qkv.bias" not in sd and "mid.attn_1.to_out.bias" in sd
    assert not [k for k in sd if ".attn" in k and ".norm." in k]
    res = net.load_state_dict(sd_ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # attn_type="linear" is the same request; the vanilla tree is what it was
    assert set(getattr(modules, which)(attn_type="linear", **DD).state_dict()) == set(sd)
    assert "mid.attn_1.q.weight" in getattr(modules, which)(**DD).state_dict()


def test_yaml_ddconfig_with_use_linear_attn_instantiates(tmp_path):
    from odvae_amd import modules
    from odvae_amd.config import Config, instantiate_from_config
    lines = ["target: src.modules.autoencodermodules.feat_encoder.FeatEncoder", "params:"]
    lines += ["  %s: %s" % (k, v) for k, v in DD.items()] + ["  use_linear_attn: True"]
    path = tmp_path / "enc.yaml"
    path.write_text("\n".join(lines) + "\n")
    enc = instantiate_from_config(Config.load(str(path)))
    assert isinstance(enc, modules.Encoder) and isinstance(enc.mid.attn_1, modules.LinAttnBlock)
    assert isinstance(enc.down[1].attn[0], modules.LinAttnBlock)


def test_reference_module_is_the_functional_core():
    torch.manual_seed(0)
    blk = R.LinAttnBlock(32).double()
    x = torch.randn(2, 32, 5, 7, dtype=torch.float64)
    q, k, v = blk.to_qkv(x).reshape(2, 3, 32, 35).unbind(1)
    ks = torch.softmax(k, dim=2)
    assert torch.allclose(ks.sum(2), torch.ones(2, 32, dtype=torch.float64))
    out = torch.stack([sum(torch.outer(ks[b, :, n], v[b, :, n]) for n in range(35)).t() @ q[b] for b in range(2)])
    want = blk.to_out(out.reshape(2, 32, 5, 7))
    assert torch.allclose(blk(x), want, atol=1e-12)


def test_softmax_backward_identity_removes_the_reduction_over_tokens():
    """sum_n s[n][d] ds[n][d] = g[d] = sum_e ctx[d][e] dctx[d][e]: the host model (which uses it) reproduces autograd in float64."""
    q, k, v, do = (t.double() for t in R.make_qkv(2, 32, 35))
    refs = R.core_refs(q, k, v, do)
    ks = k.softmax(-1)
    dctx = torch.einsum("bdn,ben->bde", q, do)
    ds = torch.einsum("ben,bde->bdn", v, dctx)
    g = (refs[64]["ctx"] * dctx).sum(-1)
    assert ((ks * ds).sum(-1) - g).abs().max().item() < 1e-12 * g.abs().max().item()
    assert (ks * (ds - g.unsqueeze(-1)) - refs[64]["dk"]).abs().max().item() < 1e-12


@pytest.mark.parametrize("n,c,t", CORE_CASES, ids=lambda v: str(v))
def test_rule_admits_host_f32(n, c, t):
    q, k, v, do = R.make_qkv(n, c, t)
    refs = R.core_refs(q, k, v, do)
    R.check(R.core_figures(R.host_model(q, k, v, do), refs), "host f32 N%d C%d T%d" % (n, c, t))


@pytest.mark.parametrize("a", R.OFFSETS)
def test_rule_admits_host_f32_on_the_offset_ladder(a):
    q, k, v, do = R.make_qkv(2, 32, 64, offset=a)
    refs = R.core_refs(q, k, v, do)
    got = R.host_model(q, k, v, do)
    assert all(torch.isfinite(t).all() for t in got.values())
    R.check(R.core_figures(got, refs), "host f32 offset %g" % a)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_rule_rejects_planted_faults(fault):
    a = 90 if fault == "no_max_subtraction" else 0
    q, k, v, do = R.make_qkv(2, 32, 64, offset=a)
    refs = R.core_refs(q, k, v, do)
    got = R.host_model(q, k, v, do, fault=fault)
    figs = R.core_figures(got, refs)
    bad = [f["name"] for f in figs if not R.inside(f)]
    assert bad, "the rule admits the fault %s" % fault
    if fault == "no_max_subtraction":      # exp(90 + randn) overflows f32: the result is not finite
        assert not all(torch.isfinite(t).all() for t in got.values())
    if fault == "g_dropped":
        assert bad == ["dk"], bad
