"""ddconfig.resamp_with_conv = False and tanh_out = True: the module tree (no device needed).  Upstream's Upsample / Downsample have no
`conv` without with_conv, so the state_dict has no `upsample.conv.*` / `downsample.conv.*` keys; the oracle (oracle/ldm_model.py) is the
reference for the key set, and a state_dict must load strictly in both directions."""
import pytest
import torch

DD = dict(double_z=True, z_channels=16, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2, 4],
          num_res_blocks=2, attn_resolutions=[16], dropout=0.0)


def _pair(which, **extra):
    from odvae_amd import modules
    from oracle import ldm_model
    torch.manual_seed(3)
    cfg = dict(DD, **extra)
    return getattr(modules, which)(**cfg), getattr(ldm_model, which)(**cfg)


@pytest.mark.parametrize("which,extra", [("Encoder", dict(resamp_with_conv=False)),
                                         ("Decoder", dict(resamp_with_conv=False, tanh_out=True)),
                                         ("Decoder", dict(tanh_out=True))], ids=["encoder", "decoder", "decoder-tanh-only"])
def test_construction_and_state_dict_both_ways(which, extra):
    net, ref = _pair(which, **extra)
    assert set(net.state_dict()) == set(ref.state_dict())
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    res = ref.load_state_dict(net.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if not extra.get("resamp_with_conv", True):
        assert not [k for k in net.state_dict() if "sample.conv" in k]
        samplers = [m for m in net.modules() if type(m).__name__ in ("Upsample", "Downsample")]
        assert len(samplers) == 4 and all(not m.with_conv and not hasattr(m, "conv") and not list(m.parameters()) for m in samplers)
    if which == "Decoder":
        assert net.tanh_out is True


@pytest.mark.parametrize("which", ["Encoder", "Decoder"])
def test_default_key_set_is_unchanged(which):
    net, ref = _pair(which)
    plain, _ = _pair(which, resamp_with_conv=True)
    keys = list(net.state_dict())
    assert keys == list(plain.state_dict()) and set(keys) == set(ref.state_dict())
    kind = "downsample" if which == "Encoder" else "upsample"
    assert sum(k.endswith("%s.conv.weight" % kind) for k in keys) == 4 and sum(k.endswith("%s.conv.bias" % kind) for k in keys) == 4
    conv_less, _ = _pair(which, resamp_with_conv=False)
    assert set(keys) - set(conv_less.state_dict()) == {k for k in keys if "sample.conv" in k}
    if which == "Decoder":
        assert net.tanh_out is False


def test_grad_reducer_arena_has_no_resampler_convs(tmp_path):
    """Layout only (single process, gloo group of one over a file store): the gradient arena of a conv-less Encoder + Decoder covers
    exactly its parameters -- eight 3x3 convs (weight + bias) fewer than the default network's."""
    import torch.distributed as dist
    from odvae_amd.parallel import GradReducer
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        sizes = {}
        for with_conv in (True, False):
            enc, _ = _pair("Encoder", resamp_with_conv=with_conv)
            dec, _ = _pair("Decoder", resamp_with_conv=with_conv, tanh_out=True)
            params = list(enc.parameters()) + list(dec.parameters())
            red = GradReducer(torch.optim.Adam(params, lr=1e-4), bucket_mb=1.0)
            assert len(red.slices) == len(params) and sum(n for _, _, n in red.slices) == sum(p.numel() for p in params)
            assert sum(e - s for s, e in red.buckets) == red.arena.numel()
            sizes[with_conv] = (len(params), sum(p.numel() for p in params))
        convs = [32, 32, 64, 64] + [128, 64, 64, 32]      # channels at the four Downsamples and the four Upsamples (ch=32, ch_mult 1,1,2,2,4)
        assert sizes[True][0] - sizes[False][0] == 16
        assert sizes[True][1] - sizes[False][1] == sum(9 * c * c + c for c in convs)
    finally:
        if own:
            dist.destroy_process_group()
