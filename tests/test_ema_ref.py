"""model.params.ema_decay / learn_logvar on the host: the `model_ema.*` key set, what the optimizers own, the constructor's checks, and the
restatement of LitEma's schedule (tests/ema_ref.py) against the numbers it is specified by.  No library call, no device."""
import os

import pytest
import torch

import ema_ref as E

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PLAIN_YAML = os.path.join(GOLDEN, "autoencoder_kl_plain.yaml")
POSE_YAML = os.path.join(GOLDEN, "autoencoder_kl_16x16x16.yaml")
SMALL = ["model.params.ddconfig.ch=32", "model.params.ddconfig.ch_mult=[1,2]", "model.params.ddconfig.num_res_blocks=1",
         "model.params.ddconfig.resolution=32"]
TRAINED = ("encoder.", "decoder.", "quant_conv.", "post_quant_conv.", "loss.discriminator.")


def plain(*dots):
    from odvae_amd.config import Config, instantiate_from_config
    torch.manual_seed(23)
    return instantiate_from_config(Config.merge(Config.load(PLAIN_YAML), Config.from_dotlist(SMALL + list(dots))).model)


def pose(**params):
    from odvae_amd import synthetic
    from odvae_amd.config import instantiate_from_config
    cfg, _ = synthetic.model_config(POSE_YAML, latent_hw=4, ch=32)
    for k, v in params.items():
        cfg.params[k] = v
    torch.manual_seed(23)
    return instantiate_from_config(cfg)


def check_key_set(model, decay, trained_prefixes):
    sd = model.state_dict()
    ema = {k[len("model_ema."):]: v for k, v in sd.items() if k.startswith("model_ema.")}
    rest = {k for k in sd if not k.startswith("model_ema.")}
    want = {E.shadow_name(n): p for n, p in model.named_parameters() if p.requires_grad}
    assert set(ema) == set(want) | {"decay", "num_updates"}
    assert ema["decay"].dtype == torch.float32 and ema["decay"].shape == () and ema["decay"] == torch.tensor(decay, dtype=torch.float32)
    assert ema["num_updates"].dtype == torch.int32 and ema["num_updates"].shape == () and int(ema["num_updates"]) == 0
    for k, p in want.items():
        assert "." not in k and ema[k].dtype == torch.float32 and ema[k].shape == p.shape and torch.equal(ema[k], p.detach()), k
        assert ema[k].data_ptr() != p.data_ptr(), k      # a clone, not an alias
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert "loss.logvar" in names and all(n == "loss.logvar" or n.startswith(trained_prefixes) for n in names)
    for prefix in trained_prefixes:
        assert any(n.startswith(prefix) for n in names), prefix
    # the frozen perceptual net is in the state_dict and has no shadow
    assert any(k.startswith("loss.perceptual_loss.") for k in rest) and not any(k.startswith("lossperceptual_loss") for k in ema)
    assert not any(p.requires_grad for p in model.loss.perceptual_loss.parameters())
    assert not list(model.model_ema.parameters())      # buffers only: no optimizer and no gradient ever sees the average
    return rest


def test_plain_model_has_exactly_the_model_ema_keys():
    model = plain("model.params.ema_decay=0.999")
    assert model.use_ema and model.learn_logvar is False
    rest = check_key_set(model, 0.999, TRAINED)
    off = plain()
    assert not off.use_ema and not hasattr(off, "model_ema")
    assert set(off.state_dict()) == rest and not any(k.startswith("model_ema") for k in off.state_dict())
    sd = model.state_dict()
    assert sd["model_ema.encoderconv_inweight"].shape == (32, 3, 3, 3) and "model_ema.losslogvar" in sd
    # moves, saves and loads on the host
    other = plain("model.params.ema_decay=0.5")
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
        model.model_ema.num_updates.fill_(7)
    res = other.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(other.model_ema.decay) == float(torch.tensor(0.999, dtype=torch.float32)) and int(other.model_ema.num_updates) == 7
    assert torch.equal(other.model_ema.encoderconv_inweight, model.model_ema.encoderconv_inweight)
    assert not torch.equal(other.model_ema.encoderconv_inweight, other.encoder.conv_in.weight)
    assert other.double().model_ema.encoderconv_inweight.dtype == torch.float64 and other.model_ema.num_updates.dtype == torch.int32


def test_a_checkpoint_without_the_average_loads_non_strictly():
    model, off = plain("model.params.ema_decay=0.999"), plain()
    before = {k: v.clone() for k, v in model.model_ema.state_dict().items()}
    with pytest.raises(RuntimeError, match="model_ema"):
        model.load_state_dict(off.state_dict(), strict=True)
    res = model.load_state_dict(off.state_dict(), strict=False)
    assert set(res.missing_keys) == {"model_ema." + k for k in before} and not res.unexpected_keys
    assert all(torch.equal(v, before[k]) for k, v in model.model_ema.state_dict().items())


@pytest.mark.parametrize("decay", [0, 1, 1.5, 0.0, 1.0, -0.1])
def test_ema_decay_outside_the_open_interval_asserts(decay):
    with pytest.raises(AssertionError):
        plain("model.params.ema_decay=%r" % decay)
    with pytest.raises(AssertionError):
        pose(ema_decay=decay)


def owners(model):
    model.learning_rate = 1e-4
    (opt_ae, opt_disc), schedulers = model.configure_optimizers()
    assert schedulers == []
    return [[id(p) for g in o.param_groups for p in g["params"]] for o in (opt_ae, opt_disc)]


@pytest.mark.parametrize("build", [plain, pose], ids=["plain", "pose"])
def test_learn_logvar_puts_logvar_into_optimizer_0_alone(build):
    on = build("model.params.learn_logvar=True") if build is plain else build(learn_logvar=True)
    off = build()
    assert on.learn_logvar is True and off.learn_logvar is False and not on.use_ema
    own_on, own_off = owners(on), owners(off)
    assert own_on[0].count(id(on.loss.logvar)) == 1 and id(on.loss.logvar) not in own_on[1]
    assert id(off.loss.logvar) not in own_off[0] + own_off[1]
    assert len(own_on[0]) == len(own_off[0]) + 1 and len(own_on[1]) == len(own_off[1])
    assert own_on[0][-1] == id(on.loss.logvar)      # appended: the other parameters keep their arena offsets


def test_pose_model_takes_the_two_keys_as_an_extension():
    model = pose(ema_decay=0.9999)
    assert model.use_ema
    check_key_set(model, 0.9999, TRAINED[:2] + ("quant_conv_obj.", "quant_conv_pose.", "post_quant_conv.", "pose_encoder.", "pose_decoder.",
                                               "loss.discriminator."))
    off = pose()
    assert not off.use_ema and not hasattr(off, "model_ema") and not any(k.startswith("model_ema") for k in off.state_dict())


def test_the_update_needs_a_hip_device():
    from odvae_amd.lib import HipLibraryError
    model = plain("model.params.ema_decay=0.999")
    with pytest.raises(HipLibraryError):
        model.model_ema(model)
    with pytest.raises(HipLibraryError):
        model.on_train_batch_end()
    with pytest.raises(HipLibraryError):
        with model.ema_scope():
            pass
    plain().on_train_batch_end()      # without the average the hook does nothing
    # the launch plan (a weak reference to the model among it) stays out of copies and pickles
    import copy
    import io
    twin = copy.deepcopy(model)
    assert twin.model_ema is not model.model_ema and torch.equal(twin.model_ema.losslogvar, model.model_ema.losslogvar)
    buf = io.BytesIO()
    torch.save(model.model_ema, buf)


# ---- the restatement's schedule against the specification's numbers -----------------------------------------------------------------
def test_schedule_is_the_f32_division_of_the_two_converted_integers():
    import numpy as np
    decay = torch.tensor(0.9999, dtype=torch.float32)
    n = torch.tensor(0, dtype=torch.int32)
    for k in list(range(1, 2001)) + [10 ** 4, 10 ** 5, 2 * 10 ** 5, 10 ** 6]:
        n, d, omd = E.schedule(decay, torch.tensor(k - 1, dtype=torch.int32))
        assert int(n) == k and n.dtype == torch.int32
        q = np.float32(1 + k) / np.float32(10 + k)                      # one correctly rounded f32 division
        assert q.dtype == np.float32 and q == np.float32(np.float64(1 + k) / np.float64(10 + k))      # (double rounding cannot bite: 53 >= 2 * 24 + 2)
        want = q if q < np.float32(0.9999) else np.float32(0.9999)
        assert d.dtype == torch.float32 and d.item() == float(want), k
        assert omd.dtype == torch.float32 and omd.item() == float(np.float32(1) - want), k


def test_the_cap_takes_over_at_80_for_decay_0_9():
    decay = torch.tensor(0.9, dtype=torch.float32)
    ds = [E.schedule(decay, torch.tensor(k - 1, dtype=torch.int32))[1] for k in range(1, 200)]
    first_capped = next(k for k, d in zip(range(1, 200), ds) if torch.equal(d, decay))
    assert first_capped == 80                                           # (1 + 80) / (10 + 80) = 0.9; at 79 the quotient 80 / 89 = 0.8989 is below it
    assert all(d < decay for d in ds[:79]) and all(torch.equal(d, decay) for d in ds[79:])
    assert ds[0].item() == float(torch.tensor(2.0) / torch.tensor(11.0))


def test_without_the_counter_the_decay_is_constant():
    ref = E.LitEmaRef({"a.b": torch.zeros(3)}, 0.5, use_num_upates=False)
    assert int(ref.num_updates) == -1 and list(ref.shadow) == ["ab"]
    d, omd = ref({"a.b": torch.ones(3)})
    assert int(ref.num_updates) == -1 and d.item() == 0.5 and omd.item() == 0.5 and torch.equal(ref.shadow["ab"], torch.full((3,), 0.5))
    assert set(ref.state_dict()) == {"model_ema.decay", "model_ema.num_updates", "model_ema.ab"}


def test_update_is_three_roundings():
    """s - omd * (s - p) differs from the fused and from the algebraically equal d * s + omd * p on ordinary inputs: the restatement is the
    three-operation form"""
    g = torch.Generator().manual_seed(3)
    s, p = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    omd = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.9999, dtype=torch.float32)
    got = E.update_(s.clone(), p, omd)
    t = (s - p)
    assert torch.equal(got, s - (omd * t))
    fused = (s.double() - omd.double() * t.double()).float()            # what one rounding of s - omd * t gives
    assert not torch.equal(got, fused)
    assert not torch.equal(got, torch.tensor(0.9999) * s + omd * p)
