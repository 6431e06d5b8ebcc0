"""Anomaly mode without a GPU: the C ABI of csrc/anomaly.hip (exported, declared, host-side argument checks that fail before any
launch), the mode switch of Trainer(detect_anomaly=...) and the yaml -> Trainer mapping of the runner."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
SYMBOLS = ("odvae_anomaly_scan", "odvae_anomaly_reset")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


def test_symbols_exported_and_declared(built_lib):
    handle = built_lib.load()
    declared = built_lib.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in built_lib.PROTOTYPES and hasattr(handle, name), name
    assert handle.odvae_abi_version() == 4
    assert "anomaly.hip" in open(os.path.join(ROOT, "generative-detection_amd", "build.py")).read()


def test_descriptor_layout_matches_header():
    from odvae_amd import anomaly
    assert ctypes.sizeof(anomaly._TensorDesc) == 24
    text = open(os.path.join(ROOT, "include", "odvae_hip.h")).read()
    assert "typedef struct { const void* ptr; int64_t numel; int32_t dtype; int32_t output_index; } OdvaeAnomalyTensor;" in text
    assert "#define ODVAE_ANOMALY_CLEAN 0x7fffffffffffffffull" in text and anomaly.CLEAN == 0x7fffffffffffffff


def _descs(*items):
    from odvae_amd import anomaly
    return (anomaly._TensorDesc * len(items))(*[anomaly._TensorDesc(*it) for it in items])


def test_bad_arguments_fail_on_the_host(built_lib):
    """Every call below returns ODVAE_ERR_ARG (1) with a message before any launch; the pointers are never dereferenced."""
    h = built_lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    rec = ctypes.c_void_p(base)
    good = (base + 64, 16, 0, 0)
    null = ctypes.c_void_p(0)
    scan = h.odvae_anomaly_scan
    assert scan(_descs(good), 1, 0, 0, null, null) == 1
    assert b"null record" in h.odvae_last_error()
    assert scan(_descs(good), 1, 0, 0, ctypes.c_void_p(base + 4), null) == 1
    assert b"misaligned record" in h.odvae_last_error()
    assert scan(None, 1, 0, 0, rec, null) == 1
    assert scan(_descs(*[good] * 9), 9, 0, 0, rec, null) == 1
    assert b"9 tensors" in h.odvae_last_error()
    assert scan(_descs(good), 0, 0, 0, rec, null) == 1
    assert scan(_descs(good, (base + 64, -1, 0, 1)), 2, 0, 0, rec, null) == 1
    assert b"negative count" in h.odvae_last_error()
    assert scan(_descs((base + 64, 16, 2, 0)), 1, 0, 0, rec, null) == 1
    assert b"dtype" in h.odvae_last_error()
    assert scan(_descs((base + 64, 16, 0, -1)), 1, 0, 0, rec, null) == 1
    assert scan(_descs((base + 64, 16, 0, 1 << 20)), 1, 0, 0, rec, null) == 1
    assert scan(_descs((None, 16, 0, 0)), 1, 0, 0, rec, null) == 1
    assert b"null" in h.odvae_last_error()
    assert scan(_descs((base + 66, 16, 0, 0)), 1, 0, 0, rec, null) == 1      # f32 at a 2-byte offset
    assert scan(_descs((base + 65, 16, 1, 0)), 1, 0, 0, rec, null) == 1      # bf16 at an odd byte
    assert b"misaligned" in h.odvae_last_error()
    assert scan(_descs(good), 1, -1, 0, rec, null) == 1
    assert scan(_descs(good), 1, 1 << 43, 0, rec, null) == 1
    assert scan(_descs(good), 1, 0, 2, rec, null) == 1
    assert b"mode" in h.odvae_last_error()
    assert h.odvae_anomaly_reset(null, null) == 1
    assert h.odvae_anomaly_reset(ctypes.c_void_p(base + 4), null) == 1


@pytest.mark.parametrize("value,mode", [(False, None), (True, "nan"), ("nan", "nan"), ("nonfinite", "nonfinite"), (0, None), (1, "nan"),
                                        ("NaN", "nan"), ("true", "nan"), ("false", None)])
def test_mode_values(value, mode):
    from odvae_amd import anomaly
    assert anomaly.parse_mode(value) == mode


@pytest.mark.parametrize("env,mode", [(None, None), ("", None), ("0", None), ("1", "nan"), ("nonfinite", "nonfinite")])
def test_mode_from_environment(monkeypatch, env, mode):
    from odvae_amd import anomaly
    if env is None:
        monkeypatch.delenv("ODVAE_DETECT_ANOMALY", raising=False)
    else:
        monkeypatch.setenv("ODVAE_DETECT_ANOMALY", env)
    assert anomaly.parse_mode(None) == mode
    assert anomaly.parse_mode(False) is None          # an explicit False wins over the environment


@pytest.mark.parametrize("value", ["inf", 2, "yes please"])
def test_mode_rejects(value):
    from odvae_amd import anomaly
    with pytest.raises(ValueError):
        anomaly.parse_mode(value)


def test_watch_is_a_noop_when_off():
    import torch
    from odvae_amd import anomaly
    x = torch.randn(4, requires_grad=True)
    y = (x * 2).sum()
    anomaly.watch(y)                                  # no active phase: nothing registered, nothing launched
    y.backward()
    assert torch.equal(x.grad, torch.full((4,), 2.0))


def test_yaml_maps_detect_anomaly_to_the_trainer():
    from odvae_amd import run
    from odvae_amd.config import Config
    cfg = Config.load(YAML)
    kw = run.trainer_kwargs(cfg.lightning.trainer)
    assert kw == {"gradient_clip_val": 1.0, "precision": 32, "detect_anomaly": True}
    assert run.trainer_kwargs(Config.create())["detect_anomaly"] is None


def test_trainer_accepts_detect_anomaly():
    import inspect
    from odvae_amd.trainer import AnomalyError, Trainer
    assert "detect_anomaly" in inspect.signature(Trainer.__init__).parameters
    assert issubclass(AnomalyError, RuntimeError)


def test_message_starts_with_torchs_sentence():
    from odvae_amd import anomaly
    d = anomaly.Detector("nan")
    msg = d.message("_Conv3x3Backward", 0, "decoder.up.2.block.1.conv1")
    assert msg.startswith("Function '_Conv3x3Backward' returned nan values in its 0th output.")
    assert "decoder.up.2.block.1.conv1" in msg


def test_dense_layouts_are_scanned_in_place():
    """Any stride order counts as dense (channels-last included); slices with gaps and broadcast views do not."""
    import torch
    from odvae_amd import anomaly
    cl = torch.empty(2, 5, 3, 8).permute(0, 3, 1, 2)
    assert anomaly.dense(cl) and anomaly.dense(torch.empty(4, 6).t()) and anomaly.dense(torch.empty(9)[3:])
    assert not anomaly.dense(cl[:, 1:]) and not anomaly.dense(torch.empty(4, 6)[:, ::2])
    assert not anomaly.dense(torch.empty(1, 3, 1, 1).expand(2, 3, 1, 1))
