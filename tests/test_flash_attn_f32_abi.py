"""C ABI of the fused f32 attention (flash_attn_f32.hip): exported and declared, the shape query, and host-side argument checks that
return an error before anything touches a device.  Runs without a GPU."""
import ctypes

import pytest

SYMBOLS = ("odvae_flash_attn_f32_supported", "odvae_flash_attn_fwd_f32", "odvae_flash_attn_bwd_f32")


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


@pytest.mark.parametrize("c", [64, 128, 256, 512])
@pytest.mark.parametrize("n,t", [(1, 1), (3, 45), (32, 4096), (2, 16384), (32, 16384), (65535, 7)])
def test_supported_accepts(built_lib, n, t, c):
    assert built_lib.load().odvae_flash_attn_f32_supported(n, t, c) == 1


@pytest.mark.parametrize("n,t,c", [(0, 16, 64), (-1, 16, 64), (65536, 16, 64), (1, 0, 64), (1, -5, 64),
                                   (1, 16, 0), (1, 16, 32), (1, 16, 48), (1, 16, 96), (1, 16, 192), (1, 16, 320), (1, 16, 1024)])
def test_supported_rejects(built_lib, n, t, c):
    assert built_lib.load().odvae_flash_attn_f32_supported(n, t, c) == 0


def test_bad_arguments_fail_on_the_host(built_lib):
    """Null, misaligned and unsupported arguments return ODVAE_ERR_ARG (1) with a message; the check comes before any launch,
    so these calls are safe without a device (the pointers are never dereferenced)."""
    h = built_lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    null = ctypes.c_void_p(0)
    fwd, bwd = h.odvae_flash_attn_fwd_f32, h.odvae_flash_attn_bwd_f32
    assert fwd(null, 1, 4, 64, 0.125, p, p, null) == 1
    assert b"null" in h.odvae_last_error()
    assert fwd(p, 1, 4, 64, 0.125, null, p, null) == 1
    assert fwd(p, 1, 4, 64, 0.125, p, null, null) == 1
    assert fwd(p, 1, 4, 48, 0.125, p, p, null) == 1
    assert b"unsupported" in h.odvae_last_error()
    assert fwd(p, 0, 4, 64, 0.125, p, p, null) == 1
    assert fwd(odd, 1, 4, 64, 0.125, p, p, null) == 1
    assert b"misaligned" in h.odvae_last_error()
    assert bwd(p, p, p, p, 1, 4, 64, 0.125, p, null, null) == 1
    assert bwd(p, p, null, p, 1, 4, 64, 0.125, p, p, null) == 1
    assert bwd(p, p, p, p, 1, 0, 64, 0.125, p, p, null) == 1
    assert bwd(p, p, p, p, 1, 4, 100, 0.125, p, p, null) == 1
    assert bwd(p, p, p, p, 1, 4, 64, 0.125, odd, p, null) == 1
    assert b"misaligned" in h.odvae_last_error()
