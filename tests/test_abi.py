"""The C ABI library builds for gfx950, loads without a GPU and exports exactly what include/odvae_hip.h declares; the ctypes
binding and the build derive from that header."""
import ctypes as c
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


def test_library_exports_every_header_symbol(built_lib):
    handle = built_lib.load()
    names = built_lib.header_symbols()
    assert len(names) >= 30
    assert "odvae_groupnorm_recentred" in names and "odvae_device_health" in names
    for name in names:
        assert hasattr(handle, name), name


def test_binding_table_matches_header(built_lib):
    assert sorted(built_lib.PROTOTYPES) == built_lib.header_symbols()


# ---- the parser, on synthetic header text ------------------------------------------------------------------------------------------
def _parse(text):
    from odvae_amd import lib
    return lib.parse_header(text)


def test_parser_reads_a_declaration_spread_over_lines():
    got = _parse("#include <stddef.h>\nint odvae_a(int M,\n            float alpha /* scale */,\n"
                 "            int64_t stride,\n            void* stream);\nsize_t odvae_b(double p, unsigned long long seed, size_t n);\n")
    assert got == {"odvae_a": (c.c_int, [c.c_int, c.c_float, c.c_int64, c.c_void_p]),
                   "odvae_b": (c.c_size_t, [c.c_double, c.c_uint64, c.c_size_t])}


def test_parser_ignores_comments_and_preprocessor_lines():
    got = _parse("/* call odvae_x(1, 2); first\n * int odvae_y(int a); */\n#define ODVAE_Z(a) odvae_z(a)\nint odvae_real(void);\n")
    assert got == {"odvae_real": (c.c_int, [])}


def test_parser_arrays_and_pointers_to_pointers_are_pointers():
    got = _parse("int odvae_p(int out[8], const float* const* src, uint64_t* record, uint64_t n);")
    assert got == {"odvae_p": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64])}


def test_parser_void_gives_no_arguments_and_char_pointer_returns():
    assert _parse("const char* odvae_s(void);\nconst char *odvae_t( void );") == {"odvae_s": (c.c_char_p, []), "odvae_t": (c.c_char_p, [])}


@pytest.mark.parametrize("text", ["int odvae_f(long foo);", "int odvae_f(int a, unsigned b);", "long odvae_f(int a);",
                                  "void odvae_f(int a);", "int odvae_f(int a); int odvae_f(int a);",
                                  "int odvae_f(void (*cb)(int));"])
def test_parser_rejects_what_it_does_not_know(text):
    from odvae_amd import lib
    with pytest.raises(lib.HipLibraryError, match="odvae_f"):
        lib.parse_header(text)


def test_missing_header_names_the_path(tmp_path):
    from odvae_amd import lib
    missing = str(tmp_path / "no_such_header.h")
    with pytest.raises(lib.HipLibraryError, match="no_such_header.h"):
        lib.header_symbols(missing)
    path = tmp_path / "small.h"
    path.write_text("int odvae_one(int a);\nsize_t odvae_two(void);\n")
    assert lib.header_symbols(str(path)) == ["odvae_one", "odvae_two"]


# ---- the real header: signatures written out here, so a changed type or a lost argument in the header or in the parser shows ---------
_P, _I, _L, _F, _Z, _D, _U = c.c_void_p, c.c_int, c.c_int64, c.c_float, c.c_size_t, c.c_double, c.c_uint64
PINNED = {
    # exactly the argtypes of the stub in INTEGRATION.md
    "odvae_groupnorm_fwd_f32": (_I, [_P] + [_I] * 4 + [_P] * 2 + [_F, _I] + [_P] * 4 + [_Z, _P]),
    "odvae_last_error": (c.c_char_p, []),
    "odvae_gemm_f32_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "odvae_colsum_f32": (_I, [_P, _L, _I, _P, _P, _Z, _P]),
    "odvae_groupnorm_fwd_drop_f32": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _I, _D, _U, _P, _P, _P, _P, _Z, _P]),
    "odvae_conv3x3_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "odvae_grad_accumulate_f32": (_I, [_P, _L, _P, _P, _P, _I, _P]),
    "odvae_anomaly_scan": (_I, [_P, _I, _L, _I, _P, _P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    from odvae_amd import lib
    assert lib.PROTOTYPES[name] == PINNED[name]


def test_library_exports_what_the_header_declares_and_nothing_else(built_lib):
    """The defined dynamic symbols with C linkage (a C++ symbol is mangled and starts with _Z) are the header's, plus the
    library's own error setter."""
    built_lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("odvae_"))
    assert exported == sorted(built_lib.header_symbols() + ["odvae_set_error"])


def test_abi_version_has_one_source(built_lib):
    handle = built_lib.load()
    assert built_lib.ABI_VERSION == handle.odvae_abi_version() == 4
    assert "#define ODVAE_ABI_VERSION 4" in open(built_lib.HEADER_PATH).read()
    pkg = os.path.dirname(built_lib.LIB_PATH)
    assert "return ODVAE_ABI_VERSION;" in open(os.path.join(pkg, "csrc", "runtime.cpp")).read()


# ---- build.py ------------------------------------------------------------------------------------------------------------------------
def test_build_raises_on_a_listed_source_that_does_not_exist(built_lib, monkeypatch):
    from odvae_amd import build
    monkeypatch.setattr(build, "HIP_SOURCES", build.HIP_SOURCES + ["no_such_kernel.hip"])
    with pytest.raises(FileNotFoundError, match="no_such_kernel.hip"):
        build.build_library()


def test_any_header_under_csrc_makes_objects_stale(built_lib, monkeypatch, tmp_path):
    """The header directory is globbed: a header nobody listed (here a new one, in a stand-in for csrc/) is a dependency."""
    from odvae_amd import build
    src = os.path.join(build.CSRC, "linear_f32.hip")
    obj = os.path.join(build.OBJ_DIR, "linear_f32.hip.o")
    assert os.path.exists(obj) and not build._stale(obj, build._deps(src))
    assert os.path.join(build.INCLUDE, "odvae_hip.h") in build._deps(src) and os.path.abspath(build.__file__) in build._deps(src)
    assert set(build._deps(src)) >= {os.path.join(build.CSRC, h) for h in os.listdir(build.CSRC) if h.endswith(".h")}
    monkeypatch.setattr(build, "CSRC", str(tmp_path))
    new = tmp_path / "brand_new.h"
    new.write_text("// nothing\n")
    later = os.path.getmtime(obj) + 10
    os.utime(new, (later, later))
    assert str(new) in build._deps(src) and build._stale(obj, build._deps(src))


def test_identification_calls(built_lib):
    handle = built_lib.load()
    assert handle.odvae_abi_version() == built_lib.ABI_VERSION == 4
    assert handle.odvae_target_arch() == b"gfx950"
    # pure host queries (no kernel launch)
    assert handle.odvae_conv3x3_pack_reduce_pad(3) == 32 and handle.odvae_conv3x3_pack_out_pad(3) == 32
    assert handle.odvae_conv3x3_pack_out_pad(256) == 256
    assert handle.odvae_conv3x3_pack_floats(128, 128) == 9 * 128 * 128
    assert handle.odvae_gemm_f32_workspace_bytes(128, 128, 1 << 20, 1) > 0
    assert handle.odvae_gemm_f32_workspace_bytes(4096, 4096, 256, 32) == 0


def test_product_path_fails_loudly_without_gpu(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from odvae_amd import ops
    with pytest.raises(built_lib.HipLibraryError):
        ops.group_norm(torch.randn(1, 32, 4, 4), torch.ones(32), torch.zeros(32), 32, 1e-6, True)
    with pytest.raises(built_lib.HipLibraryError):
        ops.conv3x3(torch.randn(1, 4, 4, 4), torch.randn(4, 4, 3, 3))


def test_no_product_module_imports_the_oracle():
    pkg = os.path.join(ROOT, "generative-detection_amd")
    seen = 0
    for where, _, files in os.walk(pkg):      # sub-packages too (ops/)
        for fn in files:
            if fn.endswith(".py"):
                text = open(os.path.join(where, fn)).read()
                assert "import oracle" not in text and "from oracle" not in text, os.path.join(where, fn)
                seen += 1
    assert seen > len([fn for fn in os.listdir(pkg) if fn.endswith(".py")]), "the walk did not reach the sub-packages"
