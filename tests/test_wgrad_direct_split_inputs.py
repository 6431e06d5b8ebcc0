"""The cases of tests/wgrad_direct_split_cases.py against the plan the library reports and against its gate
(odvae_conv3x3_wgrad_split_supported).  Host only: neither query launches anything nor needs a device.  Without these assertions a GPU
case could silently run the f32 kernel, or miss the property it is listed for."""
import pytest

import wgrad_direct_inputs as W
import wgrad_direct_split_cases as C


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_is_admitted_and_has_the_properties_it_is_listed_for(lib, name):
    mode, n, cin, cout, hi, wi, expect = C.CASES[name]
    assert lib.load().odvae_conv3x3_wgrad_split_supported(mode, n, hi, wi, cin, cout) == 1
    plan = lib.conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout)
    print(name, plan)
    got = C.properties(plan, n, hi, wi, cin, cout)
    assert {k: got[k] for k in expect} == expect, "%s: the library plans %s" % (name, plan)
    W.make_exact(mode, n, cin, cout, hi, wi, W.case_seed(name))      # asserts sum |x| |dy| < 2^24


@pytest.mark.parametrize("mode", [5, 1])
def test_the_cases_cover_each_split_kernel_between_them(lib, mode):
    of = [C.properties(lib.conv3x3_wgrad_plan(m, n, hi, wi, cin, cout), n, hi, wi, cin, cout)
          for (m, n, cin, cout, hi, wi, _) in C.CASES.values() if m == mode]
    assert any(p["tiles_per_split"] == 1 for p in of)                                # a block that never comes back to a buffer
    assert any(p["tiles_per_split"] >= 4 and p["last"] < p["tiles_per_split"] for p in of)      # both buffers reused; a short last split
    assert any(p["crosses_images"] for p in of)
    for key in ("ragged_w", "ragged_h", "ragged_ci", "ragged_co"):
        assert any(p[key] for p in of), key
    assert any(p["ci_tiles"] > 1 and p["co_tiles"] > 1 for p in of)
    if mode == 5:      # its loop steps by tile: two tiles per block use each buffer once, an odd count ends on the first
        assert any(p["tiles_per_split"] == 2 for p in of)
        assert any(p["last"] % 2 == 1 and p["last"] > 1 for p in of)


@pytest.mark.parametrize("name", list(C.ADMITTED_BY_THE_RULE))
def test_the_rule_cases_sit_on_the_edge_of_the_rule(lib, name):
    mode, n, cin, cout, hi, wi = C.ADMITTED_BY_THE_RULE[name]
    assert lib.load().odvae_conv3x3_wgrad_split_supported(mode, n, hi, wi, cin, cout) == 1
    plan = lib.conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout)
    assert plan["tiles_per_split"] == 16 and plan["ntiles"] == 16 * plan["nsplit"], plan
    assert cin % 64 == 0 and cout % 128 == 0 and min(cin, cout) >= 128


@pytest.mark.parametrize("name", list(C.BELOW_THE_GATE))
def test_calls_below_the_gate_are_not_admitted(lib, name):
    mode, n, cin, cout, hi, wi = C.BELOW_THE_GATE[name]
    assert lib.load().odvae_conv3x3_wgrad_split_supported(mode, n, hi, wi, cin, cout) == 0
    plan = lib.conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout)
    assert plan["kind"] != "up" and not (plan["kind"] == "v2" and plan["effective_mode"] == 1)


def test_the_gate_is_the_two_kernels_with_a_split_form(lib):
    """admitted exactly where the plan is the parity-class kernel, or the LDS-DMA kernel in mode 1; an empty shape is not admitted"""
    L = lib.load()
    for mode in (0, 1, 2, 5):
        for cin, cout in ((64, 64), (128, 256), (4, 4), (4, 68), (66, 128), (64, 3), (3, 64)):
            plan = lib.conv3x3_wgrad_plan(mode, 2, 8, 16, cin, cout)
            want = plan["kind"] == "up" or (plan["kind"] == "v2" and plan["effective_mode"] == 1)
            assert L.odvae_conv3x3_wgrad_split_supported(mode, 2, 8, 16, cin, cout) == int(want), (mode, cin, cout, plan)
    assert L.odvae_conv3x3_wgrad_split_supported(5, 0, 8, 16, 64, 64) == 0
    assert L.odvae_conv3x3_wgrad_split_supported(7, 2, 8, 16, 64, 64) == 0


def test_selector_returns_the_previous_setting_and_clamps(lib):
    L = lib.load()
    first = L.odvae_conv3x3_wgrad_select(1)
    try:
        assert first == -1, "the default is the shape rule"
        assert L.odvae_conv3x3_wgrad_select(0) == 1
        assert L.odvae_conv3x3_wgrad_select(7) == 0
        assert L.odvae_conv3x3_wgrad_select(-5) == 1
        assert L.odvae_conv3x3_wgrad_select(-1) == -1
    finally:
        L.odvae_conv3x3_wgrad_select(first)
