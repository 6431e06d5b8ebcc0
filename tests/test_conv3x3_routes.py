"""Which kernels an f32 3x3 conv call gets: ops._conv3x3_route on fixed shapes and under the A/B switches, and the pack kind / direct
weight-gradient mode of every route (ops.CONV3X3_ROUTES).  Host only: the route needs odvae_conv3x3_wino4_supported, no device."""
import pytest


@pytest.fixture(scope="module")
def ops(built_lib):
    from odvae_amd import ops
    return ops


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from odvae_amd import lib
    return lib


# (mode, input H, input W, Cin, Cout, fused ReLU) -> route, all switches at their defaults.  F(4x4) wants H, W in multiples of 4, H >= 16,
# W >= 32 (of the OUTPUT for an Upsample conv) and channels in multiples of 8 from 64; F(2x2) even H, W and channels in multiples of 4 from 16.
ROUTES = [
    (0, 256, 256, 128, 128, False, "wino4"),
    (0, 16, 32, 64, 64, False, "wino4"),
    (0, 256, 256, 64, 64, True, "wino2"),        # the ReLU VGG stack stays off F(4x4)
    (0, 16, 16, 512, 512, False, "wino2"),       # W < 32
    (0, 12, 32, 64, 64, False, "wino2"),         # H < 16
    (0, 18, 34, 128, 128, False, "wino2"),       # not multiples of 4
    (0, 64, 64, 32, 64, False, "wino2"),         # Cin < 64
    (0, 256, 256, 3, 128, False, "direct"),
    (0, 256, 256, 128, 3, False, "direct"),
    (0, 17, 32, 64, 64, False, "direct"),        # odd H
    (0, 64, 64, 16, 12, False, "direct"),        # Cout < 16
    (1, 64, 64, 128, 128, False, "down"),
    (2, 128, 128, 256, 256, False, "wino4_up"),
    (2, 8, 16, 64, 64, False, "wino4_up"),       # output 16 x 32
    (2, 11, 21, 64, 160, False, "up_parity"),    # output 22 x 42
    (2, 8, 8, 64, 64, False, "up_parity"),       # output W < 32
]


@pytest.mark.parametrize("mode,hi,wi,cin,cout,relu,route", ROUTES)
def test_route_at_default_switches(ops, mode, hi, wi, cin, cout, relu, route):
    assert ops._conv3x3_route(mode, hi, wi, cin, cout, relu) == route


# route with ONE switch turned off, for the two wino4_up rows and the first wino4 row
SWITCHED = [
    ((2, 128, 128, 256, 256, False), {"WINOGRAD": "up_parity", "WINOGRAD4": "up_parity", "UPCONV_WINOGRAD4": "up_parity", "UPCONV_BY_PARITY": "up_dense"}),
    ((2, 8, 16, 64, 64, False), {"WINOGRAD": "up_parity", "WINOGRAD4": "up_parity", "UPCONV_WINOGRAD4": "up_parity", "UPCONV_BY_PARITY": "up_dense"}),
    ((0, 256, 256, 128, 128, False), {"WINOGRAD": "direct", "WINOGRAD4": "wino2", "UPCONV_WINOGRAD4": "wino4", "UPCONV_BY_PARITY": "wino4"}),
]


@pytest.mark.parametrize("switch", ["WINOGRAD", "WINOGRAD4", "UPCONV_WINOGRAD4", "UPCONV_BY_PARITY"])
@pytest.mark.parametrize("call,expected", SWITCHED)
def test_route_with_one_switch_off(ops, monkeypatch, call, expected, switch):
    monkeypatch.setattr(ops, switch, False)
    assert ops._conv3x3_route(*call) == expected[switch]


def test_a_fused_relu_keeps_an_upsample_conv_off_the_f4_kernel(ops):
    assert ops._conv3x3_route(2, 128, 128, 256, 256, True) == "up_parity"


def test_unknown_mode_is_an_error(ops):
    with pytest.raises(ValueError):
        ops._conv3x3_route(3, 64, 64, 64, 64, False)


def test_pack_kind_and_direct_wgrad_mode_of_every_route(ops):
    assert {r: (e[0], e[3]) for r, e in ops.CONV3X3_ROUTES.items()} == {
        "direct": ("direct", 0), "down": ("direct", 1), "up_dense": ("direct", 2), "up_parity": ("up", 5),
        "wino2": ("wino", 0), "wino4": ("wino4", 0), "wino4_up": ("wino4", 5)}
    # the direct kernel's forward / data-gradient modes; None: a Winograd launcher
    assert {r: (e[1], e[2]) for r, e in ops.CONV3X3_ROUTES.items()} == {
        "direct": (0, 0), "down": (1, 3), "up_dense": (2, 0), "up_parity": (5, 6),
        "wino2": (None, None), "wino4": (None, None), "wino4_up": (None, None)}
