"""Cases for the bf16-split form of the direct 3x3 weight-gradient kernels (csrc/conv3x3_wgrad_f32.hip, odvae_conv3x3_wgrad_select), for
tests/test_wgrad_direct_split_inputs.py (host) and tests/test_wgrad_direct_split_gpu.py.  Operands and the float64 gradient come from
tests/wgrad_direct_inputs.py.  Plain module: no fixtures, no device.

name -> (mode, n, cin, cout, INPUT hi, wi, expectation); the expectation names properties of the plan the library reports
(wgrad_direct_inputs.plan_properties) plus
    ci_tiles, co_tiles   channel tiles of the plan
    ragged_w             the tiled width (mode 5: the input's, mode 1: the output's) is no multiple of 16: the last tile of a row has
                         columns outside the image
    ragged_h             ... the tiled height no multiple of the tile's 2 rows
    ragged_ci, ragged_co the last channel tile (64 ci; 64 co in mode 5, 128 co in mode 1) is not full
    crossing_split       index of a split whose tiles belong to two images
The split form serves the parity-class kernel (mode 5, both channel counts multiples of 4) and the Downsample conv where it gets the
LDS-DMA kernel (mode 1, both channel counts multiples of 4, Cout > 64).  In mode 1 every tile reads the zero pad: the halo row below
an image's last tile row is row Hi, the halo column right of a row's last tile is column Wi (where the width is ragged, further
columns too).
"""
import wgrad_direct_inputs as W

CASES = {
    # 27 tiles of 2 x 16 low-res pixels (3 per row of 36), 7 x 5 channel tiles, 7 splits of 4: split 2 = tiles 8 .. 11 crosses from image
    # 0 (tiles 0 .. 8) into image 1, the last split holds 3
    "up-4-per-block": (5, 3, 448, 320, 6, 36, dict(kind="up", effective_mode=5, ntiles=27, nsplit=7, tiles_per_split=4, last=3, crosses_images=True,
                                                   ci_tiles=7, co_tiles=5, ragged_w=True, crossing_split=2)),
    # one tile per block at the smallest channel counts the kernel takes; 3 x 5 low-res pixels: both tile rows and columns ragged
    "up-smallest": (5, 2, 4, 4, 3, 5, dict(kind="up", effective_mode=5, ntiles=4, nsplit=4, tiles_per_split=1, last=1, ci_tiles=1, co_tiles=1,
                                           ragged_w=True, ragged_h=True, ragged_ci=True, ragged_co=True)),
    # channel tiles with a ragged tail on both axes (68 = 64 + 4, 36), two tiles per block (130 tiles are the fewest with two channel
    # tiles): both LDS buffers, whole tiles only
    "up-ragged-channels": (5, 1, 68, 36, 20, 208, dict(kind="up", effective_mode=5, ntiles=130, nsplit=65, tiles_per_split=2, last=2, ci_tiles=2,
                                                       co_tiles=1, ragged_w=False, ragged_h=False, ragged_ci=True, ragged_co=True)),
    # 42 tiles of 2 x 16 output pixels (3 per row of 40, 7 tile rows of 14), 7 x 3 channel tiles, the last co tile 64 of 128 wide,
    # 11 splits of 4: split 5 = tiles 20 .. 23 crosses from image 0 (tiles 0 .. 20) into image 1, the last split holds 2
    "down-4-per-block": (1, 2, 448, 320, 28, 80, dict(kind="v2", effective_mode=1, ntiles=42, nsplit=11, tiles_per_split=4, last=2, crosses_images=True,
                                                      ci_tiles=7, co_tiles=3, ragged_w=True, ragged_h=False, ragged_co=True, crossing_split=5)),
    # one tile per block at the smallest channel counts the gate admits (Cout > 64); 3 x 5 output pixels: the second tile has one row
    "down-smallest": (1, 1, 4, 68, 6, 10, dict(kind="v2", effective_mode=1, ntiles=2, nsplit=2, tiles_per_split=1, last=1, ci_tiles=1, co_tiles=1,
                                               ragged_w=True, ragged_h=True, ragged_ci=True, ragged_co=True)),
}
ACCURACY_SHAPES = {5: "up-4-per-block", 1: "down-4-per-block"}
# the smallest shapes the default shape rule admits: 16 tiles per block (1 024 tiles over 64 blocks per channel tile pair; 512 over 32),
# full channel tiles of at least 128 channels.  (mode, n, cin, cout, INPUT hi, wi)
ADMITTED_BY_THE_RULE = {
    "up-rule": (5, 4, 128, 128, 32, 256),
    "down-rule": (1, 4, 256, 256, 64, 256),
}
# calls the split form does not serve: they must give the f32 kernels' bits under every setting
BELOW_THE_GATE = {
    "m1-v1": (1, 2, 128, 64, 12, 40),             # Downsample conv with Cout <= 64: the kernel without LDS-DMA
    "m5-falls-back-to-m2": (5, 2, 66, 66, 6, 20),      # channel counts that are no multiples of 4: dense form, v1
    "m0-v2": (0, 1, 128, 128, 8, 16),
}


def properties(plan, n, hi, wi, cin, cout):
    """wgrad_direct_inputs.plan_properties plus the tile and raggedness properties above"""
    got = W.plan_properties(plan, n, hi)
    ranges = W.split_ranges(plan)
    per_image = plan["ntiles"] // n
    crossing = [s for s, (a, b) in enumerate(ranges) if a // per_image != (b - 1) // per_image]
    th, tw = (hi, wi) if plan["kind"] == "up" else W.out_hw(plan["effective_mode"], hi, wi)      # what the tiles cover
    got.update(ci_tiles=plan["ci_tiles"], co_tiles=plan["co_tiles"], ragged_w=tw % 16 != 0, ragged_h=th % plan["tile_rows"] != 0,
               ragged_ci=cin % 64 != 0, ragged_co=cout % (64 if plan["kind"] == "up" else 128) != 0,
               crossing_split=crossing[0] if crossing else None)
    return got
