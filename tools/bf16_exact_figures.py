"""The figures of profiles/bf16_exact.md: per case group of tests/test_bf16_exact_gpu.py the elements compared, the share of bf16 outputs
that needed rounding, the share of exact ties, and the largest sum of |terms| in units against 2^24.  Host only (float64 references).
    python tools/bf16_exact_figures.py
"""
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_inputs as E            # noqa: E402
import test_bf16_exact_gpu as T     # noqa: E402

NAMES = {0: "3x3", 1: "Downsample", 2: "Upsample", 4: "1x1"}


def main():
    groups = OrderedDict()
    for lst, backward, tag in ((T.CONV_CASES, True, "fwd + bwd"), (T.FWD_ONLY_CASES, False, "forward only")):
        for recipe, mode, n, cin, cout, h, w in lst:
            c = E.make_case(recipe, mode, n, cin, cout, h, w)
            s = E.assert_exactly_summable(c)
            r = E.references(c)
            g = groups.setdefault("%s %s, %s" % (recipe, NAMES[mode], tag), {"cases": 0, "elems": 0, "bf": 0, "inexact": 0.0, "ties": 0.0, "worst": 0.0})
            outs = [r["y_exact"]] + ([r["dx_exact"]] if backward else [])
            g["cases"] += 1
            g["elems"] += r["y"].numel() + (r["dx"].numel() + r["dw"].numel() + r["db"].numel() + r["dres"].numel() if backward else 0)
            for o in outs:
                a, b = E.rounding_profile(o)
                g["bf"] += o.numel(); g["inexact"] += a * o.numel(); g["ties"] += b * o.numel()
            g["worst"] = max(g["worst"], s["worst"])
    for n, cin, cout, h, w in T.STATS_CASES:
        c = E.make_case("C", 0, n, cin, cout, h, w)
        s = E.assert_exactly_summable(c, stats_groups=32)
        r = E.references(c, stats_groups=32)
        g = groups.setdefault("C 3x3 + statistics", {"cases": 0, "elems": 0, "bf": 0, "inexact": 0.0, "ties": 0.0, "worst": 0.0})
        a, b = E.rounding_profile(r["y_exact"])
        g["cases"] += 1; g["elems"] += r["y"].numel() + r["partials"].numel(); g["bf"] += r["y"].numel()
        g["inexact"] += a * r["y"].numel(); g["ties"] += b * r["y"].numel(); g["worst"] = max(g["worst"], s["worst"])
    print("| case group | cases | elements compared | bf16 outputs that needed rounding | exact ties | largest sum of \\|terms\\| (units; limit 1.68e7) |")
    print("|---|---|---|---|---|---|")
    for name, g in groups.items():
        print("| %s | %d | %d | %.1f %% | %.1f %% | %.3g |" % (name, g["cases"], g["elems"], 100 * g["inexact"] / g["bf"], 100 * g["ties"] / g["bf"], g["worst"]))


if __name__ == "__main__":
    main()
