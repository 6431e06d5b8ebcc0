"""Timing of the direct 3x3 weight-gradient kernels of the Upsample (mode 5, parity classes) and Downsample (mode 1) convs on the layer
shapes of the headline step: per shape ten launches behind device events, after 30 warm-up launches on a full queue, of the f32 MFMA form
and of the bf16-split form (odvae_conv3x3_wgrad_select).  A library without the selector (a build of an earlier commit, in whose tree this
file can be dropped) is timed as "parent".  `time all` adds one shape per kernel kind the step does not reach (v2 in modes 0 and 2, v1 in
modes 0 and 1, mode 5 falling back to v1).  `pmc`: six launches per form of one shape per mode, for a rocprofv3 --pmc pass (a run of its
own, no tracing).  ODVAE_PROBE_LIB names another build of the library (A/B runs).  python tools/wgrad_direct_probe.py [time [all]|pmc]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odvae_amd import lib as _lib, ops

dev = "cuda:0"
if os.environ.get("ODVAE_PROBE_LIB"):      # A/B builds of the library (tools/bin/, not shipped)
    _lib.LIB_PATH = os.environ["ODVAE_PROBE_LIB"]
L = _lib.load()
HAS_SELECT = hasattr(L, "odvae_conv3x3_wgrad_select")

# (mode, B, Cin, Cout, INPUT H = W): the four Upsample convs and the four Downsample convs of bench.py's step (256^2, B = 32)
STEP_SHAPES = [(5, 32, 512, 512, 16), (5, 32, 256, 256, 32), (5, 32, 256, 256, 64), (5, 32, 128, 128, 128),
               (1, 32, 128, 128, 256), (1, 32, 128, 128, 128), (1, 32, 256, 256, 64), (1, 32, 256, 256, 32)]
# the kinds the step does not reach: v2 mode 0, v2 mode 2, v1 (Cout <= 64) modes 0 and 1, mode 5 with a channel count that is no multiple of 4
OTHER_KINDS = [(0, 8, 128, 128, 128), (2, 8, 128, 128, 64), (0, 8, 128, 64, 128), (1, 8, 128, 64, 128), (5, 8, 128, 126, 64)]


def run(mode, x, dy, cin, cout):
    n, hi, wi = x.shape[0], x.shape[1], x.shape[2]
    ho, wo = dy.shape[1], dy.shape[2]
    dw = torch.empty(cout, cin, 3, 3, device=dev)
    db = torch.empty(cout, device=dev)
    wp, wn = ops._ws(L.odvae_conv3x3_wgrad_workspace_bytes(mode, n, ho, wo, cin, cout), x)
    _lib.check(L.odvae_conv3x3_wgrad_f32(mode, x.data_ptr(), dy.data_ptr(), n, hi, wi, cin, ho, wo, cout, dw.data_ptr(), db.data_ptr(),
                                         wp, wn, _lib.stream_ptr()), "wgrad")
    return dw, db


def launches_ms(fn, n=10):
    """n launches, each behind its own pair of device events"""
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def time_(shapes):
    for (mode, b, cin, cout, hi) in shapes:
        ho = hi if mode == 0 else hi // 2 if mode == 1 else 2 * hi
        x = torch.randn(b, hi, hi, cin, device=dev)
        dy = torch.randn(b, ho, ho, cout, device=dev)
        gf = 2.0 * 9 * cin * cout * b * ho * ho / 1e9
        res = {}
        for form in ((0, 1) if HAS_SELECT else ("parent",)):
            def fn():
                if form == "parent":
                    return run(mode, x, dy, cin, cout)
                prev = L.odvae_conv3x3_wgrad_select(form)
                try:
                    return run(mode, x, dy, cin, cout)
                finally:
                    L.odvae_conv3x3_wgrad_select(prev)
            for _ in range(30): fn()      # clock ramp, full queue
            torch.cuda.synchronize()
            ts = launches_ms(fn)
            res[form] = (fn()[0], sum(ts) / len(ts), min(ts), max(ts))
            print("mode %d B%d %d->%d in %d^2 out %d^2  %-7s mean %.4f ms  min %.4f  max %.4f  %.1f TFLOP/s (dense-form FLOPs)"
                  % (mode, b, cin, cout, hi, ho, "form %s" % form if form != "parent" else form, res[form][1], res[form][2], res[form][3],
                     gf / res[form][1]), flush=True)
        torch.cuda.synchronize()
        if HAS_SELECT:
            same = torch.equal(res[0][0], res[1][0])
            sup = L.odvae_conv3x3_wgrad_split_supported(mode, b, hi, hi, cin, cout)
            print("   supported %d; split / f32 = %.3f; slowest split %s fastest f32%s;  max |split - f32| / max |f32| = %.2e"
                  % (sup, res[1][1] / res[0][1], "<" if res[1][3] < res[0][2] else ">=",
                     " (same bits: the split form does not serve this shape)" if same else "",
                     (res[1][0] - res[0][0]).abs().max().item() / res[0][0].abs().max().item()), flush=True)


def pmc():
    for (mode, b, cin, cout, hi) in (STEP_SHAPES[2], STEP_SHAPES[4]):
        ho = 2 * hi if mode == 5 else hi // 2
        x = torch.randn(b, hi, hi, cin, device=dev)
        dy = torch.randn(b, ho, ho, cout, device=dev)
        for form in (0, 1):
            prev = L.odvae_conv3x3_wgrad_select(form)
            try:
                for _ in range(6): run(mode, x, dy, cin, cout)
            finally:
                L.odvae_conv3x3_wgrad_select(prev)
            torch.cuda.synchronize()


if __name__ == "__main__":
    pmc() if len(sys.argv) > 1 and sys.argv[1] == "pmc" else time_(STEP_SHAPES + (OTHER_KINDS if "all" in sys.argv[2:] else []))
