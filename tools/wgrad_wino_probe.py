"""Winograd-domain weight gradient vs the direct weight-gradient kernel (both through the C ABI) and vs torch CPU on small
shapes; timing of its two main loops (f32 MFMA, bf16 split: odvae_conv3x3_wgrad_wino_select) and of the direct kernel on the layer
shapes of the headline step.  python tools/wgrad_wino_probe.py [check|time]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odvae_amd import lib as _lib, ops

dev = "cuda:0"
if os.environ.get("ODVAE_PROBE_LIB"):      # A/B builds of the library (tools/bin/, not shipped)
    _lib.LIB_PATH = os.environ["ODVAE_PROBE_LIB"]
L = _lib.load()


def run(kind, x, dy, cin, cout):
    n, h, w = x.shape[0], x.shape[1], x.shape[2]
    dw = torch.empty(cout, cin, 3, 3, device=dev)
    db = torch.empty(cout, device=dev)
    if kind == "wino":
        need = L.odvae_conv3x3_wgrad_wino_workspace_bytes(n, h, w, cin, cout)
        wp, wn = ops._ws(need, x)
        _lib.check(L.odvae_conv3x3_wgrad_wino_f32(x.data_ptr(), dy.data_ptr(), n, h, w, cin, cout, dw.data_ptr(), db.data_ptr(),
                                                  wp, wn, _lib.stream_ptr()), "wgrad_wino")
    else:
        need = L.odvae_conv3x3_wgrad_workspace_bytes(0, n, h, w, cin, cout)
        wp, wn = ops._ws(need, x)
        _lib.check(L.odvae_conv3x3_wgrad_f32(0, x.data_ptr(), dy.data_ptr(), n, h, w, cin, h, w, cout, dw.data_ptr(), db.data_ptr(),
                                             wp, wn, _lib.stream_ptr()), "wgrad")
    return dw, db


def check():
    for (n, cin, cout, h, w) in [(2, 128, 128, 16, 16), (1, 128, 256, 8, 12), (3, 256, 128, 6, 10), (2, 128, 128, 2, 2), (1, 384, 128, 4, 34)]:
        g = torch.Generator().manual_seed(n * 1000 + cin + h)
        x = torch.randn(n, cin, h, w, generator=g)
        dy = torch.randn(n, cout, h, w, generator=g)
        wt = torch.zeros(cout, cin, 3, 3, requires_grad=True)
        b = torch.zeros(cout, requires_grad=True)
        torch.nn.functional.conv2d(x, wt, b, padding=1).backward(dy)
        xd = x.to(dev).permute(0, 2, 3, 1).contiguous()
        dyd = dy.to(dev).permute(0, 2, 3, 1).contiguous()
        assert L.odvae_conv3x3_wgrad_wino_supported(n, h, w, cin, cout) == 1
        dw, db = run("wino", xd, dyd, cin, cout)
        dw2, db2 = run("direct", xd, dyd, cin, cout)
        torch.cuda.synchronize()
        s = wt.grad.abs().max().item()
        e1 = (dw.cpu() - wt.grad).abs().max().item() / s
        e2 = (dw2.cpu() - wt.grad).abs().max().item() / s
        eb = (db.cpu() - b.grad).abs().max().item() / b.grad.abs().max().item()
        print("N%d %d->%d %dx%d: wino rel err %.2e (direct %.2e), bias %.2e" % (n, cin, cout, h, w, e1, e2, eb), flush=True)
        assert e1 < 2e-4 and eb < 2e-4


# the stride-1 3x3 layers of the headline step (bench.py: 256^2, B = 32) that reach this kernel, and how often per step
STEP_SHAPES = [(32, 128, 128, 256, 10), (32, 128, 128, 128, 9), (32, 256, 128, 128, 1), (32, 256, 256, 64, 9), (32, 128, 256, 64, 1),
               (32, 256, 256, 32, 9), (32, 512, 256, 32, 1), (32, 512, 512, 16, 17), (32, 256, 512, 16, 1)]


def launches_ms(fn, n=10):
    """n launches, each behind its own pair of device events"""
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def time_():
    """Per shape: ten launches of each form (0 = f32 loop, 1 = bf16-split loop where supported) and of the direct kernel."""
    for (b, cin, cout, h, per_step) in STEP_SHAPES:
        x = torch.randn(b, h, h, cin, device=dev)
        dy = torch.randn(b, h, h, cout, device=dev)
        gf = 2.0 * 9 * cin * cout * b * h * h / 1e9
        res = {}
        for form in (0, 1, "direct"):
            def fn():
                if form == "direct":
                    return run("direct", x, dy, cin, cout)
                prev = L.odvae_conv3x3_wgrad_wino_select(form)
                try:
                    return run("wino", x, dy, cin, cout)
                finally:
                    L.odvae_conv3x3_wgrad_wino_select(prev)
            for _ in range(30): fn()      # clock ramp
            torch.cuda.synchronize()
            ts = launches_ms(fn)
            res[form] = (fn()[0], sum(ts) / len(ts), min(ts), max(ts))
            print("B%d %d->%d @%d x%d per step  %-7s mean %.4f ms  min %.4f  max %.4f  %.1f TFLOP/s (direct-form FLOPs)"
                  % (b, cin, cout, h, per_step, "form %s" % form if form != "direct" else form, res[form][1], res[form][2], res[form][3], gf / res[form][1]), flush=True)
        torch.cuda.synchronize()
        same = torch.equal(res[0][0], res[1][0])
        print("   split / f32 = %.3f%s;  max |wino - direct| / max|direct| = %.2e"
              % (res[1][1] / res[0][1], " (same bits: the split loop does not serve this shape)" if same else "",
                 (res["direct"][0] - res[1][0]).abs().max().item() / res["direct"][0].abs().max().item()), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "check"
    check() if what == "check" else time_()
