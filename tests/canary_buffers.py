"""Device buffers with canaries behind them, for the tests that call kernels through the C ABI: outputs pre-filled with NaN, so an
element a kernel skips shows, and PAD canary elements (64 canary bytes for a workspace) past the end, so a write past the end shows.
Plain helpers, no fixtures; every function needs a HIP device."""
import torch

DEV = "cuda:0"
CANARY = 12345.0
PAD = 8


def call(fn, *args):
    from odvae_amd import lib
    lib.check(fn(*args, lib.stream_ptr()), fn.__name__)


def out_buf(n, fill=float("nan")):
    """n output elements pre-filled with NaN and PAD canary elements behind them: (whole buffer, view of the n)"""
    buf = torch.full((int(n) + PAD,), fill, device=DEV)
    buf[int(n):] = CANARY
    return buf, buf[:int(n)]


def padded(t):
    """a device copy of t with PAD canary elements behind it: (whole buffer, view shaped like t)"""
    buf, view = out_buf(t.numel())
    view.copy_(t.reshape(-1))
    return buf, view.view(t.shape)


def assert_canary(*bufs):
    for b in bufs:
        assert (b[-PAD:] == CANARY).all().item(), "the kernel wrote past the end of an output"


def workspace(nbytes):
    """exactly nbytes of workspace with 64 canary bytes behind it"""
    buf = torch.full((int(nbytes) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf


def assert_workspace_canary(buf):
    assert (buf[-64:] == 0xA5).all().item(), "the kernel wrote past the workspace it asked for"
