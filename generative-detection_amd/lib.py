"""ctypes binding of libodvae_hip.so, derived from include/odvae_hip.h at import: the prototypes and the ABI version are
parsed from the header, never written out here.  The product path has no CPU fallback: every op raises if the library is
missing or the tensors are not on a HIP device."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libodvae_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "odvae_hip.h")

_c = ctypes
_I = _c.c_int

_CTYPES = {"int": _c.c_int, "int64_t": _c.c_int64, "float": _c.c_float, "double": _c.c_double, "size_t": _c.c_size_t,
           "uint64_t": _c.c_uint64, "unsigned long long": _c.c_uint64}
_RESTYPES = {"int": _c.c_int, "size_t": _c.c_size_t, "const char*": _c.c_char_p}


class HipLibraryError(RuntimeError):
    """libodvae_hip.so is missing, stale or a kernel call failed."""


def _header_text(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise HipLibraryError("C ABI header %s cannot be read: %s" % (path, e)) from e


def parse_header(text):
    """name -> (restype, argtypes) of every `ret odvae_name(params);` in the text of a C header.  Every pointer or array
    parameter binds as c_void_p; a type the tables above do not know raises, so a new one cannot bind as int unnoticed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([^;{}()]*?)\b(odvae_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        decl = "%s %s(%s)" % (" ".join(ret.split()), name, " ".join(params.split()))
        ret = re.sub(r"\s*\*\s*", "*", " ".join(ret.split()))
        if ret not in _RESTYPES or name in protos:
            raise HipLibraryError("header declaration %r: %s" % (decl, "declared twice" if name in protos else "unknown return type"))
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            if "*" in param or "[" in param:
                args.append(_c.c_void_p)
                continue
            words = param.split()
            ctype = _CTYPES.get(" ".join(words[:-1])) or _CTYPES.get(" ".join(words))    # with or without a parameter name
            if ctype is None:
                raise HipLibraryError("header declaration %r: unknown parameter type %r" % (decl, " ".join(words)))
            args.append(ctype)
        protos[name] = (_RESTYPES[ret], args)
    stray = set(re.findall(r"\b(odvae_[a-z0-9_]+)\s*\(", text)) - set(protos)
    if stray:
        raise HipLibraryError("header mentions %s outside a declaration of the form `ret odvae_name(params);`" % sorted(stray))
    return protos


def header_symbols(path=HEADER_PATH):
    """Function names declared in include/odvae_hip.h."""
    return sorted(parse_header(_header_text(path)))


def _abi_version(text):
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+ODVAE_ABI_VERSION[ \t]+(\d+)", text, flags=re.M)
    if m is None:
        raise HipLibraryError("%s does not #define ODVAE_ABI_VERSION" % HEADER_PATH)
    return int(m.group(1))


# The header is the one declaration of the C ABI: the sources compile against it (csrc/common.h includes it) and the binding
# is derived from it here, at import.  name -> (restype, argtypes)
PROTOTYPES = parse_header(_header_text(HEADER_PATH))
ABI_VERSION = _abi_version(_header_text(HEADER_PATH))   # the header's #define; odvae_abi_version() returns the same macro


_lib = None


def load():
    """dlopen the in-tree library and declare every prototype.  Raises HipLibraryError when it is absent
    (build it with `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            "HIP kernel library %s not found; run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the OD-VAE hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    # the version first: a stale prebuilt library then fails here, with a message that says so, not at some symbol lookup
    try:
        lib.odvae_abi_version.restype = _I
        have = lib.odvae_abi_version()
    except AttributeError as e:
        raise HipLibraryError("%s does not export odvae_abi_version (not an OD-VAE kernel library?)" % LIB_PATH) from e
    if have != ABI_VERSION:
        raise HipLibraryError("ABI version mismatch: library %d, binding %d (stale libodvae_hip.so? rebuild with __graft_entry__.build())"
                              % (have, ABI_VERSION))
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError("%s does not export %s (stale build?)" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.odvae_abi_version() != ABI_VERSION:
        raise HipLibraryError("ABI version mismatch: library %d, binding %d (stale libodvae_hip.so? rebuild with __graft_entry__.build())"
                              % (lib.odvae_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().odvae_last_error().decode("utf-8", "replace")
        raise HipLibraryError("%s failed (code %d): %s" % (what, rc, msg))


WGRAD_PLAN_FIELDS = ("kind", "ntiles", "nsplit", "tiles_per_split", "ci_tiles", "co_tiles", "tile_rows", "effective_mode")
WGRAD_KINDS = ("thin", "v1", "v2", "up")


def conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout):
    """odvae_conv3x3_wgrad_plan as a dict (kind by name); host only, needs no device.  hi, wi are the input's."""
    out = (_I * 8)()
    check(load().odvae_conv3x3_wgrad_plan(mode, n, hi, wi, cin, cout, out), "odvae_conv3x3_wgrad_plan")
    plan = dict(zip(WGRAD_PLAN_FIELDS, out))
    plan["kind"] = WGRAD_KINDS[plan["kind"]]
    return plan


def conv_wgrad_bf16_plan(mode, n, ho, wo, cin, cout):
    """odvae_conv_wgrad_bf16_plan as a dict; host only, needs no device.  ho, wo are the OUTPUT's (dy's)."""
    out = (_I * 4)()
    check(load().odvae_conv_wgrad_bf16_plan(mode, n, ho, wo, cin, cout, out), "odvae_conv_wgrad_bf16_plan")
    return dict(zip(("nsplit", "ntiles", "tile_rows", "tile_cols"), out))


def stream_ptr():
    """hipStream_t of torch's current stream, as an integer for ctypes."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def require_device(*tensors, dtypes=(torch.float32,)):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipLibraryError(
                "OD-VAE HIP op called with a %s tensor: the hot path runs only on a HIP device (no CPU fallback)" % t.device)
        if t is not None and t.dtype not in dtypes:
            raise HipLibraryError("OD-VAE HIP op needs %s tensors, got %s" % (" / ".join(str(d) for d in dtypes), t.dtype))


class _Workspace:
    """One grow-only scratch buffer per device; kernels on one stream use it back to back."""

    def __init__(self):
        self.buf = {}

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 16384)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b.data_ptr(), b.numel()


workspace = _Workspace()


class _Uploader:
    """Host -> device copies that do not stall the host.  `tensor.to(device)` from pageable memory synchronises the
    stream first (the host waits for every kernel already queued), which stops the host from running ahead of the GPU
    four times per forward pass (the reference draws its noise on the CPU, autoencoder.py:239-240).  Here the data is
    copied into a small ring of pinned staging buffers and sent with an asynchronous copy on the current stream; an event
    per slot keeps a buffer from being reused before its copy has run."""

    SLOTS = 8

    def __init__(self):
        self.rings = {}

    def __call__(self, t, device):
        device = torch.device(device)
        if t.device == device:
            return t
        if t.is_cuda or device.type != "cuda":
            return t.to(device)
        key = (t.dtype, t.numel())
        ring = self.rings.get(key)
        if ring is None:
            ring = self.rings[key] = {"next": 0, "slots": [None] * self.SLOTS}
        i = ring["next"]
        ring["next"] = (i + 1) % self.SLOTS
        slot = ring["slots"][i]
        if slot is None:
            slot = ring["slots"][i] = (torch.empty(t.numel(), dtype=t.dtype, pin_memory=True), torch.cuda.Event())
        else:
            slot[1].synchronize()   # eight copies ago: long done in practice
        slot[0].copy_(t.reshape(-1))
        out = slot[0].to(device, non_blocking=True).view(t.shape)
        slot[1].record(torch.cuda.current_stream(device))
        return out


upload = _Uploader()
