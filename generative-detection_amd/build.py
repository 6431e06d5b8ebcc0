"""Builds libodvae_hip.so (gfx950) in-tree with hipcc.  No torch headers: the library is a plain C ABI."""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")   # odvae_hip.h: every source compiles against the public declarations
OBJ_DIR = os.path.join(HERE, "build")
LIB_PATH = os.path.join(HERE, "libodvae_hip.so")
HIP_SOURCES = ["gemm_f32.hip", "gemm_f32_split.hip", "conv3x3_f32.hip", "conv3x3_wino_f32.hip", "conv3x3_wino4_f32.hip", "conv3x3_wgrad_f32.hip", "conv4x4_wgrad_f32.hip", "conv3x3_wgrad_wino_f32.hip", "groupnorm.hip", "elementwise.hip",
               "gan_f32.hip", "gan_norm.hip", "lpips_f32.hip", "patch_u8.hip", "pose_f32.hip", "linear_f32.hip",
               "conv_bf16.hip", "conv_wgrad_bf16.hip", "flash_attn_bf16.hip", "bf16_ops.hip", "lpips_bf16.hip",
               "flash_attn_f32.hip", "linattn_f32.hip", "anomaly.hip", "latent_noise.hip", "vq_f32.hip"]
CXX_SOURCES = ["runtime.cpp"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", CSRC, "-I", INCLUDE]
# Per-file code-generation switches (none in use).  Tried on flash_attn_bf16.hip: `-mllvm -amdgpu-mfma-vgpr-form=1` removes the
# 256 v_accvgpr_read/write per 32 MFMAs that hipcc's default register split puts at the loop back-edge of the attention kernels
# (592 vs 565 TFLOP/s forward), but the D >= 256 forward kernels then return wrong results (tests/test_bf16_gpu.py), so it stays off.
# In use: -fno-slp-vectorize for the attention file and the bf16-split GEMM (its row sums and splits sit beside MFMAs too).  At -O3 hipcc packs adjacent f32 multiplies / adds of the softmax sections into
# v_pk_mul_f32 / v_pk_add_f32; beside MFMAs a packed f32 op costs more issue time than the two plain ones it replaces
# (MI355X_MICROARCH.md, "price of one filler beside MFMAs").
PER_FILE_FLAGS = {"flash_attn_bf16.hip": ["-fno-slp-vectorize"], "gemm_f32_split.hip": ["-fno-slp-vectorize"]}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps(src):
    """What an object is rebuilt for: its source, every header there is (not a list of them: a new header cannot leave stale
    objects behind), the public header and this file (the flags)."""
    return [src, os.path.join(INCLUDE, "odvae_hip.h"), os.path.abspath(__file__)] + glob.glob(os.path.join(CSRC, "*.h"))


def _compile(src):
    obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
    if _stale(obj, _deps(src)):
        cmd = [HIPCC] + FLAGS + PER_FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
    return obj


def build_library(force=False, verbose=False):
    """Compile every kernel source for gfx950 and link the shared library.  Returns its path."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES + CXX_SOURCES]
    missing = [s for s in srcs if not os.path.exists(s)]
    if missing:
        raise FileNotFoundError("listed in HIP_SOURCES / CXX_SOURCES but not in %s: %s" % (CSRC, ", ".join(map(os.path.basename, missing))))
    if force:
        for f in os.listdir(OBJ_DIR):
            os.remove(os.path.join(OBJ_DIR, f))
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(_compile, srcs))
    if force or _stale(LIB_PATH, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stderr[-4000:])
    if verbose:
        print("built", LIB_PATH, file=sys.stderr)
    return LIB_PATH


if __name__ == "__main__":
    build_library(force="--force" in sys.argv, verbose=True)
