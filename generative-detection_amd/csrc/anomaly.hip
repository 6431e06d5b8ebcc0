// Device-side anomaly scan of backward outputs: the check torch.autograd.set_detect_anomaly(True) makes after every backward node
// (`isnan(output).any().item()` per output), without the host synchronisation per output (generative-detection_amd/anomaly.py).
//
// One launch covers up to 8 outputs of one backward node; their descriptors travel in the kernel-argument block (no host-to-device
// copy).  The test works on bit patterns, so no fast-math flag can fold it away:
//   f32  NaN  : (bits & 0x7fffffff) >  0x7f800000      nonfinite: >= 0x7f800000 (also +-Inf)
//   bf16 NaN  : (h    & 0x7fff)     >  0x7f80          nonfinite: >= 0x7f80
// Sign and quiet / signalling bit do not matter.  Each lane keeps the running maximum of the magnitude bits and compares once at the
// end: two VALU operations per element beside a 16-byte streaming load.  A wave that found something combines its keys with a
// 64-lane butterfly and one lane does a single 64-bit vector atomic min on the record: key = (node_seq << 20) | output_index, so the
// record ends up holding the earliest node and its lowest offending output.  Clean data issues no atomics.  No LDS.
#include "common.h"

#define ANOMALY_MAX_TENSORS 8

struct AnomalyTensorArg {
  const void* p;
  int64_t n;
  int dtype;   // 0 f32, 1 bf16
  int index;   // output index within the node
};

struct AnomalyArgs {
  AnomalyTensorArg t[ANOMALY_MAX_TENSORS];
  unsigned long long* record;
  unsigned long long seq;
  int count;
  int nonfinite;
};

// the descriptors sit in a struct, so the compiler cannot see that their pointers are global: say so, to get global_load_dwordx4
// instead of flat loads
typedef const __attribute__((address_space(1))) u32x4 gu32x4;
typedef const __attribute__((address_space(1))) uint32_t gu32;
typedef const __attribute__((address_space(1))) uint16_t gu16;

// Lane maxima of the magnitude bits.  f32: lo only.  bf16: lo holds the low halves (& 0x7fff), hi the high halves (& 0x7fff0000).
__device__ __forceinline__ void acc_f32(const u32x4 w, uint32_t& lo) {
  lo = max(lo, max(max(w.x & 0x7fffffffu, w.y & 0x7fffffffu), max(w.z & 0x7fffffffu, w.w & 0x7fffffffu)));
}
__device__ __forceinline__ void acc_bf16(const u32x4 w, uint32_t& lo, uint32_t& hi) {
  lo = max(lo, max(max(w.x & 0x7fffu, w.y & 0x7fffu), max(w.z & 0x7fffu, w.w & 0x7fffu)));
  hi = max(hi, max(max(w.x & 0x7fff0000u, w.y & 0x7fff0000u), max(w.z & 0x7fff0000u, w.w & 0x7fff0000u)));
}

__global__ __launch_bounds__(256) void anomaly_scan_kernel(const AnomalyArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned long long key = ~0ull;
  for (int s = 0; s < a.count; ++s) {
    const AnomalyTensorArg t = a.t[s];
    const uintptr_t addr = (uintptr_t)t.p;
    const int esz = t.dtype == 0 ? 4 : 2;
    const int epv = 16 / esz;                                           // elements per 16-byte vector
    int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / esz);           // elements before the first 16-byte boundary
    if (head > t.n) head = t.n;
    const int64_t nv = (t.n - head) / epv;
    const int64_t tail0 = head + nv * epv;
    gu32x4* v = (gu32x4*)(addr + head * esz);
    uint32_t lo = 0, hi = 0;
    if (t.dtype == 0) {
      int64_t i = tid;
      for (; i + 3 * stride < nv; i += 4 * stride) {                    // four 16-byte loads in flight per lane
        const u32x4 w0 = v[i], w1 = v[i + stride], w2 = v[i + 2 * stride], w3 = v[i + 3 * stride];
        acc_f32(w0, lo); acc_f32(w1, lo); acc_f32(w2, lo); acc_f32(w3, lo);
      }
      for (; i < nv; i += stride) acc_f32(v[i], lo);
      gu32* e = (gu32*)addr;
      for (int64_t j = tid; j < head + (t.n - tail0); j += stride) lo = max(lo, e[j < head ? j : tail0 + (j - head)] & 0x7fffffffu);
    } else {
      int64_t i = tid;
      for (; i + 3 * stride < nv; i += 4 * stride) {
        const u32x4 w0 = v[i], w1 = v[i + stride], w2 = v[i + 2 * stride], w3 = v[i + 3 * stride];
        acc_bf16(w0, lo, hi); acc_bf16(w1, lo, hi); acc_bf16(w2, lo, hi); acc_bf16(w3, lo, hi);
      }
      for (; i < nv; i += stride) acc_bf16(v[i], lo, hi);
      gu16* e = (gu16*)addr;
      for (int64_t j = tid; j < head + (t.n - tail0); j += stride) lo = max(lo, (uint32_t)(e[j < head ? j : tail0 + (j - head)] & 0x7fffu));
    }
    // f32: lo against 0x7f800000.  bf16: lo against 0x7f80, hi against 0x7f800000 (its low 16 bits are zero).
    const uint32_t lim_lo = t.dtype == 0 ? 0x7f800000u : 0x7f80u;
    const bool bad = a.nonfinite ? (lo >= lim_lo || hi >= 0x7f800000u) : (lo > lim_lo || hi > 0x7f800000u);
    const unsigned long long k = (a.seq << 20) | (unsigned long long)(unsigned)t.index;
    if (bad && k < key) key = k;
  }
  if (__ballot(key != ~0ull)) {         // wave-uniform: only a wave that found something touches the record
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other < key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(a.record, key);
  }
}

__global__ void anomaly_reset_kernel(unsigned long long* record) {
  if (threadIdx.x == 0) *record = 0x7fffffffffffffffull;      // a plain vector store
}

extern "C" {

int odvae_anomaly_scan(const OdvaeAnomalyTensor* tensors, int n, int64_t node_seq, int mode, uint64_t* record, void* stream) {
  ODVAE_CHECK_ARG(record, "anomaly_scan: null record");
  ODVAE_CHECK_ARG(((uintptr_t)record & 7) == 0, "anomaly_scan: misaligned record (8-byte alignment required)");
  ODVAE_CHECK_ARG(tensors, "anomaly_scan: null tensor list");
  ODVAE_CHECK_ARG(n >= 1 && n <= ANOMALY_MAX_TENSORS, "anomaly_scan: %d tensors (1..%d per launch)", n, ANOMALY_MAX_TENSORS);
  ODVAE_CHECK_ARG(node_seq >= 0 && node_seq < (1ll << 43), "anomaly_scan: node_seq %lld out of range [0, 2^43)", (long long)node_seq);
  ODVAE_CHECK_ARG(mode == 0 || mode == 1, "anomaly_scan: mode %d (0 nan, 1 nonfinite)", mode);
  AnomalyArgs a = {};
  int64_t most = 0;
  for (int s = 0; s < n; ++s) {
    const OdvaeAnomalyTensor& t = tensors[s];
    ODVAE_CHECK_ARG(t.numel >= 0, "anomaly_scan: tensor %d has a negative count", s);
    ODVAE_CHECK_ARG(t.dtype == 0 || t.dtype == 1, "anomaly_scan: tensor %d has dtype code %d (0 f32, 1 bf16)", s, t.dtype);
    ODVAE_CHECK_ARG(t.output_index >= 0 && t.output_index < (1 << 20), "anomaly_scan: tensor %d output index %d out of range", s, t.output_index);
    ODVAE_CHECK_ARG(t.numel == 0 || t.ptr, "anomaly_scan: tensor %d is null", s);
    ODVAE_CHECK_ARG(((uintptr_t)t.ptr & (t.dtype == 0 ? 3 : 1)) == 0, "anomaly_scan: tensor %d misaligned for its dtype", s);
    a.t[s].p = t.ptr;
    a.t[s].n = t.numel;
    a.t[s].dtype = t.dtype;
    a.t[s].index = t.output_index;
    most = std::max<int64_t>(most, t.numel / (t.dtype == 0 ? 4 : 8) + 1);
  }
  a.record = reinterpret_cast<unsigned long long*>(record);
  a.seq = (unsigned long long)node_seq;
  a.count = n;
  a.nonfinite = mode;
  // grid-stride; at most 4 blocks of 256 lanes per CU (256 CUs), fewer for small outputs
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(ceil_div64(most, 256), 1), 1024);
  hipLaunchKernelGGL(anomaly_scan_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  ODVAE_LAUNCH_CHECK("anomaly_scan");
  return ODVAE_OK;
}

int odvae_anomaly_reset(uint64_t* record, void* stream) {
  ODVAE_CHECK_ARG(record, "anomaly_reset: null record");
  ODVAE_CHECK_ARG(((uintptr_t)record & 7) == 0, "anomaly_reset: misaligned record (8-byte alignment required)");
  hipLaunchKernelGGL(anomaly_reset_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long*>(record));
  ODVAE_LAUNCH_CHECK("anomaly_reset");
  return ODVAE_OK;
}

}  // extern "C"
