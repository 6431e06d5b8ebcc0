/* libodvae_hip.so -- C ABI of the MI355X (gfx950) kernels behind the OD-VAE autoencoder training step.
 *
 * The reference (tanushreebanerjee/generative-detection) has no FFI of its own: its hot path calls
 * torch ops from Python ([UPSTREAM] ldm/modules/diffusionmodules/model.py through
 * src/modules/autoencodermodules/feat_encoder.py:4, feat_decoder.py:4; src/models/autoencoder.py;
 * src/util/distributions.py; src/modules/losses/contperceptual.py).  Each entry point below names the
 * torch call it stands in for.  The host side binds these with ctypes
 * (generative-detection_amd/lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP global memory) unless it says "host";
 *   - tensors are f32, activations are NHWC ([N][H][W][C], channels contiguous), conv weights OIHW;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only enqueue work, they
 *     never synchronise the device and never allocate;
 *   - scratch comes from the caller: `workspace`/`workspace_bytes`, sized by the *_workspace_bytes query;
 *   - return value: 0 on success, ODVAE_ERR_* otherwise; odvae_last_error() holds the message.
 */
#ifndef ODVAE_HIP_H
#define ODVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODVAE_ABI_VERSION 4            /* odvae_abi_version() of a library built from this header */
#define ODVAE_OK 0
#define ODVAE_ERR_ARG 1
#define ODVAE_ERR_WORKSPACE 2
#define ODVAE_ERR_HIP 3

/* ---- runtime.cpp ------------------------------------------------------------------------------- */
const char* odvae_last_error(void);   /* host string, thread-local */
int odvae_abi_version(void);          /* == ODVAE_ABI_VERSION of this header; bumped whenever the exported surface changes */
const char* odvae_target_arch(void);  /* "gfx950" */

/* ---- gemm_f32.hip: torch.nn.Conv2d(k=1) / torch.bmm ---------------------------------------------
 * C[b] = alpha * op(A[b]) * op(B[b]) (+ bias[col]) (+ residual[b]); row-major;
 * transA=0: A is [M][K]; transA=1: A is stored [K][M]; transB=0: B is [K][N]; transB=1: B is stored [N][K].
 * Stands in for the 1x1 convolutions (nin_shortcut, AttnBlock q/k/v/proj_out, quant_conv_obj/pose,
 * post_quant_conv: src/models/autoencoder.py:88-90,179-180) and AttnBlock's torch.bmm products.
 * Deep plain products -- staging per shape (below), unsplit (odvae_gemm_f32_workspace_bytes == 0), transB = 0, K >= 1024, no bias, no
 * residual: the attention's P V, P^T dO, dS K, dS^T Q at 4 096 tokens from batch 8 up -- do not run on v_mfma_f32_32x32x2_f32: each f32
 * operand is split exactly into three bf16 numbers in the loader and six of the nine cross products are accumulated in f32 on the bf16
 * MFMA (gemm_f32_split.hip).  The result is within 2^-22 of sum_k |a_k| |b_k| of the f32 kernel's (the dropped products), deterministic;
 * an Inf operand yields NaN.  odvae_gemm_select_staging(0 | 1 | 2) forces the f32 MFMA kernel at every shape. */
size_t odvae_gemm_f32_workspace_bytes(int M, int N, int K, int batch);
/* operand staging of the two GEMM entry points: -1 per shape (default: LDS-DMA where A is row-contiguous), 0 through registers,
 * 1 by LDS-DMA (`buffer_load ... lds`, two stages of 32-wide steps), 2 the same with 16-wide steps (four blocks per CU); identical
 * results among 0 / 1 / 2, which always mean the f32 MFMA kernel; -1 also lets deep plain products (above) and the attention's two
 * T x T products (odvae_gemm_exp_bound_f32, odvae_gemm_softmax_bwd[_scaled]_f32) run as bf16 splits; returns the previous setting. */
int odvae_gemm_select_staging(int mode);
/* torch.set_float32_matmul_precision for the bf16-split kernel (gemm_f32_split.hip): how many bf16 planes of each f32 operand it keeps.
 *   0 "highest" (value at library load): hi, mid, lo; six products -- the kernel described above, unchanged to the bit;
 *   1 "high": hi, mid; the products a_mid b_hi, a_hi b_mid, a_hi b_hi -- within 2^-14 of sum_k |a_k| |b_k| of the f32 kernel's result;
 *   2 "medium": hi; the one product a_hi b_hi (bf16 operands, f32 accumulation) -- within 2^-6.
 * Clamps to 0..2, returns the previous setting; process-global, host only.  It applies to EVERY launch of the split kernel: the four
 * odvae_gemm_* entry points that dispatch to it (odvae_gemm_f32, odvae_gemm_rownorm_f32, odvae_gemm_exp_bound_f32,
 * odvae_gemm_softmax_bwd[_scaled]_f32), and with them a 1x1 convolution's weight gradient where odvae_gemm_f32 sends it there (deep K,
 * unsplit: 1 024 pixels; deeper ones run split-K on the f32 kernel) -- which in the reference falls under cuDNN's TF32 allowance
 * (torch.backends.cudnn.allow_tf32, on by default), not under this setting.  The dispatch does not
 * move with the level: a shape that runs on the f32 MFMA kernel does so at every level, and a forced staging mode
 * (odvae_gemm_select_staging(0 | 1 | 2)) still means the f32 MFMA kernel.  The row sums of odvae_gemm_rownorm_f32 come from the unsplit
 * f32 values at every level.  Non-finite operands never give a finite output: at 0 and 1 an Inf operand yields NaN (x - hi = NaN), at 2
 * Inf times a finite non-zero value is Inf (no subtraction happens) and Inf times zero NaN. */
int odvae_gemm_select_precision(int level);
int odvae_gemm_f32(int transA, int transB, int M, int N, int K, float alpha,
                   const float* A, int lda, int64_t strideA,
                   const float* B, int ldb, int64_t strideB,
                   float* C, int ldc, int64_t strideC,
                   const float* bias, const float* residual, int batch,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- conv3x3_f32.hip: torch.nn.Conv2d(k=3) in ResnetBlock / Downsample / Upsample / conv_in / conv_out
 * Weight packs: reduction axis padded to odvae_conv3x3_pack_reduce_pad(), output axis to
 * odvae_conv3x3_pack_out_pad(); a pack has odvae_conv3x3_pack_floats(c_reduce, c_out) floats.
 * odvae_conv3x3_pack_f32 turns OIHW into the forward pack (reduce=Cin,out=Cout) and/or the
 * data-gradient pack (reduce=Cout,out=Cin, taps flipped); either output may be NULL. */
int odvae_conv3x3_pack_reduce_pad(int c_reduce);
int odvae_conv3x3_pack_out_pad(int c_out);
size_t odvae_conv3x3_pack_floats(int c_reduce, int c_out);
int odvae_conv3x3_pack_f32(const float* w_oihw, int Cout, int Cin, float* fwd_pack, float* dgrad_pack, void* stream);
/* 16-tap packs of an Upsample conv (modes 5 / 6): odvae_conv3x3_up_pack_floats(c_reduce, c_out) floats each */
size_t odvae_conv3x3_up_pack_floats(int c_reduce, int c_out);
int odvae_conv3x3_pack_up_f32(const float* w_oihw, int Cout, int Cin, float* fwd16, float* dgrad16, void* stream);
/* mode 0: stride 1 pad 1 (ResnetBlock.conv1/conv2, conv_in, conv_out)
 * mode 1: F.pad(x,(0,1,0,1)) + stride 2 pad 0 (Downsample.forward)      Ho = Hi/2
 * mode 2: F.interpolate(scale 2, nearest) + stride 1 pad 1 (Upsample)   Ho = 2*Hi
 * mode 3: data gradient of mode 1 (x = dy, y = dx, wpk = dgrad pack)    Ho = 2*Hi
 * mode 5: mode 2 evaluated per output parity class on the low-res input with the taps that hit the same input pixel
 *         pre-summed (wpk = fwd16 of odvae_conv3x3_pack_up_f32; 16 instead of 36 tap-products per input pixel)  Ho = 2*Hi
 * mode 6: data gradient of mode 2 / 5 = 4x4-tap stride-2 pad-1 conv over dy (x = dy, y = dx, wpk = dgrad16)   Ho = Hi/2
 * The data gradient of mode 0 is mode 0 with the dgrad pack. */
int odvae_conv3x3_f32(int mode, const float* x, int N, int Hi, int Wi, int Cin,
                      const float* wpk, int Cout, const float* bias, const float* residual,
                      float* y, int Ho, int Wo, int act /* 0 none, 1 ReLU */, void* stream);

/* ---- conv3x3_wino_f32.hip: the stride-1 pad-1 3x3 convolution (mode 0 above and its data gradient) by Winograd
 * F(2x2, 3x3) with fused input / output transforms: f32 throughout, 2.25x fewer multiply-adds, summation order differs
 * from the direct form (~1e-6 relative).  Packs: U = G g G^T per (ci, co), [16][reduce_pad/4][out_pad][4] floats;
 * fwd_pack (reduce = Cin) and/or dgrad_pack (reduce = Cout, taps flipped), either may be NULL.  Needs even H, W and
 * Cin % 4 == 0. */
int odvae_conv3x3_wino_reduce_pad(int c_reduce);
int odvae_conv3x3_wino_out_pad(int c_out);
size_t odvae_conv3x3_wino_pack_floats(int c_reduce, int c_out);
int odvae_conv3x3_pack_wino_f32(const float* w_oihw, int Cout, int Cin, float* fwd_pack, float* dgrad_pack, void* stream);
int odvae_conv3x3_wino_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout,
                           const float* bias, const float* residual, float* y, int act /* 0 none, 1 ReLU */, void* stream);

/* ---- conv3x3_wino4_f32.hip: the same convolution by Winograd F(4x4, 3x3): 4x fewer multiply-adds than the direct form
 * (1.78x fewer than F(2x2)), f32 throughout; the wider interpolation points cost accuracy (max deviation from an f64 direct
 * convolution ~4e-6 of max|y| at Cin = 128, F(2x2) / direct f32: 2e-7).  Packs: [36][reduce_pad/4][out_pad][4] floats.
 * Needs H, W in multiples of 4 and Cin % 8 == 0; `supported` names the shapes the step routes here (forward and data
 * gradient both qualify). */
int odvae_conv3x3_wino4_reduce_pad(int c_reduce);
int odvae_conv3x3_wino4_out_pad(int c_out);
size_t odvae_conv3x3_wino4_pack_floats(int c_reduce, int c_out);
int odvae_conv3x3_wino4_supported(int H, int W, int Cin, int Cout);
int odvae_conv3x3_pack_wino4_f32(const float* w_oihw, int Cout, int Cin, float* fwd_pack, float* dgrad_pack, void* stream);
/* Batched packs: ONE launch for n weights (a training step repacks every conv weight after each optimizer step).  items = device array of
 * n records {const float* w; void* fwd_pack; void* dgrad_pack; int Cout, Cin, taps, reserved;} (40 bytes, natural alignment; either pack
 * may be NULL), channel counts that need no padding (c == *_reduce_pad(c) == *_out_pad(c)).  (The bf16 packs stay per weight: batching them
 * was measured slower -- a pack made right before its conv is still in L2 when the conv reads it.) */
int odvae_conv3x3_pack_wino_batch(const void* items, int n, void* stream);
int odvae_conv3x3_pack_wino4_batch(const void* items, int n, void* stream);

int odvae_conv3x3_wino4_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout,
                            const float* bias, const float* residual, float* y, int act /* must be 0: no fused activation */, void* stream);
/* The same, and the output transform also leaves the GroupNorm statistics of y for the layer that reads it (GroupNorm row:
 * "statistics from the producing conv's epilogue"): gn_partial [N][odvae_conv3x3_wino4_stats_chunks(H, W)][gn_groups][2] = (sum, sum of
 * squares) of y per output tile and channel group, every slot written by exactly one block (deterministic).  Cout / gn_groups must be a
 * power of two <= 32.  Feed it to odvae_groupnorm_fwd_partials_f32. */
int odvae_conv3x3_wino4_stats_chunks(int H, int W);
int odvae_conv3x3_wino4_stats_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout,
                                  const float* bias, const float* residual, float* y, float* gn_partial, int gn_groups, void* stream);
/* The Upsample conv (nearest 2x, then 3x3 stride 1 pad 1) on the same kernel: x [N][H/2][W/2][Cin] low resolution, y [N][H][W][Cout];
 * upk = the forward pack of odvae_conv3x3_pack_wino4_f32; gn_partial / gn_groups as above or NULL / 0.  Shapes:
 * odvae_conv3x3_wino4_supported(H, W, Cin, Cout) on the OUTPUT size. */
int odvae_conv3x3_wino4_up_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout, const float* bias,
                               const float* residual, float* y, float* gn_partial, int gn_groups, void* stream);
/* Data gradient of the Upsample conv w.r.t. its LOW-resolution input ([UPSTREAM] Upsample.forward: interpolate(2x, nearest), conv): x = the
 * conv's dy [N][H][W][Cin], upk = its data-gradient pack, y [N][H/2][W/2][Cout] = the 2x2 sums of the full-resolution gradient, formed in the
 * output transform (that gradient is never stored; odvae_upsample2x_bwd_f32 is not needed behind it). */
int odvae_conv3x3_wino4_pool_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout, float* y, void* stream);
/* Data gradient of a conv whose INPUT was a = swish(GroupNorm(gn_x)) ([UPSTREAM] ResnetBlock: `h = conv(nonlinearity(norm(h)))`), and the
 * first pass of that GroupNorm's backward out of the same output transform: x = the conv's dy [N][H][W][Cin], upk = its data-gradient
 * pack, y = da [N][H][W][Cout]; gn_partial [N][odvae_conv3x3_wino4_stats_chunks(H, W)][2][Cout] = per output tile and channel
 * (sum du * xhat, sum du), du = da * swish'(xhat * gamma + beta) -- every slot written by exactly one block.  Feed it to
 * odvae_groupnorm_bwd_partials_f32: da and gn_x are then not streamed a second time for the sums. */
int odvae_conv3x3_wino4_gnbwd_f32(const float* x, int N, int H, int W, int Cin, const float* upk, int Cout, float* y,
                                  const float* gn_x, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta,
                                  int gn_groups, float* gn_partial, void* stream);

/* ---- conv3x3_wgrad_f32.hip: weight/bias gradient autograd computes for those convolutions (modes 0-2; mode 5 =
 * mode 2 accumulated per output parity class, 16 instead of 36 tap-products per input pixel, same dw)
 * dw is OIHW [Cout][Cin][3][3], overwritten; dbias [Cout] or NULL. */
size_t odvae_conv3x3_wgrad_workspace_bytes(int mode, int N, int Ho, int Wo, int Cin, int Cout);
int odvae_conv3x3_wgrad_f32(int mode, const float* x, const float* dy, int N, int Hi, int Wi, int Cin,
                            int Ho, int Wo, int Cout, float* dw, float* dbias,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Which kernel that call gets and how its pixels are split over blocks: host only, needs no device, launches nothing.  Hi, Wi are the
 * INPUT's.  out = {kind, ntiles, nsplit, tiles_per_split, ci_tiles, co_tiles, tile_rows, effective_mode}: kind 0 thin (conv_in /
 * conv_out), 1 v1, 2 v2 (LDS-DMA), 3 up (parity classes); tiles are tile_rows x 16 output pixels (kind 3: low-resolution pixels), split
 * s owns tiles [s * tiles_per_split, min(ntiles, (s + 1) * tiles_per_split)); effective_mode is 2 where mode 5 falls back to the dense
 * form.  kind 0: {0, blocks per channel group, waves (= partial slabs), channel groups of 128, 0, 0, 1, 0}; wave w owns image rows w,
 * w + waves, ... of the N * Hi rows. */
int odvae_conv3x3_wgrad_plan(int mode, int N, int Hi, int Wi, int Cin, int Cout, int out[8]);
/* How odvae_conv3x3_wgrad_f32 forms a pixel tile's products: -1 by a shape rule (default), 0 the f32 MFMA kernels everywhere, 1 the
 * bf16-split form (each f32 value of x and dy split exactly into three bf16, six products on v_mfma_f32_32x32x16_bf16, f32
 * accumulation) wherever ..._split_supported() == 1: the parity-class kernel (kind 3) and the LDS-DMA kernel in mode 1 (kind 2).  Plan,
 * slabs, reduction and workspace are the same under every setting, dbias is the same bits; dw of the split form is within 2^-22 of
 * sum |x| |dy| of the f32 kernels' error.  The rule admits what was measured faster (profiles/wgrad_direct_split.md): at least 16 tiles per
 * block, 128 or more channels on both sides, whole channel tiles.  Returns the previous setting.  ..._split_supported is host only and
 * launches nothing. */
int odvae_conv3x3_wgrad_select(int form);
int odvae_conv3x3_wgrad_split_supported(int mode, int N, int Hi, int Wi, int Cin, int Cout);

/* ---- conv3x3_wgrad_wino_f32.hip: the same weight/bias gradient for mode 0 (stride 1, pad 1) in the Winograd
 * F(2x2,3x3) domain: dU[xi] = sum over 2x2 tiles of (B^T d B)[xi]^T (A dY A^T)[xi], dw = G^T dU G -- 16 instead of 36
 * multiply-adds per tile.  Serves even H, W, channel counts in multiples of 128 and tensors below 4 GiB
 * (..._supported() == 1); everything else stays on odvae_conv3x3_wgrad_f32.  dw OIHW overwritten; dbias [Cout] or NULL.
 * Replaces autograd's weight gradient of F.conv2d(x, w, b, stride=1, padding=1) ([UPSTREAM] ldm ResnetBlock.conv1/conv2,
 * Encoder/Decoder convs; reference call sites src/modules/autoencodermodules/feat_encoder.py:2, feat_decoder.py:2). */
int odvae_conv3x3_wgrad_wino_supported(int N, int H, int W, int Cin, int Cout);
size_t odvae_conv3x3_wgrad_wino_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int odvae_conv3x3_wgrad_wino_f32(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout,
                                 float* dw, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
/* The main loop of odvae_conv3x3_wgrad_wino_f32: -1 by the shape rule (default), 0 the f32 MFMA loop at every shape, 1 the bf16-split
 * loop (each transformed f32 value split exactly into three bf16, six products on v_mfma_f32_32x32x16_bf16, f32 accumulation) wherever
 * it supports the shape (W / 2 a multiple of 16, tensors below 2 GiB; the f32 loop elsewhere).  Returns the previous setting.  dbias is
 * the same bits under every setting; dw of the split loop is closer to the exact sum than the f32 loop's. */
int odvae_conv3x3_wgrad_wino_select(int form);

/* ---- groupnorm.hip: Normalize = GroupNorm(32, C, eps=1e-6) followed by x*sigmoid(x) -----------------
 * x,y: [N][HW][C]; mean,rstd: [N][G]; swish: 0 identity, 1 x*sigmoid(x).
 * Shapes every f32 entry point of this section takes (ODVAE_ERR_ARG otherwise, nothing written): C % 4 == 0, C <= 1024, G <= 256,
 * G divides C, N <= 65535 (and HW * C / 4 < 2^31); the dropout forms also need C % 8 == 0.  x, y, dy, dx, dx_add, gamma and beta
 * 16-byte aligned.  tests/test_groupnorm_edges_gpu.py holds both ends of each limit. */
size_t odvae_groupnorm_workspace_bytes(int N, int HW, int C, int G);
int odvae_groupnorm_fwd_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                            float eps, int swish, float* y, float* mean, float* rstd,
                            void* workspace, size_t workspace_bytes, void* stream);
/* the same without the statistics pass: partial [N][chunks][G][2] = (sum, sum of squares) of x per chunk and channel group, as the kernel
 * that produced x left them (odvae_conv3x3_wino4_stats_f32); finalize (f64, fixed order) + apply, x read once */
int odvae_groupnorm_fwd_partials_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                     float eps, int swish, float* y, float* mean, float* rstd,
                                     const float* partial, int chunks, void* stream);
/* the apply pass alone from a forward call's mean / rstd: y = act(GroupNorm(x)) re-made from x (the recompute of the "norm" checkpoint policy:
 * the conv that consumed y keeps (x, mean, rstd) instead of y); odvae_groupnorm_apply_bf16 is its bf16 twin */
int odvae_groupnorm_apply_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                              const float* mean, const float* rstd, int swish, float* y, void* stream);
int odvae_groupnorm_apply_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                               const float* mean, const float* rstd, int swish, void* y, void* stream);
int odvae_groupnorm_bwd_f32(const float* x, const float* dy, int N, int HW, int C, int G,
                            const float* gamma, const float* beta, const float* mean, const float* rstd, int swish,
                            float* dx, float* dgamma, float* dbeta, const float* dx_add,
                            void* workspace, size_t workspace_bytes, void* stream);
/* the same with the sums of the first pass given: partial [N][chunks][2][C] as odvae_conv3x3_wino4_gnbwd_f32 leaves it; finalize (f64,
 * fixed order) + apply.  workspace: (N * 2 * C + N * G * 2) floats (odvae_groupnorm_workspace_bytes covers it). */
int odvae_groupnorm_bwd_partials_f32(const float* x, const float* dy, int N, int HW, int C, int G,
                                     const float* gamma, const float* beta, const float* mean, const float* rstd, int swish,
                                     float* dx, float* dgamma, float* dbeta, const float* dx_add, const float* partial, int chunks,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* ---- ResnetBlock dropout inside GroupNorm (+ swish): y = keep * scale * act(GroupNorm(x)), ddconfig.dropout of the reference's yaml
 * ([UPSTREAM] model.py ResnetBlock: conv2(dropout(nonlinearity(norm2(h))))).  The mask is a pure function of (seed, element index, p),
 * re-made inside every kernel -- no mask tensor, nothing but (p, seed) to keep for the backward (csrc/dropout_mask.h; the package's
 * dropout_mask.py restates it in numpy, bit for bit):
 *   one Philox4x32-10 call (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85) per 8 consecutive channels of
 *   a pixel: octet g = ((n * HW + px) * C + c) / 8 (64-bit), counter = (lo32(g), hi32(g), 0, 0), key = (lo32(seed), hi32(seed)); the four
 *   output words are eight 16-bit lanes, channel 8g + 2j the low half of word j and channel 8g + 2j + 1 the high half; an element is
 *   dropped iff lane < thr = round-half-even(p * 65536) (so p = 1 drops everything); kept elements are multiplied by
 *   scale = (float)(1 / (1 - p)), 0 at p = 1.
 * Needs 0 <= p <= 1 and C % 8 == 0 (ODVAE_ERR_ARG otherwise); every other argument as in the plain form of the same name.  The statistics
 * (mean, rstd, the conv epilogue's partials) are those of x: they come before the dropout.  The backward forms dy_eff = dy * keep * scale and
 * runs the reduce + apply kernels on it (never the read-once kernel; there is no bwd_partials form: the sums of
 * odvae_conv3x3_wino4_gnbwd_f32 know nothing of the mask). */
int odvae_groupnorm_fwd_drop_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                 float eps, int swish, double p, unsigned long long seed, float* y, float* mean, float* rstd,
                                 void* workspace, size_t workspace_bytes, void* stream);
int odvae_groupnorm_fwd_partials_drop_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                          float eps, int swish, double p, unsigned long long seed, float* y, float* mean, float* rstd,
                                          const float* partial, int chunks, void* stream);
int odvae_groupnorm_apply_drop_f32(const float* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                   const float* mean, const float* rstd, int swish, double p, unsigned long long seed, float* y, void* stream);
int odvae_groupnorm_bwd_drop_f32(const float* x, const float* dy, int N, int HW, int C, int G,
                                 const float* gamma, const float* beta, const float* mean, const float* rstd, int swish,
                                 double p, unsigned long long seed, float* dx, float* dgamma, float* dbeta, const float* dx_add,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* backward form of odvae_groupnorm_bwd_f32: -1 (default) the read-once kernel where ONE block holds a (sample, 32-channel slab) in its
 * registers (HW <= 256; C % 32 == 0, whole groups per slab), reduce + apply (x and dy read twice) elsewhere; 0 always reduce + apply;
 * 1 the read-once kernel on every shape it takes (teams of ceil(HW / 256) resident blocks that meet at a per-item barrier in L2 --
 * measured slower than the two-kernel form on this chip for HW >= 1024, kept for A/B) or ODVAE_ERR_ARG.  Returns the previous setting. */
int odvae_groupnorm_select_backward(int mode);
/* team-barrier waits of the read-once kernels that gave up (0.2 s) since the library was loaded; synchronises the device.  Must be 0. */
int odvae_groupnorm_fused_timeouts(void);
/* both device-side health counters (synchronises the device; call where the host waits anyway: validation, checkpoint, end of fit):
 * *gn_timeouts != 0 -> a GroupNorm backward's team barrier gave up and its gradients are WRONG (stop the run); *attn_fallbacks = exact-softmax
 * fallbacks of the folded attention softmax taken so far (correct results, three extra passes each).  inject_* > 0: test hooks that bump the
 * counters first (inject_gn_timeouts < 0 clears that counter).  Mirrors nothing in the reference (its torch ops cannot fail this way); generative-detection_amd/trainer.py reads it. */
int odvae_device_health(int* gn_timeouts, int* attn_fallbacks, int inject_gn_timeouts, int inject_attn_fallbacks);
int odvae_attn_softmax_fallbacks(int add);
/* (sample, group) statistics that the finalize step of a GroupNorm forward (f32 or bf16, own statistics pass or a conv's epilogue sums) took
 * from centred sums since the library was loaded, because |mean| / std of the group exceeded 8 and E[x^2] - E[x]^2 from f32 sums would
 * have lost the variance: correct results, one more read of that group by one wavefront.  0 in a healthy run; synchronises the device.
 * add > 0: test hook that bumps the counter first.  -1 if the counter cannot be read.  generative-detection_amd/trainer.py reads it beside
 * the two counters above. */
int odvae_groupnorm_recentred(int add);
/* dx_add (nullable, same shape as x): a second gradient reaching x (the ResnetBlock / AttnBlock skip connection,
   [UPSTREAM] model.py `return x + h`), summed into dx in the same pass instead of autograd's separate add kernel */

/* ---- elementwise.hip ------------------------------------------------------------------------------ */
/* torch.nn.functional.softmax(scale * x, dim=-1) over rows (AttnBlock); y may alias x */
int odvae_softmax_rows_f32(const float* x, float* y, int64_t rows, int cols, float scale, void* stream);
int odvae_softmax_rows_bwd_f32(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, void* stream);
/* Attention backward with the softmax backward folded into the product dP = dO V^T ([UPSTREAM] ldm AttnBlock.forward under
 * autograd): rowdot[i] = dO[i] . O[i] (= sum_j P[i][j] dP[i][j]); dS = alpha * P .* (A B^T - rowdot[row]).
 * A [M][K], B [N][K]; P, dS [M][N] (leading dimension ldc, batch stride strideC; dS may alias P); rowdot [batch][M].
 * With staging per shape, ceil(M/128) * ceil(N/128) * batch >= 512 and K >= 64 (the AttnBlocks at 4 096 tokens from batch 1 up) the
 * product A B^T is the f32-accumulated sum of six bf16 products of exactly split operands (gemm_f32_split.hip, as odvae_gemm_f32's deep
 * products): within 2^-22 of sum_k |a_k| |b_k| of the f32 kernel's, rowdot subtracted from the finished sum, deterministic; an Inf in A
 * or B yields NaN.  The same holds for odvae_gemm_softmax_bwd_scaled_f32 and odvae_gemm_exp_bound_f32 below.
 * odvae_gemm_select_staging(0 | 1 | 2) forces the f32 MFMA kernel at every shape. */
int odvae_rowdot_f32(const float* a, const float* b, int64_t rows, int cols, float* out, void* stream);
int odvae_gemm_softmax_bwd_f32(int M, int N, int K, float alpha, const float* A, int lda, int64_t strideA,
                               const float* B, int ldb, int64_t strideB, const float* P, const float* rowdot,
                               int64_t strideRow, float* dS, int ldc, int64_t strideC, int batch, void* stream);
/* Attention forward with the row softmax folded into the two products ([UPSTREAM] ldm AttnBlock.forward: bmm -> softmax(dim=2) -> bmm).
 * softmax is invariant to the shift it subtracts, so the QK^T epilogue can write E = exp(scale * (q_i . k_j - bound_i)) against any bound_i >=
 * max_j q_i . k_j -- |q_i| * max_j |k_j| -- instead of waiting for the row maximum, and the PV product sums l_i = sum_j E_ij beside its
 * multiplies and divides by it: P = E / l is never formed, the T x T tensor is written once and read once (the separate softmax pass read and
 * rewrote it: 3.9 of 232 ms per step).  A bound far above the maximum underflows a whole row; odvae_gemm_rownorm_f32 then raises *flag and
 * the caller's PREDICATED fallback launches (odvae_gemm_pred_f32, odvae_softmax_rows_pred_f32: no-ops unless *flag != 0) redo the block with
 * the row maximum -- no host synchronisation either way.
 *   odvae_attn_row_bound_f32: qkv [N][T][3C] (q | k | v per token) -> bound [N*T] (unscaled), *flag = 0; nk_scratch [N*T]
 *   odvae_gemm_exp_bound_f32: E = exp(alpha * (A B^T - rowbound[row])); A [M][K], B [N][K]; above the gate of odvae_gemm_softmax_bwd_f32
 *                             A B^T comes from the bf16-split kernel (E moves by at most E * alpha * 2^-22 sum_k |a_k| |b_k|; Inf gives NaN)
 *   odvae_gemm_rownorm_f32:   C = (A B) / l[row], l = row sums of A [M][K]; B [K][N]; rinv [batch][M] = 1 / l; *flag |= (some l < 1e-30 or not finite)
 *                             (under odvae_gemm_f32's rule for deep products A B is a sum of six bf16 products of split operands; l is summed from
 *                             the unsplit f32 values and the flag condition is the same)
 *   odvae_gemm_pred_f32:      odvae_gemm_f32 (unsplit shapes, no bias / residual) under the predicate
 *   odvae_softmax_rows_pred_f32: odvae_softmax_rows_f32 under the predicate, and ones[row] = 1
 * Backward with P given as (E, rinv): odvae_rowdot_scale_f32 (out[i] = a_i . b_i, a_scaled[i][:] = a[i][:] * row_scale[i]: D_i and dO_i / l_i),
 * odvae_gemm_softmax_bwd_scaled_f32 (dS = alpha * E .* rinv[row] .* (A B^T - rowdot[row]); the same kernels and gate as
 * odvae_gemm_softmax_bwd_f32). */
int odvae_attn_row_bound_f32(const float* qkv, int N, int T, int C, float* bound, float* nk_scratch, int* flag, void* stream);
int odvae_gemm_exp_bound_f32(int M, int N, int K, float alpha, const float* A, int lda, int64_t strideA, const float* B, int ldb, int64_t strideB,
                             const float* rowbound, int64_t strideRow, float* E, int ldc, int64_t strideC, int batch, void* stream);
int odvae_gemm_rownorm_f32(int M, int N, int K, const float* A, int lda, int64_t strideA, const float* B, int ldb, int64_t strideB,
                           float* C, int ldc, int64_t strideC, float* rinv, int64_t strideRow, int* flag, int batch, void* stream);
int odvae_gemm_pred_f32(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda, int64_t strideA,
                        const float* B, int ldb, int64_t strideB, float* C, int ldc, int64_t strideC, int batch, const int* pred, void* stream);
int odvae_softmax_rows_pred_f32(const float* x, float* y, int64_t rows, int cols, float scale, const int* pred, float* ones, void* stream);
int odvae_rowdot_scale_f32(const float* a, const float* b, const float* row_scale, int64_t rows, int cols, float* out, float* a_scaled, void* stream);
int odvae_gemm_softmax_bwd_scaled_f32(int M, int N, int K, float alpha, const float* A, int lda, int64_t strideA,
                                      const float* B, int ldb, int64_t strideB, const float* E, const float* rowdot, const float* rinv,
                                      int64_t strideRow, float* dS, int ldc, int64_t strideC, int batch, void* stream);
/* backward of F.interpolate(scale_factor=2, mode="nearest"): dx[N][H][W][C] from du[N][2H][2W][C] */
int odvae_upsample2x_bwd_f32(const float* du, float* dx, int N, int H, int W, int C, void* stream);
/* The conv-less resamplers (ddconfig.resamp_with_conv = False), NHWC, C % 4 == 0, C <= 1024, 16-byte aligned operands, no atomics.
 * avgpool2x2: y [N][H/2][W/2][C] = F.avg_pool2d(x [N][H][W][C], 2, 2); an odd last row / column is dropped (H, W >= 2).  Its backward
 * overwrites dx [N][H][W][C] = 0.25 dy broadcast, zeros in a dropped row / column.  upsample2x: u [N][2H][2W][C] =
 * F.interpolate(x [N][H][W][C], scale_factor=2, mode="nearest"); its backward is odvae_upsample2x_bwd_f32.
 * gn_partial (nullable): the same pass leaves the GroupNorm statistics of the RESULT, gn_partial [N][chunks][gn_groups][2] = (sum, sum of
 * squares), every slot written -- the layout odvae_groupnorm_fwd_partials_f32 takes (gn_groups <= 256 divides C).  The kernel cuts the result's
 * pixels into `chunks` runs itself; pass the count the consumer expects (odvae_conv3x3_wino4_stats_chunks of the result's H, W). */
int odvae_avgpool2x2_f32(const float* x, float* y, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream);
int odvae_avgpool2x2_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
int odvae_upsample2x_f32(const float* x, float* u, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream);
/* Decoder(tanh_out=True): y = tanh(x) on a flat f32 array of n elements; dx = dy * (1 - y * y) from the saved y */
int odvae_tanh_f32(const float* x, float* y, int64_t n, void* stream);
int odvae_tanh_bwd_f32(const float* y, const float* dy, float* dx, int64_t n, void* stream);
/* PoseAutoencoder._rescale (src/models/autoencoder.py:434-436): NCHW in, NHWC out; workspace >= 8 KiB */
int odvae_rescale_minmax_f32(const float* x_nchw, float* y_nhwc, int N, int C, int HW, float* minmax_out,
                             void* workspace, size_t workspace_bytes, void* stream);
/* DiagonalGaussianDistribution (src/util/distributions.py:5-41): moments [N][HW][2*Cz] */
int odvae_gaussian_sample_f32(const float* moments, const float* eps, float* z, int N, int HW, int Cz, void* stream);
int odvae_gaussian_kl_f32(const float* moments, float* kl, int N, int HW, int Cz, void* stream);
int odvae_gaussian_bwd_f32(const float* moments, const float* eps, const float* dz, const float* dkl,
                           float* dmoments, int N, int HW, int Cz, void* stream);
/* PoseLoss._get_rec_loss pixel term with mask_2d_bbox applied (contperceptual.py:137,252-255):
 * out[n] = sum |x*m - xr*m|; workspace >= N*1 KiB */
int odvae_l1_masked_sum_f32(const float* x, const float* xr, const float* mask, float* out, int N, int HW, int C,
                            void* workspace, size_t workspace_bytes, void* stream);
int odvae_l1_masked_bwd_f32(const float* x, const float* xr, const float* mask, const float* g, float* dxr,
                            int N, int HW, int C, void* stream);
/* image_mask_key: PoseLoss's terms on a 4-channel reconstruction (contperceptual.py:230-257,166-174) in one pass.  rec [N][HW][4] (16-byte
 * aligned: one load per pixel), rgb_gt [N][HW][3], mask_gt [N][HW], box [N][HW] or NULL (= 1): any 4-byte aligned base.
 * l1_sum[n] = sum over pixels and RGB of |rgb_gt*box - rec*box| (the term of odvae_l1_masked_sum_f32); mask_sum[n] = sum over pixels of
 * |mask_gt*box - rec_3*box| (l2 = 0) or its square (l2 = 1); every product, difference and addition separately rounded.  Each of
 * rec_rgb_m / gt_rgb_m [N][HW][3] and rec_rgba_m / gt_rgba_m [N][HW][4] (16-byte aligned; gt_rgba_m = cat(rgb_gt, mask_gt) * box) is
 * written unless NULL.  The sums go through the workspace (odvae_rgba_terms_workspace_bytes(N) bytes) in a fixed order, no atomics;
 * l1_sum and mask_sum both NULL: the copies alone, no sums, no workspace (the discriminator phase).  N <= 65535.
 * odvae_rgba_terms_bwd_f32: d_rec [N][HW][4] (overwritten) from g_l1[N], g_mask[N], g_rec_rgb_m [N][HW][3], g_rec_rgba_m [N][HW][4], each
 * NULL = zero; the L1 term's sign rule is odvae_l1_masked_bwd_f32's (0 at a tie). */
size_t odvae_rgba_terms_workspace_bytes(int N);
int odvae_rgba_terms_f32(const float* rec, const float* rgb_gt, const float* mask_gt, const float* box, int l2, float* l1_sum, float* mask_sum,
                         float* rec_rgb_m, float* gt_rgb_m, float* rec_rgba_m, float* gt_rgba_m, int N, int HW,
                         void* workspace, size_t workspace_bytes, void* stream);
int odvae_rgba_terms_bwd_f32(const float* rec, const float* rgb_gt, const float* mask_gt, const float* box, int l2, const float* g_l1,
                             const float* g_mask, const float* g_rec_rgb_m, const float* g_rec_rgba_m, float* d_rec, int N, int HW, void* stream);
/* The losses' `weights` argument as a weight map (contperceptual.py:147-158: weights * nll_loss on [N,C,H,W]): three per-sample sums from
 * one pass.  x [N][HW][C]; xr [N][HW][Cr], Cr >= C, only its first C channels are read (a 4-channel reconstruction in place: C 3, Cr 4);
 * box [N][HW] or NULL (= 1); wgt [N][HW] (wgt_per_channel 0) or [N][HW][C] (1).  Any 4-byte aligned bases; a 16-byte aligned xr with
 * Cr == 4 is read with one load per pixel.  Per element, every operation separately rounded: xm = x*box, rm = xr*box, t = |xm - rm|,
 * l1_sum[n] += t, wl1_sum[n] += wgt*t, w_sum[n] += wgt (a per-pixel weight counts once per channel; w_sum is not box-masked).  Each output
 * is skipped when NULL; all three NULL is an error.  x and xr both NULL: w_sum alone may be asked for.  The sums go through the workspace
 * (odvae_l1_weighted_workspace_bytes(N) bytes) in a fixed order, no atomics.  N <= 65535.
 * odvae_l1_weighted_bwd_f32: dxr [N][HW][Cr], overwritten: ((g_l1[n] + g_wl1[n]*wgt) * sign(rm - xm)) * box for c < C (0 at a tie, as
 * odvae_l1_masked_bwd_f32; a NULL gradient counts as zero), 0 for the channels C .. Cr-1. */
size_t odvae_l1_weighted_workspace_bytes(int N);
int odvae_l1_weighted_sums_f32(const float* x, const float* xr, const float* box, const float* wgt, int wgt_per_channel, float* l1_sum,
                               float* wl1_sum, float* w_sum, int N, int HW, int C, int Cr, void* workspace, size_t workspace_bytes,
                               void* stream);
int odvae_l1_weighted_bwd_f32(const float* x, const float* xr, const float* box, const float* wgt, int wgt_per_channel, const float* g_l1,
                              const float* g_wl1, float* dxr, int N, int HW, int C, int Cr, void* stream);
/* disc_conditional: the discriminator's input torch.cat((x * mask_2d_bbox, cond), dim=1) (contperceptual.py:283-289,354-361) in one pass.
 * x [N][HW][Cx], box [N][HW] or NULL (= 1), cond [N][HW][Cc], y [N][HW][Cx+Cc]; cond is copied, never multiplied by box.  Any 4-byte
 * aligned bases (a 16-byte aligned y with Cx + Cc == 4 is written with one store per pixel); N <= 65535, HW * (Cx + Cc) < 2^31.
 * odvae_cat_mask_bwd_f32: dx [N][HW][Cx] = dy[..., :Cx] * box, dy [N][HW][Cx+Cc]. */
int odvae_cat_mask_f32(const float* x, const float* box, const float* cond, float* y, int N, int HW, int Cx, int Cc, void* stream);
int odvae_cat_mask_bwd_f32(const float* dy, const float* box, float* dx, int N, int HW, int Cx, int Cc, void* stream);
/* bias gradient of a 1x1 convolution: out[c] = sum_rows x[row][c] */
size_t odvae_colsum_workspace_bytes(int64_t rows, int C);
int odvae_colsum_f32(const float* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* torch.nn.utils.clip_grad_norm_ over one flat arena: out[0] = norm, out[1] = clip coefficient; workspace >= 4 KiB */
int odvae_grad_norm_f32(const float* g, int64_t n, float max_norm, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* torch.optim.Adam step (src/models/autoencoder.py:365-377) over flat arenas; clip = odvae_grad_norm_f32 output or NULL */
int odvae_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, int step, const float* clip, void* stream);
/* The same step with gr = clamp(g, -clamp, +clamp) in place of g * coefficient (lightning.trainer.gradient_clip_algorithm: value;
 * torch.nn.utils.clip_grad_value_ folded into the step, g itself is not rewritten).  torch.clamp's rules: NaN stays NaN, +-inf becomes
 * +-clamp, -0.0 stays -0.0.  clamp is a host float > 0 (anything else, NaN included, is refused). */
int odvae_adam_step_clamp_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, int step, float clamp, void* stream);
/* Segmented p-norms of one flat f32 arena (lightning.trainer.track_grad_norm): out[i] = the norm of g[off[i] .. off[i] + len[i]) for
 * i < n_seg, out[n_seg] = the same kind of norm of the f32 values out[i] of the segments with counts[i] != 0 (counts NULL: all of them;
 * none: 0) -- what torch.tensor([p.grad.norm(k) ...]).norm(k) computes.  kind: ODVAE_NORM_MAX ('inf': the largest |g|, a NaN propagates
 * as in torch.norm), ODVAE_NORM_L1, ODVAE_NORM_L2, ODVAE_NORM_P (the general kind, p finite and > 0; p is ignored by the others).
 * Every sum is taken in f64 ((double)g products, pow in f64), in an order fixed by the segments alone: no atomics, the same bits on any
 * launch grid; a segment's norm is (float)S, (float)sqrt(S) or (float)pow(S, 1 / p), the total is summed in f64 again and rounded once.
 * off / len / counts are host arrays (floats; len >= 1, off a multiple of 4 floats, off + len <= n); nothing outside a segment is read,
 * nothing but out[0 .. n_seg] is written.  The tables travel in the kernel arguments: no copy, no allocation, no host wait;
 * ceil(n_seg / K) + 2 launches, K = odvae_grad_seg_norms_segments_per_launch() (one block per 4096-float chunk of a segment, one
 * wavefront per segment, one block for the total).  workspace: 16-byte aligned, odvae_grad_seg_norms_workspace_bytes(len, n_seg) bytes
 * (0 for lengths the call refuses).  A refused call launches nothing. */
#define ODVAE_NORM_MAX 0
#define ODVAE_NORM_L1 1
#define ODVAE_NORM_L2 2
#define ODVAE_NORM_P 3
int odvae_grad_seg_norms_segments_per_launch(void);
size_t odvae_grad_seg_norms_workspace_bytes(const int64_t* len, int n_seg);
int odvae_grad_seg_norms_f32(const float* g, int64_t n, const int64_t* off, const int64_t* len, const unsigned char* counts, int n_seg,
                             int kind, double p, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Gradient accumulation (lightning.trainer.accumulate_grad_batches): arena[dst_off[i] + j] += src[i][j], j < numel[i], for `count` disjoint
 * segments in ceil(count / K) launches, K = odvae_grad_accumulate_segments_per_launch().  dst_off / numel are host arrays, src a host array
 * of device pointers; the table travels in the kernel arguments (no copy, no allocation, no host wait).  One f32 rounding per element, no
 * atomics; NaN / Inf propagate.  Every segment is validated before the first launch; count == 0 is a no-op. */
int odvae_grad_accumulate_segments_per_launch(void);
int odvae_grad_accumulate_f32(float* arena, int64_t arena_numel, const int64_t* dst_off, const float* const* src, const int64_t* numel,
                              int count, void* stream);
/* Exponential moving average of the weights (model.params.ema_decay; [UPSTREAM] ldm.modules.ema.LitEma), all on the device.
 * odvae_ema_tick: one thread.  num_updates >= 0: num_updates += 1, q = float(1 + num_updates) / float(10 + num_updates) (one correctly
 * rounded f32 division), d = q < decay ? q : decay; num_updates < 0: d = decay.  state[0] = 1 - d, state[1] = d.  Nothing is read back.
 * odvae_ema_update_f32: shadow[i] <- shadow[i] - omd[0] * (shadow[i] - p[i]) as three separately rounded f32 operations (no fused
 * multiply-add); omd = the state the tick wrote.  odvae_ema_swap_f32: a[i] <-> b[i] in one pass.  Both walk any 4-byte aligned pair of
 * disjoint arrays: 16-byte accesses where the two pointers share their alignment (scalar head and tail), scalar otherwise.  NaN / Inf propagate. */
int odvae_ema_tick(const float* decay, int* num_updates, float* state, void* stream);
int odvae_ema_update_f32(const float* p, float* shadow, int64_t n, const float* omd, void* stream);
int odvae_ema_swap_f32(float* a, float* b, int64_t n, void* stream);
int odvae_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int HW, void* stream);
/* y = x * mask[n][hw] broadcast over channels (inputs*mask_2d_bbox, contperceptual.py:252-255); x,y [npix][C] */
int odvae_mul_mask_f32(const float* x, const float* mask, float* y, int64_t npix, int C, void* stream);
/* out = z*mask + add, mask/add may be NULL (dropout on z_obj, +noise, +enc_pose: src/models/autoencoder.py:233-253) */
int odvae_latent_combine_f32(const float* z, const float* mask, const float* add, float* out, int64_t n, void* stream);

/* ---- latent_noise.hip: the latent stage's draws made on the device (model.params.device_noise; csrc/latent_noise.h defines the draw) ----
 * A draw is a pure function of (seed, step_word, tag, element index): seed = the 64-bit Philox key (the model's seed plus its rank's
 * offset), step_word = lo32(global_step), tag = stream << 29 | training << 28 | call (each a 32-bit word in a uint64_t).
 * odvae_noise_fill_f32: out[e] = element first + e of the stream in `tag`, e in [0, n); kind 0 = standard normal, 1 = dropout multiplier
 * of probability p (0 or f32(1 / (1 - p)); all 0 at p = 1).  first < 2^62 and need not be a multiple of 4.
 * odvae_latent_stage_f32: z = ((mean + std * eps) * m + noise) + add on NHWC moments [N][HW][2*Cz] (logvar clamped to [-30, 20]), add
 * (may be NULL) and z [N][HW][Cz]; eps, m, noise are streams 0, 1, 2 of `tag` (whose stream bits must be 0), element = flat index of z.
 * flags: 1 = sample (else mode: z0 = mean), 2 = dropout on, 4 = noise on.  Bit for bit the chain odvae_gaussian_sample_f32 ->
 * odvae_latent_combine_f32 (mask) -> (add = noise) -> (add) fed odvae_noise_fill_f32's tensors for the same words.
 * odvae_latent_stage_bwd_f32: dmoments from moments and dz alone (eps and m are drawn again); the gradient of add is dz itself. */
int odvae_noise_fill_f32(float* out, int64_t n, uint64_t first, uint64_t seed, uint64_t step_word, uint64_t tag, int kind, double p,
                         void* stream);
int odvae_latent_stage_f32(const float* moments, const float* add, float* z, int N, int HW, int Cz, uint64_t seed, uint64_t step_word,
                           uint64_t tag, int flags, double p, void* stream);
int odvae_latent_stage_bwd_f32(const float* moments, const float* dz, float* dmoments, int N, int HW, int Cz, uint64_t seed,
                               uint64_t step_word, uint64_t tag, int flags, double p, void* stream);

/* ---- gan_f32.hip, gan_norm.hip: PatchGAN NLayerDiscriminator ([UPSTREAM] taming discriminator; contperceptual.py:285,355-356) ----
 * gan_f32.hip: the convolution pieces, LeakyReLU, the logit terms; gan_norm.hip: BatchNorm2d / ActNorm + LeakyReLU (f32 here, bf16 below).
 * Conv2d(k=4, pad=1, stride 1|2) = im2col + odvae_gemm_f32 against the weight reordered to [Cout][(kh,kw,ci)];
 * cols is [N*Ho*Wo][16*C]; col2im is its adjoint (data gradient). */
int odvae_im2col4x4_f32(const float* x, float* cols, int N, int Hi, int Wi, int C, int Ho, int Wo, int stride, void* stream);
int odvae_col2im4x4_f32(const float* dcols, float* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, int stride, void* stream);
int odvae_weight4x4_reorder_f32(const float* src, float* dst, int Cout, int Cin, int to_gemm, void* stream);
/* ---- conv3x3_f32.hip, conv4x4_wgrad_f32.hip: the same Conv2d(k=4, pad=1, stride 1|2) as an implicit GEMM, exact f32, no cols matrix
 * (opt-in: ODVAE_DISC_F32_IMPLICIT=1).  NHWC; Ho = (Hi - 2) / stride + 1, Hi and Wi may be odd.  Packs are [16][reduce_pad/4][out_pad][4]
 * with the pads of odvae_conv3x3_pack_reduce_pad / _out_pad; the data-gradient pack (flipped taps, channel roles swapped; stride 2:
 * ordered by output parity class) depends on the stride.
 * odvae_conv4x4_f32, dgrad = 0: y = conv(x) + bias, wpk = forward pack.  dgrad = 1: x = dy [N][Hi][Wi][Cin = the layer's output
 * channels], y = dx [N][Ho][Wo][Cout = the layer's input channels], Hi = (Ho - 2) / stride + 1, wpk = data-gradient pack, bias null.
 * odvae_conv4x4_wgrad_f32: dw OIHW [Cout][Cin][4][4] and dbias [Cout] (or null), partial sums reduced in a fixed order (deterministic);
 * odvae_conv4x4_wgrad_plan (host only): out = {kind (1), ntiles, nsplit, tiles_per_split, ci_tiles, co_tiles, tile_rows, stride}. */
int odvae_conv4x4_f32_supported(int stride, int N, int Hi, int Wi, int Cin, int Cout);
size_t odvae_conv4x4_pack_floats(int c_reduce, int c_out);
int odvae_conv4x4_pack_f32(const float* w_oihw, int Cout, int Cin, int stride, float* fwd_pack, float* dgrad_pack, void* stream);
int odvae_conv4x4_f32(int stride, int dgrad, const float* x, int N, int Hi, int Wi, int Cin, const float* wpk, int Cout,
                      const float* bias, float* y, int Ho, int Wo, void* stream);
size_t odvae_conv4x4_wgrad_workspace_bytes(int stride, int N, int Ho, int Wo, int Cin, int Cout);
int odvae_conv4x4_wgrad_f32(int stride, const float* x, const float* dy, int N, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout,
                            float* dw, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int odvae_conv4x4_wgrad_plan(int stride, int N, int Hi, int Wi, int Cin, int Cout, int out[8]);
/* torch.nn.BatchNorm2d (batch statistics when train=1, running-stat update with momentum) + LeakyReLU(slope), x [rows][C] */
size_t odvae_batchnorm_workspace_bytes(int64_t rows, int C);
int odvae_batchnorm_lrelu_fwd_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                                  float momentum, float slope, int train, float* mean, float* rstd,
                                  float* running_mean, float* running_var, float* y,
                                  void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, float slope, int train,
                                  float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* Synchronised BatchNorm + LeakyReLU (torch.nn.SyncBatchNorm = BatchNorm2d on the ranks' rows together): the training forward and
 * backward cut where the ranks exchange a few KB.  The library makes no collective; the caller carries the f64 buffers between ranks.
 *   forward : stats_record (each rank) -> gather -> stats_merge -> odvae_batchnorm_lrelu_fwd_*(train = 0) with the merged mean / rstd
 *   backward: bwd_sums (each rank) -> gather -> bwd_dx
 * record  : double [C][3] = {rows, mean_c, M2_c}, M2 = sum (x - mean_c)^2, from the sums about the pivot x[0][c].
 * records : double [world][C][3], merged pairwise in index order by Chan's update in f64 (the same bits on every rank that holds the same
 *           records) into f32 mean, rstd = 1 / sqrt(M2 / n + eps), and the momentum update of the running estimates with the unbiased
 *           variance over the total count (running_mean = running_var = NULL: none).  One merge serves f32 and bf16 activations.
 * sums    : double [2][C] = (sum g, sum g * xhat), g = dy * lrelu'(u); dbeta, dgamma are the same local sums in f32.
 *           total_rows (one f64 on the device, may be NULL) receives the rows of all ranks.
 * sums_all: double [world][2][C], added in index order in f64; m_total: the rows of all ranks ON THE DEVICE (the merge's total_rows: row
 *           counts may differ per rank, and the total never passes through the host); dx by the unsynchronised backward's expression.
 * A record / sums buffer smaller than odvae_batchnorm_sync_record_bytes(C) / _sums_bytes(C) (times world where all ranks' are read) is
 * ODVAE_ERR_WORKSPACE with the needed size.  Workspace where one is taken: odvae_batchnorm_workspace_bytes(rows, C). */
size_t odvae_batchnorm_sync_record_bytes(int C);
size_t odvae_batchnorm_sync_sums_bytes(int C);
int odvae_batchnorm_sync_stats_record_f32(const float* x, int64_t rows, int C, double* record, size_t record_bytes,
                                          void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_sync_stats_merge(const double* records, size_t records_bytes, int world, int C, float eps, float momentum,
                                     float* mean, float* rstd, float* running_mean, float* running_var, double* total_rows, void* stream);
int odvae_batchnorm_sync_bwd_sums_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                      const float* mean, const float* rstd, float slope, double* sums, size_t sums_bytes,
                                      float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_sync_bwd_dx_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                    const float* mean, const float* rstd, float slope, const double* sums_all, size_t sums_bytes,
                                    int world, const double* m_total, float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* ActNorm ([UPSTREAM] taming ActNorm: h = scale[c] * (x + loc[c])) + LeakyReLU(slope), x [rows][C].
 * init: loc = -mean_c, scale = 1 / (std_c + eps), std_c the unbiased standard deviation over the rows (rows >= 2), written on the device.
 * bwd: dx = scale * g, dloc = scale * sum g, dscale = sum g (x + loc), g = dy * lrelu'(h); dloc = dscale = NULL: dx only, no workspace. */
size_t odvae_actnorm_workspace_bytes(int64_t rows, int C);
int odvae_actnorm_init_f32(const float* x, int64_t rows, int C, float eps, float* loc, float* scale,
                           void* workspace, size_t workspace_bytes, void* stream);
int odvae_actnorm_lrelu_fwd_f32(const float* x, int64_t rows, int C, const float* loc, const float* scale, float slope, float* y, void* stream);
int odvae_actnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* loc, const float* scale, float slope,
                                float* dx, float* dloc, float* dscale, void* workspace, size_t workspace_bytes, void* stream);
/* torch.nn.LeakyReLU(slope); the backward with slope 0 is the ReLU backward */
int odvae_leaky_relu_f32(const float* x, float* y, float slope, int64_t n, void* stream);
int odvae_leaky_relu_bwd_f32(const float* x, const float* dy, float* dx, float slope, int64_t n, void* stream);
/* The scalar terms of the GAN losses over the discriminator's logits ([UPSTREAM] ldm LPIPSWithDiscriminator.forward, taming hinge_d_loss /
 * vanilla_d_loss), one launch pair each way:
 *   out6 = [mean real, mean fake, mean relu(1 - real), mean relu(1 + fake), mean softplus(-real), mean softplus(fake)]  (device, 6 floats)
 * real may be NULL with n_real == 0 (generator phase: its three terms are written as 0); n_real != n_fake is allowed.  softplus(x) =
 * max(x, 0) + log1p(exp(-|x|)); a NaN logit makes its three terms NaN.  Each term is summed in f64 in a fixed order (no atomics: the same
 * bits on every run), divided by n in f64 and rounded to f32 once.  Workspace: odvae_gan_logit_terms_workspace_bytes, 8-byte aligned.
 * bwd: dout6 is the upstream gradient ON THE DEVICE;  dreal_i = (d0 - d2 [real_i < 1] - d4 sigmoid(-real_i)) / n_real,
 *      dfake_i = (d1 + d3 [fake_i > -1] + d5 sigmoid(fake_i)) / n_fake  (strict inequalities: relu'(0) = 0); dreal or dfake may be NULL. */
size_t odvae_gan_logit_terms_workspace_bytes(int64_t n_real, int64_t n_fake);
int odvae_gan_logit_terms_f32(const float* real, int64_t n_real, const float* fake, int64_t n_fake, float* out6,
                              void* workspace, size_t workspace_bytes, void* stream);
int odvae_gan_logit_terms_bwd_f32(const float* real, int64_t n_real, const float* fake, int64_t n_fake, const float* dout6,
                                  float* dreal, float* dfake, void* stream);

/* ---- lpips_f32.hip: LPIPS-style perceptual distance ([UPSTREAM] taming lpips.py; contperceptual.py:143) ------------- */
/* ScalingLayer (x - shift[c]) / scale[c]; backward=1 computes x / scale[c] */
int odvae_scaling_layer_f32(const float* x, const float* shift, const float* scale, float* y, int64_t npix, int C, int backward, void* stream);
/* torch.nn.MaxPool2d(2, 2): x [N][Hi][Wi][C] -> y [N][Ho][Wo][C] with Ho == Hi / 2, Wo == Wi / 2 (floor; checked): an odd last row /
 * column is dropped.  Hi, Wi >= 2; the forward needs C % 4 == 0.  A window that holds a NaN yields NaN.  The backward writes every element
 * of dx (0 on a dropped row / column); dy goes to the window's first maximum in row-major order, in a NaN window to its first NaN. */
int odvae_maxpool2x2_f32(const float* x, float* y, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
int odvae_maxpool2x2_bwd_f32(const float* x, const float* y, const float* dy, float* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
/* out[n] = spatial mean of lin_w . (normalize_tensor(f0) - normalize_tensor(f1))^2 ; gradient w.r.t. f1 only */
int odvae_lpips_distance_f32(const float* f0, const float* f1, const float* w, float* out, int N, int HW, int C,
                             void* workspace, size_t workspace_bytes, void* stream);
int odvae_lpips_distance_bwd_f32(const float* f0, const float* f1, const float* w, const float* g, float* df1,
                                 int N, int HW, int C, void* stream);

/* ---- patch_u8.hip: object-patch extraction (src/data/datasets/nuscenes.py:159-192) ------------ */
/* Replaces img_pil.crop(box) (:159) -> patch.resize((S, S), BILINEAR, reducing_gap=1.0) (:176) -> ToTensor (:190-191) and
   the NEAREST-resized 2-d box mask (:178-192), bit-identical to Pillow's 8-bit fixed-point resampler.
   d_images [B] device pointers to u8 HWC RGB camera images; d_geom [B][8] int32 {img_h, img_w, crop_x1, crop_y1, crop_size,
   table_slot, 0, 0}; d_mask_rect [B][4] int32 {x_start, x_stop, y_start, y_stop} in crop coordinates; d_tables
   [n_slots][S][8] int32 per crop size {k0..k4 (coefficients * 2^22), first source index, taps, nearest source index};
   patch [B][S][S][3] f32 in [0,1], mask [B][S][S] f32 in {0,1}.  odvae_patch_table_ints(S) = ints per table slot. */
int odvae_patch_table_ints(int S);
int odvae_patch_crop_resize_u8(const void* d_images, const void* d_geom, const void* d_mask_rect, const void* d_tables,
                               int n_slots, int B, int S, void* patch, void* mask, void* stream);
/* The same with Pillow's box pre-reduction (`reducing_gap=1.0` on a crop of side >= 2 S) per instance: d_geom[b][6] = reduce
   factor f >= 1 (0 reads as 1).  An instance with f > 1 is box-reduced by f to side r = ceil(crop_size / f) (each byte
   ((sum + n/2) * mult(n)) >> 24 in unsigned 32-bit arithmetic, n = crop pixels in the box) and its table slot then holds the
   BILINEAR windows over the reduced image (source box [0, (float)(crop_size / f)), clipped to [0, r)); the nearest source
   index stays the one of the unreduced walk.  d_mults [n_slots][4] uint32 per slot {mult(f*f), mult(f*rem), mult(rem*rem), 0},
   rem = crop_size - (r - 1) * f the width of the last box, mult(n) = (uint32)(4294967296.0f / (float)(256 * n)), 0 where
   unused.  f = 1 gives the bits of odvae_patch_crop_resize_u8; mixed batches go out in one launch. */
int odvae_patch_reduce_resize_u8(const void* d_images, const void* d_geom, const void* d_mask_rect, const void* d_tables,
                                 const void* d_mults, int n_slots, int B, int S, void* patch, void* mask, void* stream);

/* ---- pose_f32.hip: every pose-head loss term in one launch (src/modules/losses/contperceptual.py:111-132,176-212) ------------- */
/* dec_pose [B][8+NC] (pose 4 | lhw 3 | fill 1 | class logits), moments [B][16] (box posterior mean | raw logvar), prior [L][3][8]
   (mean | var | logvar per label), prior_idx [B] (< 0 = label "background").  out [9] = pose, class, bbox, fill, kl_bbox, mean t1, t2,
   t3, v3; jac_pose [4][B][8+NC] and jac_mom [B][16] = Jacobians of out[0..3] / out[4] for odvae_pose_losses_bwd_f32 */
int odvae_pose_losses_f32(const float* dec_pose, const float* pose_gt, const float* bbox_gt, const float* fill_gt, const int64_t* class_gt,
                          const float* moments, const float* prior, const int* prior_idx, int B, int NC, int L, int background_class_idx,
                          int pose_loss_l2, int train_on_yaw, float gamma, float alpha, float* out, float* jac_pose, float* jac_mom,
                          void* stream);
int odvae_pose_losses_bwd_f32(const float* g, const float* jac_pose, const float* jac_mom, int B, int NC, float* d_dec_pose,
                              float* d_moments, void* stream);

/* ---- linear_f32.hip: small-batch dense layers of the pose-head MLPs (pose_encoder.py:59-131, pose_decoder.py:60-97) ------------ */
size_t odvae_linear_workspace_bytes(int M, int N, int K);
/* y [M][N] = act(x [M][K] . w [N][K]^T + bias); act 0 none | 1 tanh | 2 swish | 3 relu; pre (optional) = the pre-activation */
int odvae_linear_fwd_f32(const float* x, const float* w, const float* bias, int M, int N, int K, int act, float* y, float* pre,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dpre [M][N] = dy * act'(pre); dx [M][K] = dpre . w (or NULL); dw [N][K] = dpre^T . x (or NULL); bias gradient = column sum of dpre */
int odvae_linear_bwd_f32(const float* x, const float* w, const float* pre, const float* dy, int M, int N, int K, int act, float* dpre,
                         float* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ==== bf16 mixed-precision path (BASELINE.json configs[4]; reference knobs: configs/autoencoder/pose/autoencoder_kl_16x16x16.yaml:139
 * `precision`, train.py:521).  Activations bf16 NHWC in HBM, master weights / weight gradients / statistics f32, accumulation f32
 * on v_mfma_f32_32x32x16_bf16.  Every `void*` activation pointer below is bf16 unless the comment says otherwise. ================ */

/* ---- conv_bf16.hip: 3x3 / 1x1 convolutions ([UPSTREAM] ldm model.py via feat_encoder.py:4, feat_decoder.py:4) ---------------- */
int odvae_conv_bf16_reduce_pad(int c);
int odvae_conv_bf16_out_pad(int c);
size_t odvae_conv_bf16_pack_elems(int reduce_c, int out_c, int taps);
/* OIHW f32 weights [Cout][Cin][k][k] (taps = k*k in {1, 9, 16}) -> bf16 MFMA-fragment packs: fwd (reduce Cin, rows Cout) and dgrad
   (reduce Cout, rows Cin, taps flipped); either may be NULL */
int odvae_conv_pack_bf16(const float* w, int Cout, int Cin, int taps, void* fwd_pack, void* dgrad_pack, void* stream);
/* mode 0 stride 1 pad 1 | 1 Downsample pad(0,1,0,1)+stride 2 | 2 nearest-2x + stride 1 | 3 data gradient of mode 1 | 4 = 1x1 with the
   pixels flattened to [N][Hi][Wi] = [1][M/16][16].  x [N][Hi][Wi][Cin] (Cin % 8 == 0), bias f32 or NULL, residual bf16
   [N][Ho][Wo][Cout] or NULL, y bf16 (out_f32 = 0, Cout % 4 == 0) or f32 (out_f32 = 1) */
int odvae_conv_bf16(int mode, const void* x, int N, int Hi, int Wi, int Cin, const void* pack, int Cout, const float* bias,
                    const void* residual, void* y, int Ho, int Wo, int out_f32, void* stream);
/* The stride-1 3x3 conv (mode 0, bf16 output) whose epilogue also leaves the GroupNorm statistics of y -- (sum, sum of squares) of the
 * bf16-rounded values per output tile and channel group, gn_partial [N][odvae_conv_bf16_stats_chunks(H, W)][gn_groups][2], every slot
 * written by exactly one block -- for odvae_groupnorm_fwd_partials_bf16.  odvae_conv_bf16_stats_supported: Cout > 64, groups of whole
 * 4-channel runs that do not straddle a 128-channel block. */
int odvae_conv_bf16_stats_chunks(int H, int W);
int odvae_conv_bf16_stats_supported(int Cout, int gn_groups);
int odvae_conv_bf16_stats(const void* x, int N, int H, int W, int Cin, const void* pack, int Cout, const float* bias, const void* residual,
                          void* y, float* gn_partial, int gn_groups, void* stream);
/* The stride-1 3x3 conv + ReLU of a VGG layer in one launch (replaces torch.relu(F.conv2d(x, w, b, padding=1)) under autocast):
 * y = max(conv(x) + bias, 0) taken on the f32 accumulator in front of the one rounding to bf16; a NaN stays a NaN.  Cout > 32, Cout % 4 == 0.
 * The 3-channel image comes in zero-padded to Cin = 8 (odvae_scaling_layer_bf16). */
int odvae_conv_bf16_relu(const void* x, int N, int H, int W, int Cin, const void* pack, int Cout, const float* bias, void* y, void* stream);
/* The stride-1 3x3 conv whose epilogue writes `mask > 0 ? acc : 0` (mask bf16 [N][H][W][Cout]).  With the data-gradient pack and mask =
 * the stored ReLU output of the layer below it replaces torch's conv2d data gradient followed by threshold_backward (dy * (y > 0)):
 * what reaches HBM is the gradient at that layer's pre-activation.  Cout > 32, Cout % 4 == 0. */
int odvae_conv_bf16_masked(const void* x, int N, int H, int W, int Cin, const void* pack, int Cout, const void* mask, void* y, void* stream);
/* The PatchGAN Conv2d(k=4, pad=1), stride 1 | 2, as an implicit GEMM on bf16 activations (opt-in: NLayerDiscriminator.set_precision
 * ("bf16")); no cols matrix is formed.  Rounding chain: x bf16, weights f32 -> bf16 once in the pack (odvae_conv_pack_bf16, taps = 16),
 * f32 accumulation, bias added in f32, one round-to-nearest-even on the store.
 * dgrad = 0: y [N][Ho][Wo][Cout] = conv(x [N][Hi][Wi][Cin]) + bias, Ho = (Hi - 2) / stride + 1 (Hi, Wi >= 2; an odd Hi at stride 2 leaves
 *   the last padded row unread), pack = the forward pack.  lrelu_slope != 0 (stride 2, bf16 output only): LeakyReLU on the f32
 *   accumulator in front of the one rounding; a NaN stays a NaN.
 * dgrad = 1: x is dy [N][Hi][Wi][Cin = the conv's Cout], pack the data-gradient pack, y = dx [N][Ho][Wo][Cout = the conv's Cin] with
 *   (Ho - 2) / stride + 1 == Hi (checked; stride 1: Ho = Hi + 1), bias NULL.  Stride 2 is the transposed convolution walked by parity
 *   class: every pixel of dx takes exactly its 2x2 of the 16 taps, no tap is masked.
 * Cin % 8 == 0 (the 3-channel image comes zero-padded to 8); y bf16 (out_f32 = 0, Cout % 4 == 0) or f32 (out_f32 = 1, any Cout >= 1:
 * the logit head, and the 3-channel data gradient of the first layer). */
int odvae_conv4x4_bf16(int stride, int dgrad, const void* x, int N, int Hi, int Wi, int Cin, const void* pack, int Cout, const float* bias,
                       void* y, int Ho, int Wo, int out_f32, float lrelu_slope, void* stream);
/* ---- conv_wgrad_bf16.hip: weight gradient, dw f32 OIHW, modes 0 / 1 / 2 / 4 as above, 5 / 6 = Conv2d(k=4, pad=1) at stride 1 / 2
 * (16 taps, Ho = (Hi - 2) / stride + 1); deterministic ------------------------------------------------------------------------ */
size_t odvae_conv_wgrad_bf16_workspace_bytes(int mode, int N, int Ho, int Wo, int Cin, int Cout);
/* host only: out = {splits, output-pixel tiles, tile height, tile width}; split s reduces tiles s, s + splits, ... */
int odvae_conv_wgrad_bf16_plan(int mode, int N, int Ho, int Wo, int Cin, int Cout, int out[4]);
/* db f32 [Cout] (bias gradient = per-channel sum of dy) or NULL, produced in the same pass */
int odvae_conv_wgrad_bf16(int mode, const void* x, const void* dy, int N, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout,
                          float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* ---- flash_attn_bf16.hip: fused single-head attention ([UPSTREAM] AttnBlock.forward), scores never in HBM --------------------- */
int odvae_flash_attn_supported(int N, int T, int C);
/* qkv [N][T][3C] (q | k | v) -> o [N][T][C], lse2 f32 [N][T] = log2 sum_j exp(score_ij * scale) */
int odvae_flash_attn_fwd_bf16(const void* qkv, int N, int T, int C, float scale, void* o, float* lse2, void* stream);
/* dqkv [N][T][3C] from d_o, o, lse2; delta_ws f32 [N*T] scratch */
int odvae_flash_attn_bwd_bf16(const void* qkv, const void* o, const void* d_o, const float* lse2, int N, int T, int C, float scale,
                              void* dqkv, float* delta_ws, void* stream);
/* ---- flash_attn_f32.hip: the same fused attention on f32 operands (exact-f32 MFMA); scores never in HBM ---------------------- */
int odvae_flash_attn_f32_supported(int N, int T, int C);   /* pure host query: N in 1..65535, T >= 1, C in 64/128/256/512 */
/* qkv f32 [N][T][3C] (q | k | v) -> o f32 [N][T][C], lse2 f32 [N][T] = log2 sum_j exp(score_ij * scale) */
int odvae_flash_attn_fwd_f32(const float* qkv, int N, int T, int C, float scale, float* o, float* lse2, void* stream);
/* dqkv f32 [N][T][3C] from d_o, o, lse2; delta f32 [N*T] receives rowsum(d_o * o).  No atomics: bit-reproducible */
int odvae_flash_attn_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse2, int N, int T, int C, float scale,
                             float* dqkv, float* delta, void* stream);
/* ---- linattn_f32.hip: linear attention ([UPSTREAM] LinAttnBlock = LinearAttention(dim C, heads 1, dim_head C)) ------------------
 * q, k, v are the channel thirds of the packed projection [N][T][3C]: pointers to the first token's channels, ld = floats between
 * tokens (3C), stride = floats between images.  k' = softmax(k over the T tokens, per image and channel); ctx [N][C][C],
 * ctx[d][e] = sum_n k'[n][d] v[n][e]; out = q ctx is odvae_gemm_f32.  Softmaxed k is never written; nothing of size T x T exists.
 * Every entry point: ODVAE_ERR_ARG for C not a positive multiple of 32, T < 1, N outside 1..65535 or a null pointer (no launch).
 * All reductions run in a fixed order without atomics: results are bit-reproducible. */
int odvae_linattn_ctx_split(void);     /* tokens per workgroup of the context product: the depth at which it starts to split T */
size_t odvae_linattn_colstats_workspace_bytes(int N, int T, int C);
/* mx [N][C] = max_n k[n][c], rinv [N][C] = 1 / sum_n exp(k[n][c] - mx[c]) */
int odvae_linattn_colstats_f32(const float* k, int ld, int64_t stride, int N, int T, int C, float* mx, float* rinv,
                               void* workspace, size_t workspace_bytes, void* stream);
size_t odvae_linattn_ctx_workspace_bytes(int N, int T, int C);
/* ctx[d][e] = rinv[d] sum_n exp(k[n][d] - mx[d]) v[n][e] on v_mfma_f32_32x32x2_f32, exp applied as k is loaded, T split across workgroups */
int odvae_linattn_ctx_f32(const float* k, const float* v, int ld, int64_t stride, const float* mx, const float* rinv, int N, int T, int C,
                          float* ctx, void* workspace, size_t workspace_bytes, void* stream);
/* backward for k and v from dctx [N][C][C] and g [N][C], g[d] = sum_e ctx[d][e] dctx[d][e]; with s = exp(k - mx) rinv:
 * dv[n][e] = sum_d s[n][d] dctx[d][e], dk[n][d] = s[n][d] (sum_e v[n][e] dctx[d][e] - g[d]); dk, dv: leading dimension ldo, image stride
 * stride_o (the k and v thirds of a packed dqkv).  k, v, mx, rinv, dctx 16-byte aligned, ld and stride multiples of 4. */
int odvae_linattn_dkv_f32(const float* k, const float* v, int ld, int64_t stride, const float* mx, const float* rinv, const float* dctx,
                          const float* g, int N, int T, int C, float* dk, float* dv, int ldo, int64_t stride_o, void* stream);
/* ---- bf16_ops.hip: GroupNorm(32, eps 1e-6) + swish with bf16 activations / f32 statistics, dtype hand-offs ----------------------
 * Shapes every bf16 GroupNorm entry point takes (ODVAE_ERR_ARG otherwise, nothing written): C % 8 == 0, 256 % (C / 8) == 0 (a thread
 * keeps one channel octet: C = 8, 16, 32, ..., 2048 -- no C = 96), C <= 2048, G <= 256, G divides C, N <= 65535 (and HW * C / 8 < 2^31).
 * x, y, dy, dx and dx_add 16-byte aligned. */
size_t odvae_groupnorm_bf16_workspace_bytes(int N, int HW, int C, int G);
int odvae_groupnorm_fwd_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                             void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream);
/* odvae_groupnorm_fwd_bf16 without its statistics pass: partial [N][chunks][G][2] as odvae_conv_bf16_stats left them */
int odvae_groupnorm_fwd_partials_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                      void* y, float* mean, float* rstd, const float* partial, int chunks, void* stream);
int odvae_groupnorm_bwd_bf16(const void* x, const void* dy, int N, int HW, int C, int G, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, int swish, void* dx, float* dgamma, float* dbeta, const void* dx_add,
                             void* workspace, size_t workspace_bytes, void* stream);
/* the dropout forms (see odvae_groupnorm_fwd_drop_f32): the multiply is in f32 before the single rounding of y; dy_eff is not rounded */
int odvae_groupnorm_fwd_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                  double p, unsigned long long seed, void* y, float* mean, float* rstd,
                                  void* workspace, size_t workspace_bytes, void* stream);
int odvae_groupnorm_fwd_partials_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                           double p, unsigned long long seed, void* y, float* mean, float* rstd,
                                           const float* partial, int chunks, void* stream);
int odvae_groupnorm_apply_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                    const float* mean, const float* rstd, int swish, double p, unsigned long long seed, void* y, void* stream);
int odvae_groupnorm_bwd_drop_bf16(const void* x, const void* dy, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, int swish, double p, unsigned long long seed,
                                  void* dx, float* dgamma, float* dbeta, const void* dx_add,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* y bf16 [rows][CP] = x f32 [rows][C], channels C..CP-1 zero (CP % 8 == 0) */
int odvae_cast_pad_bf16(const float* x, int64_t rows, int C, int CP, void* y, void* stream);
int odvae_cast_f32_from_bf16(const void* x, int64_t n, float* y, void* stream);
/* dx [N][H][W][C] = 2x2 sum-pool of du [N][2H][2W][C]: data gradient of F.interpolate(scale 2, nearest) */
int odvae_upsample2x_bwd_bf16(const void* du, void* dx, int N, int H, int W, int C, void* stream);
/* The bf16 forms of odvae_avgpool2x2_f32 / _bwd_f32 / odvae_upsample2x_f32 (C % 8 == 0, C <= 2048): f32 arithmetic, one rounding on the
 * way out; gn_partial holds the statistics of the bf16-rounded result (chunks: odvae_conv_bf16_stats_chunks of the result's H, W) */
int odvae_avgpool2x2_bf16(const void* x, void* y, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream);
int odvae_avgpool2x2_bwd_bf16(const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int odvae_upsample2x_bf16(const void* x, void* u, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream);
size_t odvae_colsum_bf16_workspace_bytes(int64_t rows, int C);
/* out f32 [C] = column sums of x bf16 [rows][C] (bias gradients) */
int odvae_colsum_bf16(const void* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- gan_norm.hip: BatchNorm2d + LeakyReLU of the PatchGAN on bf16 activations, the same kernels instantiated for bf16 elements -----
 * odvae_batchnorm_lrelu_fwd_f32 / _bwd_f32 with x, y, dy, dx bf16 [rows][C]; mean, rstd, running statistics, gamma, beta, dgamma, dbeta
 * f32.  The batch statistics are those of the stored bf16 values, summed about the pivot x[0][c] as in the f32 kernels; each output
 * element is evaluated in f32 and rounded once.  Workspace: odvae_batchnorm_workspace_bytes(rows, C). */
int odvae_batchnorm_lrelu_fwd_bf16(const void* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                                   float momentum, float slope, int train, float* mean, float* rstd,
                                   float* running_mean, float* running_var, void* y,
                                   void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_lrelu_bwd_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                   const float* mean, const float* rstd, float slope, int train,
                                   void* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* odvae_batchnorm_sync_*_f32 with x, dy, dx bf16 (the merge is odvae_batchnorm_sync_stats_merge; the apply is
 * odvae_batchnorm_lrelu_fwd_bf16 with train = 0) */
int odvae_batchnorm_sync_stats_record_bf16(const void* x, int64_t rows, int C, double* record, size_t record_bytes,
                                           void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_sync_bwd_sums_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                       const float* mean, const float* rstd, float slope, double* sums, size_t sums_bytes,
                                       float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int odvae_batchnorm_sync_bwd_dx_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                     const float* mean, const float* rstd, float slope, const double* sums_all, size_t sums_bytes,
                                     int world, const double* m_total, void* dx, void* workspace, size_t workspace_bytes, void* stream);
/* bf16_ops.hip: dx = dy * (y > 0 ? 1 : slope), all bf16, y the LeakyReLU's OUTPUT (slope > 0): the backward of odvae_conv4x4_bf16's epilogue */
int odvae_leaky_relu_bwd_bf16(const void* y, const void* dy, void* dx, float slope, int64_t n, void* stream);

/* ---- lpips_bf16.hip: the LPIPS-style perceptual distance on bf16 features (opt-in: LPIPSStyle.set_precision("bf16")) -------------
 * Features and feature gradients are bf16 NHWC, rounded to nearest even once per store; all arithmetic in between is f32.  A ReLU's
 * backward is folded into the kernel that produces its incoming gradient: `mask` below is the ReLU output that the layer consumed
 * (or NULL), and the kernel writes `mask > 0 ? value : 0`. */
/* lpips.ScalingLayer and the cast into the bf16 net in one pass (replaces ((x - shift) / scale).to(bfloat16) plus the channel pad):
 * x f32 [npix][C], C <= 8 -> y bf16 [npix][8], channels C..7 zero.  Its backward is odvae_scaling_layer_f32(backward = 1) on the f32
 * C-channel data gradient that odvae_conv_bf16(out_f32 = 1) writes. */
int odvae_scaling_layer_bf16(const float* x, const float* shift, const float* scale, void* y, int64_t npix, int C, void* stream);
/* torch.relu's backward on bf16 (threshold_backward): dx = y > 0 ? dy : 0, for a ReLU output whose consumer does not fold the mask in.
 * n % 4 == 0 */
int odvae_relu_bwd_bf16(const void* y, const void* dy, void* dx, int64_t n, void* stream);
/* torch.nn.MaxPool2d(2, 2) on bf16, the semantics of odvae_maxpool2x2_f32 / _bwd_f32: Ho == Hi / 2, Wo == Wi / 2 (floor; checked), an
 * odd last row / column is dropped and gets zero gradient, a NaN window yields NaN, dy goes to the window's first maximum in row-major
 * order (in a NaN window to its first NaN).  C % 4 == 0.  The backward recomputes the maximum from x and writes every element of dx;
 * mask [N][Hi][Wi][C] or NULL: the ReLU output the pool read (then usually x itself). */
int odvae_maxpool2x2_bf16(const void* x, void* y, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
int odvae_maxpool2x2_bwd_bf16(const void* x, const void* dy, const void* mask, void* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
/* odvae_lpips_distance_f32 / _bwd_f32 reading bf16 features (replaces normalize_tensor, the squared difference, the lin layer's 1x1 conv
 * and spatial_average of lpips.py): out f32 [N], f32 arithmetic.  C in {64, 128, 256, 512}; workspace N * 256 floats.
 * Backward: df1 bf16 = round(mask > 0 ? g[n] * d out[n] / d f1 + dnext : 0) -- dnext bf16 [N][HW][C] or NULL is the gradient arriving
 * at the same tensor from the next slice's pool, mask or NULL the tap's own ReLU output (usually f1): one f32 sum, one rounding.  The
 * normalisation term is 0 at an all-zero feature vector, as in the f32 kernel. */
int odvae_lpips_distance_bf16(const void* f0, const void* f1, const float* w, float* out, int N, int HW, int C,
                              void* workspace, size_t workspace_bytes, void* stream);
int odvae_lpips_distance_bwd_bf16(const void* f0, const void* f1, const float* w, const float* g, const void* dnext, const void* mask,
                                  void* df1, int N, int HW, int C, void* stream);

/* ---- anomaly.hip: the NaN check torch.autograd.set_detect_anomaly(True) makes on every backward output, on the device ----------
 * One launch scans up to 8 outputs of one backward node (any dense layout: ptr = lowest element, numel elements).  dtype 0 f32, 1 bf16;
 * mode 0 flags NaN (either sign, quiet or signalling), mode 1 also +-Inf.  A hit does one atomic min of
 * (node_seq << 20) | output_index on *record, so it holds the earliest node and its lowest offending output; clean data leaves it
 * untouched.  odvae_anomaly_reset sets it to ODVAE_ANOMALY_CLEAN.  The descriptors are read on the host and passed in the kernel
 * arguments: the array may be freed when the call returns. */
#define ODVAE_ANOMALY_CLEAN 0x7fffffffffffffffull
typedef struct { const void* ptr; int64_t numel; int32_t dtype; int32_t output_index; } OdvaeAnomalyTensor;
int odvae_anomaly_scan(const OdvaeAnomalyTensor* tensors /* host */, int n, int64_t node_seq, int mode, uint64_t* record, void* stream);
int odvae_anomaly_reset(uint64_t* record, void* stream);

/* ---- vq_f32.hip: the vector quantiser of ldm's VQModel ([UPSTREAM] taming VectorQuantizer2), f32 -------------------------------
 * A row m = (n, p), M = N * HW rows, is one position of a logical [N][D][H][W] tensor addressed by ELEMENT strides (sn, sc, sp):
 * element (n, d, p) is at n sn + d sc + p sp.  NCHW is (D HW, HW, 1); the NHWC memory the conv kernels write is (HW D, 1, D): neither
 * needs a permute copy.  E is the codebook [K][D], row-major.  idx is int64 [M].
 * Sizes: 1 <= D <= 512, 1 <= K <= 2^20, 1 <= M < 2^31, strides sc, sp >= 1, sn >= 0; anything else is ODVAE_ERR_ARG (no launch).
 * Nothing of size M x K is ever written.  No float atomics anywhere: two runs give the same bits, dE included. */
/* out[16]: 0 tile_rows, 1 chunk (codes per LDS chunk), 2 slab depth, 3 slabs per row, 4 nsplit (codebook splits across workgroups),
 * 5 codes_per_split, 6 search grid x, 7 its cap (row tiles beyond it: grid-stride loop), 8 finish workgroups, 9 their cap, 10 codes per
 * sort workgroup, 11 sort code ranges, 12 sort row segments, 13 rows per segment, 14 cap of the streaming grids (256 rows each), 15 0.
 * Host only. */
int odvae_vq_plan(int64_t M, int K, int D, int* out);
size_t odvae_vq_assign_workspace_bytes(int64_t M, int K, int D);
/* idx[m] = argmin_k |e_k|^2 - 2 z_m . e_k: `s < best` from (+inf, 0) over ascending k, so ties go to the lowest k, a row holding NaN
 * gets 0 and every index written is in [0, K).  zq[m] = E[idx[m]] (strides q_*).  The workspace (16-byte aligned) keeps the f64 partial
 * sums of (z_q - z)^2 for odvae_vq_loss_finalize, which must see it untouched. */
int odvae_vq_assign_f32(const float* z, int64_t z_sn, int64_t z_sc, int64_t z_sp, int64_t N, int64_t HW, int D, const float* E, int K,
                        int64_t* idx, float* zq, int64_t q_sn, int64_t q_sc, int64_t q_sp, void* workspace, size_t workspace_bytes,
                        void* stream);
/* *loss = (1 + beta) sum (z_q - z)^2 / (M D) from the workspace of the odvae_vq_assign_f32 call with the same (M, K, D): differences,
 * squares and sums in f64 in a fixed order, one rounding to f32 */
int odvae_vq_loss_finalize(const void* workspace, size_t workspace_bytes, int64_t M, int K, int D, float beta, float* loss, void* stream);
size_t odvae_vq_backward_workspace_bytes(int64_t M, int K, int D);
/* dz = gq + gl (2 c_z / (M D)) (z - E[idx]) and dE[k] = gl (2 c_e / (M D)) sum_{idx[m] = k} (e_k - z_m) (0 for unused codes);
 * legacy != 0: c_z = 1, c_e = beta; legacy == 0: c_z = beta, c_e = 1.  z, gq and dz share the strides; gl is a DEVICE scalar.  gq NULL
 * and gl NULL count as zero; dz NULL or dE NULL skips that half (the workspace is needed for dE only).  f64 arithmetic, one rounding
 * per output.  Indices outside [0, K) are clamped for dz and own no row of dE. */
int odvae_vq_backward_f32(const float* z, const float* gq, float* dz, int64_t sn, int64_t sc, int64_t sp, int64_t N, int64_t HW, int D,
                          const float* E, int K, const int64_t* idx, const float* gl, float beta, int legacy, float* dE, void* workspace,
                          size_t workspace_bytes, void* stream);
/* out[m] = E[clamp(idx[m], 0, K - 1)]: an out-of-range index is CLAMPED, never read past E */
int odvae_vq_gather_f32(const int64_t* idx, int64_t N, int64_t HW, const float* E, int K, int D, float* out, int64_t o_sn, int64_t o_sc,
                        int64_t o_sp, void* stream);
/* counts int32 [K] (zeroed here; indices outside [0, K) are not counted); out[0] = exp(-sum p log(p + 1e-10)), p = count / M;
 * out[1] = number of codes with count > 0.  Integer atomics for the counts, f64 in a fixed order for the rest */
int odvae_vq_usage(const int64_t* idx, int64_t M, int K, int* counts, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ODVAE_HIP_H */
