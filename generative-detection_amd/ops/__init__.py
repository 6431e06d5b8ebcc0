"""torch.autograd.Function wrappers around the C ABI kernels (include/odvae_hip.h).

Activations are logical NCHW tensors in channels_last memory, i.e. NHWC in HBM; conv weights stay OIHW
parameters (checkpoint interchange with the reference) and are repacked per call.
torch supplies device memory, the current stream and autograd bookkeeping; every FLOP and every byte
of the hot path moves through libodvae_hip.so.  No CPU fallback exists.

One module per kernel family; everything they define is re-exported here, so callers keep writing `ops.NAME`.
The switches and the run-time state of the whole op layer are the table below and nothing else: they are attributes of THIS
package, and the family modules read and write them here at call time (`_ops.NAME`), so `ops.NAME = value` or a
`monkeypatch.setattr(ops, NAME, value)` reaches the code that uses it.  `PACK_CACHE` (packs.py) is read the same way.
"""
import os

# ------------------------------------------------------------------------------------------------------
# switches: what the environment can turn on or off (read once, at import)
# ------------------------------------------------------------------------------------------------------
# Upsample + conv3x3: 1 = per output parity class with pre-summed taps (modes 5 / 6, 16 instead of 36 tap-products per
# input pixel); ODVAE_UPCONV_DENSE=1 keeps the dense form (mode 2, data gradient = mode 0 + 2x2 sum-pool) for A/B runs
UPCONV_BY_PARITY = os.environ.get("ODVAE_UPCONV_DENSE", "0") != "1"
# Upsample conv forward / data gradient on the F(4x4,3x3) kernel where the OUTPUT shape qualifies (2.25 instead of 4 multiply-adds per output
# pixel; the weight gradient stays on the parity-class kernel); ODVAE_UPCONV_WINOGRAD4=0 keeps modes 5 / 6
UPCONV_WINOGRAD4 = os.environ.get("ODVAE_UPCONV_WINOGRAD4", "1") != "0"
# ... and its data gradient 2x2-summed inside the F(4x4) output transform (odvae_conv3x3_wino4_pool_f32); ODVAE_UPCONV_POOLED_DGRAD=0: two steps
UPCONV_POOLED_DGRAD = os.environ.get("ODVAE_UPCONV_POOLED_DGRAD", "1") != "0"

# Stride-1 3x3 convs by Winograd F(2x2, 3x3) (conv3x3_wino_f32.hip) when the shape allows; ODVAE_CONV_WINOGRAD=0 keeps
# the direct implicit-GEMM kernel everywhere
WINOGRAD = os.environ.get("ODVAE_CONV_WINOGRAD", "1") != "0"
# Weight gradient of those convs in the Winograd domain (conv3x3_wgrad_wino_f32.hip) where the shape allows (even H, W,
# channel counts in multiples of 128); ODVAE_WGRAD_WINOGRAD=0 keeps the direct weight-gradient kernel everywhere
WGRAD_WINOGRAD = os.environ.get("ODVAE_WGRAD_WINOGRAD", "1") != "0"
# F(4x4, 3x3) (conv3x3_wino4_f32.hip) where the shape allows: 36 products per 4x4 tile instead of 64.  ODVAE_CONV_WINOGRAD4=0/1.
WINOGRAD4 = os.environ.get("ODVAE_CONV_WINOGRAD4", "1") != "0"

# GroupNorm statistics of a conv's output from its own epilogue (conv3x3_wino4_f32.hip): the F(4x4) forward convs leave (sum, sum of
# squares) per output tile and channel group, and the GroupNorm that reads the tensor skips its statistics pass.  ODVAE_GN_FUSED_STATS=0
# turns it off.
GN_FUSED_STATS = os.environ.get("ODVAE_GN_FUSED_STATS", "1") != "0"
# First pass of a GroupNorm's backward (per-channel sums of du * xhat and du) from the epilogue of the data-gradient launch that produces
# its dy: the conv that reads a = swish(GroupNorm(x)) finds the link the GroupNorm left on `a`, its backward runs
# odvae_conv3x3_wino4_gnbwd_f32 and leaves the sums in the link; the GroupNorm's backward then skips gn_bwd_reduce_kernel (one read of x
# and of dy less).  ODVAE_GN_FUSED_BWD=0 turns it off.
GN_FUSED_BWD = os.environ.get("ODVAE_GN_FUSED_BWD", "1") != "0"

# softmax backward folded into the dP product's epilogue; ODVAE_ATTN_UNFUSED=1 keeps the separate row-wise pass
FUSED_SOFTMAX_BWD = os.environ.get("ODVAE_ATTN_UNFUSED", "0") != "1"
# Row softmax folded into the two products of the forward (include/odvae_hip.h, odvae_attn_row_bound_f32 ...): the QK^T epilogue writes
# E = exp(scale (s - bound_i)) against the Cauchy-Schwarz bound of the row's scores, the PV product sums the rows of E beside its multiplies
# and normalises its result; the backward takes P = E / l through row factors.  No softmax pass over the T x T tensor.  A bound too loose
# for f32 (a row whose exponentials all underflow) raises a device flag and predicated fallback launches redo the block with the row
# maximum.  ODVAE_ATTN_FOLDED_SOFTMAX=0: bmm -> softmax pass -> bmm.
ATTN_FOLDED_SOFTMAX = os.environ.get("ODVAE_ATTN_FOLDED_SOFTMAX", "1") != "0"
# f32 path at long sequences.  _Attention keeps the probabilities P [N, T, T] for the backward: 64 MiB per image and block at T = 4 096
# (256 x 256 input), but 1 GiB at T = 16 384 (512 x 512) -- five blocks at B = 32 would hold 160 GiB.  Past this budget (bytes of P per
# block; ODVAE_ATTN_SCORE_BUDGET_GB) the block runs in groups of images through ONE score buffer and keeps only q, k, v and o: the
# backward recomputes P group by group (a fifth product, as a fused attention would) -- no T x T tensor outlives its group.
ATTN_SCORE_BUDGET = int(float(os.environ.get("ODVAE_ATTN_SCORE_BUDGET_GB", "4")) * 2 ** 30)
# Fused f32 attention (flash_attn_f32.hip, _FlashAttentionF32): no T x T tensor in HBM, 7 products per backward instead of the GEMM
# path's 4 (5 past the score budget).  ODVAE_ATTN_F32_FUSED=1 turns it on for supported shapes; off, the dispatch (attention_qkv) is unchanged.
ATTN_F32_FUSED = os.environ.get("ODVAE_ATTN_F32_FUSED", "0") == "1"

# ODVAE_LPIPS_BF16=1: `precision: bf16` takes the perceptual net along (AutoencoderKL.set_precision); default 0 = it stays f32.
LPIPS_BF16 = os.environ.get("ODVAE_LPIPS_BF16", "0") == "1"
# ODVAE_DISC_BF16=1: `precision: bf16` takes the discriminator along (AutoencoderKL.set_precision); default 0 = it stays f32.
DISC_BF16 = os.environ.get("ODVAE_DISC_BF16", "0") == "1"
# ODVAE_DISC_F32_IMPLICIT=1: the f32 PatchGAN's 4x4 convs as implicit GEMMs with their own weight-gradient kernel (_Conv4x4I: no cols
# matrix, what a conv saves is its input); default 0 = im2col + GEMM + col2im (_Conv4x4).  A bf16 discriminator never gets here.
DISC_F32_IMPLICIT = os.environ.get("ODVAE_DISC_F32_IMPLICIT", "0") == "1"

# float32_matmul_precision (the reference's launcher sets 'medium', train.py:521): how many bf16 planes of each f32 operand the
# bf16-split GEMM multiplies (ops/precision.py).  ODVAE_FLOAT32_MATMUL_PRECISION = highest (default: today's bits) | high | medium |
# torch (follow torch.get_float32_matmul_precision() at call time).  The pose head's dense layers stay exact f32 at every level.
FLOAT32_MATMUL_PRECISION = os.environ.get("ODVAE_FLOAT32_MATMUL_PRECISION", "highest").strip().lower() or "highest"
if FLOAT32_MATMUL_PRECISION not in ("highest", "high", "medium", "torch"):
    raise ValueError("ODVAE_FLOAT32_MATMUL_PRECISION must be highest, high, medium or torch, got %r" % os.environ["ODVAE_FLOAT32_MATMUL_PRECISION"])

WGRAD_1X1_GROUP = 0   # tests: force the image-group split of the 1x1 weight gradient at small sizes (0 = only past 2 GiB)
CONV_1X1_GROUP = 0    # tests: the same for the 1x1 forward / data gradient in _conv_b_raw (images per launch; 0 = only past 2 GiB)

# ------------------------------------------------------------------------------------------------------
# run-time state: written by the op layer itself while it runs
# ------------------------------------------------------------------------------------------------------
# True inside `weight_gradient_only()`: the 3x3 conv Functions skip their data gradient.  torch fixes ctx.needs_input_grad at FORWARD time, so a
# torch.autograd.grad(y, weight, grad_outputs=g) probe would otherwise also run (and throw away) the layer's data-gradient launch: the two
# last-layer probes of the adaptive weight (losses.adaptive_weight_one_pass) need decoder.conv_out's weight gradient only.
WEIGHT_GRADIENT_ONLY = False
GN_FUSED_BWD_HITS = 0      # GroupNorm backwards that ran without their reduce pass (diagnostics, tests)
GN_FUSED_BWD_SUSPENDED = 0  # > 0 inside an activation-checkpointed unit (modules.Decoder): a saved tensor of such a unit may be unpacked once per
                            # backward, and the link would read the GroupNorm's from the conv's backward before the GroupNorm's own does
_MATMUL_LEVEL_PUSHED = 0   # the level last given to odvae_gemm_select_precision (the library loads at 0); precision._sync_precision
_ATTN_LAST_FLAG = None     # (diagnostics / tests: the device flag of the last folded-softmax attention forward, 1 if its fallback ran)

# ------------------------------------------------------------------------------------------------------
# the kernel families (imported after the table: they look the names above up here)
# ------------------------------------------------------------------------------------------------------
from ._base import (  # noqa: E402
    CL, _L, BF16, _cl, _new_cl, _ws, _stamp, _stamped, _KernelEvents, KERNEL_EVENTS)
from .packs import (  # noqa: E402
    _PackCache, _PER_WEIGHT_KINDS, _BATCH_KINDS, _batchable, PACK_CACHE, _pack_conv3x3_now, pack_conv3x3)
from .gn_link import (  # noqa: E402
    GN_GROUPS, _GnBwdLink, _gn_bwd_link_of, _gn_stats_ok, _tag_gn_partials, _gn_partials_of, _f32_gn_link, gn_fused_bwd_suspended,
    _tag_gn_output)
from .precision import (  # noqa: E402
    MATMUL_PRECISION_LEVELS, MATMUL_PRECISION_VALUES, _parse_matmul_precision, _matmul_level, _sync_precision,
    set_float32_matmul_precision, get_float32_matmul_precision)
from .gemm import (  # noqa: E402
    gemm, _colsum)
from .conv_bf16 import (  # noqa: E402
    _I31, _conv_b_raw, _pad8, _ConvB, cast_pad_bf16, _ToBF16, to_bf16)
from .perceptual import (  # noqa: E402
    _ScalingLayer, scale_shift, _MaxPool2x2, maxpool2x2, _LpipsDistance, lpips_layer_distance, _conv_relu_b_raw, _conv_masked_b_raw,
    _relu_bwd_b, _ConvReluB, conv3x3_relu_bf16, _scaling_b_raw, _scaling_bwd_raw, _ScalingLayerB, _VggStemB, vgg_stem_bf16,
    _MaxPool2x2B, _LpipsTapB, lpips_tap_bf16)
from .conv import (  # noqa: E402
    _conv3x3_raw, _conv_issued, weight_gradient_only, _wino_ok, _wino4_ok, _conv3x3_wino_raw, CONV3X3_ROUTES, _conv3x3_route, _Conv3x3,
    conv3x3, _Conv1x1, conv1x1)
from .attention import (  # noqa: E402
    _qkv_views, _Attention, _AttentionRecompute, attention_qkv, _LinearAttention, linear_attention_qkv, LINATTN_CTX_SPLIT, _aligned_cl,
    _FlashKind, _FLASH_BF16, _FLASH_F32, _flash_forward, _flash_backward, _FlashAttention, _FlashAttentionF32)
from .norm import (  # noqa: E402
    _GnKind, _GN_F32, _GN_BF16, _gn_forward, _gn_backward, _GroupNorm, _GroupNormB, _gn_drop, group_norm, group_norm_skip,
    group_norm_apply, _RemakeFromNorm, remake_from_norm)
from .resample import (  # noqa: E402
    _RsKind, _RS_F32, _RS_BF16, _rs_in, _rs_forward, _rs_backward, _AvgPool2x2, _AvgPool2x2B, _Upsample2x, _Upsample2xB, avg_pool2x2,
    upsample2x)
from .elementwise import (  # noqa: E402
    _Tanh, tanh, rescale_minmax, _GaussianSample, _GaussianKL, gaussian_sample, gaussian_kl, _L1MaskedSum, l1_masked_sum, _aligned16, _RgbaTerms, rgba_terms, WEIGHT_LAYOUTS, loss_weights_layout, _L1WeightedSums, l1_weighted_sums, _CatMask, cat_mask, nhwc_to_nchw,
    _MulMask, mul_mask, _LatentCombine, latent_combine, LATENT_SAMPLE, LATENT_DROPOUT, LATENT_NOISE, noise_fill, _LatentStage, latent_stage, _flat_f32, ema_tick, ema_update, ema_swap, _PoseLosses, pose_losses, LINEAR_ACTS, _LinearAct, linear_act)
from .patchgan import (  # noqa: E402
    _conv4x4_out, _Conv4x4, _conv4x4_i_raw, _check_pack_current, _Conv4x4I, conv4x4, _BatchNormLReLU, batchnorm_lrelu, _ActNormLReLU, actnorm_init, actnorm_lrelu, _LeakyReLU,
    leaky_relu, _GanLogitTerms, gan_logit_terms, _conv4x4_b_raw, _Conv4x4B, conv4x4_bf16, _gather_f64, _SyncBatchNormLReLU, _sync_group)
from .vq import (  # noqa: E402
    VQ_PLAN_FIELDS, vq_plan, _row_strides, _rows_view, _dense, _codebook, _VqQuantize, vq_quantize, vq_gather, vq_usage)
