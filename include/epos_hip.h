/*
 * epos_hip.h -- C ABI of libepos_hip.so, the MI355X (gfx950) implementation of
 * the EPOS inference hot path (thodan/epos): DeepLabv3+/Xception-65 forward,
 * many-to-many 2D-3D correspondence extraction, per-object PnP-RANSAC.
 *
 * Conventions
 *   - plain pointers and sizes only; every `d_*` / `const float* x` marked
 *     [device] is a DEVICE pointer (HBM), everything else is host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     device entry points only enqueue work on it and never synchronise, so
 *     they can be captured into a hipGraph;
 *   - return value: 0 = OK, < 0 = error (EPOS_E_*); -1000 - hipError_t for HIP
 *     runtime failures. epos_last_error() gives a message for the last failure
 *     on the calling thread;
 *   - activations are NHWC fp32 (the reference's layout and dtype,
 *     SURVEY.md section 8); `ld*` are row strides in ELEMENTS so that a kernel
 *     can read or write a channel slice of a wider (concat) buffer.
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef EPOS_HIP_H_
#define EPOS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPOS_OK 0
#define EPOS_E_INVALID (-1)   /* bad argument (NULL, non-multiple-of-4 channels, ...) */
#define EPOS_E_CAPACITY (-2)  /* caller-provided output capacity too small */
#define EPOS_E_NODEVICE (-3)  /* no HIP device available */
#define EPOS_E_INTERNAL (-4)  /* a device-side consistency check failed (see epos_last_error) */
#define EPOS_E_HIP_BASE (-1000)

#define EPOS_ABI_VERSION 7   /* 2: EposPointwiseArgs.Ws, EposConv3x3Args.Ws, split weight packing; 3: epos_separable_conv_f32; 4: epos_solve_pnp_ransac; 5: fp16-pair GEMM (Wh, a_amax, c_amax, epos_pack_pointwise_weights_h2, epos_absmax_f32); 6: epos_separable_conv_f32 with fp16-pair intermediates on the fp16-pair kernel, epos_separable_conv_fused_state ; 7 (round 5, the diet): the measured-slower opt-ins left the library -- EposSepConvArgs lost sync / stats and epos_separable_conv_f32 issues the two launches, EposPointwiseArgs.softmax64 is reserved, removed: epos_separable_conv_sync_words, epos_separable_conv_fused_state, epos_set_h2_latency_tile_limit, epos_pointwise_workspace_bytes, epos_pointwise_conv_grouped_ws_f32, epos_pointwise_conv_grouped_sk_f32 */

int epos_abi_version(void);
const char* epos_last_error(void);
/* Number of visible HIP devices (>= 0) or a negative error. */
int epos_device_count(void);
/* Measurement aid (bench.py): a one-wave kernel on `stream` that spins for
 * `microseconds` and writes {shader-clock cycles, 100 MHz ticks} to the DEVICE
 * buffer out2[2] -- cycles / ticks * 100 = the core clock in MHz while the
 * surrounding work runs (the fp32 MFMA roof scales with it). */
int epos_clock_probe(int64_t* out2, int microseconds, void* stream);

/* ------------------------------------------------------------------------- *
 * Network layers (replace the TF1.12 ops that model.py / net_xception.py lower
 * to; call sites: SURVEY.md section 2.2).
 * ------------------------------------------------------------------------- */

/* Packs a 1x1-conv weight matrix W[K][N] (TF HWIO with H=W=1, i.e. [Cin][Cout])
 * into the tile order the MFMA kernel streams: [ceil(K/32)*8][Npad][4] floats,
 * Npad = round_up(N, 128), zero padded. Host-side helper (host pointers).
 * Returns the number of floats written (or required, if dst == NULL). */
int64_t epos_pack_pointwise_weights(const float* w_kn, int K, int N, float* dst);

/* The same matrix for the split-operand GEMM (pointwise_gemm_split_f32): every fp32
 * weight is cut into three bf16 pieces (8 + 8 + 8 significand bits; the cut itself is
 * exact, hi + mid + lo == w) and stored in the fragment order of
 * v_mfma_f32_32x32x16_bf16. The kernel then forms each product a*w from SIX of the nine
 * piece products (the three lowest-order cross terms, below 2^-23 |a*w|, are dropped):
 * fp32-equivalent, not exact -- its measured error against fp64 is below the fp32-MFMA
 * kernel's (tests/test_gpu_layers.py). Layout:
 * [ceil(N/128)][ceil(K/16)][4 column blocks][3 pieces][64 lanes][8 bf16], zero padded.
 * Host-side helper (host pointers). Returns the number of BYTES written (or required,
 * if dst == NULL). */
int64_t epos_pack_pointwise_weights_split(const float* w_kn, int K, int N, void* dst);

/* The same matrix for the fp16-pair GEMM (pointwise_gemm_h2_f32, the default fp32 GEMM
 * since round 3): every column n is scaled by a power of two 2^e_n that puts its largest
 * weight into [2^14, 2^15), and every scaled weight t is stored as TWO fp16 values
 *     hi = rn_fp16(t),  mid = rn_fp16((t - hi) * 2^11)        (t - hi is exact in fp32)
 * so that hi + mid * 2^-11 carries 22-23 significant bits of t (error <= 1 ulp of the 24-bit
 * significand). The kernel forms a*w from THREE fp16 MFMA products,
 *     ah*wh                      (main accumulator)
 *     ah*wm + am*wh              (correction accumulator, scaled by 2^-11 in the epilogue)
 * (am*wm, below 2^-22 |a*w| and of random sign, is dropped): fp32-equivalent, not exact; its
 * measured error against fp64 is below the fp32-MFMA kernel's (tests/test_gpu_layers.py).
 * Half the matrix-pipe work of the bf16 x 6 split above, 4 instead of 6 bytes per weight.
 * Layout: [ceil(N/128)][ceil(K/16)][4 column blocks][2 pieces][64 lanes][8 fp16] (fragment
 * order of v_mfma_f32_32x32x16_f16), then round_up(N,128) floats 2^-e_n.
 * Every finite matrix qualifies (round 6): a scaled weight t is reproduced to
 *     |hi + mid * 2^-11 - t| <= max(2^-22 |t|, 2^-36)
 * i.e. to full precision down to 2^-28 of its column's maximum and, below that (fp16
 * subnormal pieces, which the matrix pipe does not flush), with an ABSOLUTE error of at most
 * 2^-50 x the column maximum -- the same graceful degradation as the activation side, and
 * below the fp32 rounding of any sum the column's larger weights take part in. (Until ABI 7's
 * first release a single such weight made the packer refuse the whole matrix.) The function
 * returns 0 and writes nothing only for Inf / NaN weights or a column whose scale leaves the
 * fp32 exponent range (column maximum outside ~2^-85 .. 2^115); the caller then keeps the
 * bf16 x 6 split kernel for this layer (Wh = NULL).
 * Host-side helper (host pointers). Returns the number of BYTES written (or required, if
 * dst == NULL; 0 = not representable). */
int64_t epos_pack_pointwise_weights_h2(const float* w_kn, int K, int N, void* dst);

/* Absolute-maximum slots. The fp16-pair GEMM scales its fp32 A operand by a power of two
 * chosen from an UPPER BOUND of max|A| that it reads from device memory when it starts:
 * a slot is 64 uint32 words [device] holding the bit patterns of non-negative floats; the
 * bound is the maximum over the 64 words. Producers combine into a slot with atomic max
 * (the GEMM epilogues do when c_amax is given; epos_absmax_f32 does for any other tensor);
 * the caller zeroes a slot (epos_amax_clear) before the first producer of the step runs.
 * Any upper bound is valid (max-pool / subsample / bilinear resize outputs may reuse their
 * input's slot); a bound that is too large by 2^j costs j of the ~27 octaves below the
 * bound within which elements keep full precision. Overflow is impossible by construction.
 *
 * epos_absmax_f32: slot = max(slot, max |X[r, 0..cols)|) over `rows` rows of ldx floats. */
#define EPOS_AMAX_WORDS 64
int epos_absmax_f32(const float* X, int64_t ldx, int64_t rows, int64_t cols,
                    uint32_t* slot, void* stream);
/* Zeroes n_slots consecutive slots (a kernel on `stream`: a memset NODE of a captured graph
 * is not reliably ordered before the kernel nodes behind it when graphs replay concurrently). */
int epos_amax_clear(uint32_t* slots, int64_t n_slots, void* stream);

/* out[m, n] = act( sum_k A[row(m), k] * W[k, n] + bias[n] (+ R[m, n]) )
 * = slim.conv2d(kernel 1x1, stride `sub`) + folded BatchNorm (+ residual add)
 * (+ ReLU): net_xception.py:167-182 (pointwise half of separable_conv2d_same),
 * :296-302 (shortcut), model.py:223-224,237,257-258,349-352 (ASPP/decoder 1x1),
 * model.py:449-456 (logits, bias, no BN).
 * A [device]: rows of `lda` floats; with sub > 1 the row of output pixel
 * (b, y, x) is input pixel (b, y*sub, x*sub) of a [B, Hi, Wi] map (TF 'SAME'
 * 1x1 stride-2 conv samples even indices); M = B*Ho*Wo output pixels.
 * Wp [device]: packed by epos_pack_pointwise_weights; bias [device]: Npad floats
 * (or NULL); R [device]: optional residual rows of ldr floats; C [device]: output
 * rows of ldc floats. K % 4 == 0, lda % 4 == 0 required. */
typedef struct EposPointwiseArgs {
  const float* A; int64_t lda;
  const float* Wp; const float* bias;
  const float* R; int64_t ldr;
  float* C; int64_t ldc;
  int32_t M, N, K;
  int32_t relu;       /* apply ReLU last */
  int32_t relu_in;    /* apply ReLU to A on load (pre-activation). Served by the M <= 8 GEMV
                       * only (below): with M > 8 the library refuses it (EPOS_E_INVALID) */
  int32_t sub;        /* spatial subsampling of A rows (1 or 2) */
  int32_t Ho, Wo, Hi, Wi;   /* only read when sub > 1 */
  const void* Ws;     /* optional [device]: the same weights packed by
                       * epos_pack_pointwise_weights_split (NULL = not provided) */
  /* ---- Which kernel runs a call. ONE problem with M <= 8 and sub == 1: a GEMV on Wp alone
   *      (Ws, Wh and the a_* fields are ignored; the only kernel that applies relu_in). Every
   *      other call needs relu_in == 0 and M > 8 in every problem: the fp16-pair GEMM (ABI 5)
   *      when every problem brings Wh (EPOS_GEMM_H2=0 disables it), else the bf16 x 6 kernel
   *      when every problem brings Ws. Anything else is refused with EPOS_E_INVALID before a
   *      launch: a problem with M <= 8 inside a group or with sub > 1 (whatever weights it
   *      brings; epos_last_error() says so), relu_in with M > 8, and a problem with neither
   *      Wh nor Ws -- the fp32-MFMA kernels are in the test build (libepos_hip_ref.so) only,
   *      where they take these calls. */
  const void* Wh;     /* optional [device]: epos_pack_pointwise_weights_h2 of the weights */
  const uint32_t* a_amax;   /* optional [device]: slot bounding max|A| (see above). NULL
                       * with Wh given: the library measures A itself first (one memset +
                       * one reduction launch into an internal slot ring of 256 slots --
                       * convenient for single calls; plans pass their own slots) */
  const uint32_t* a_amax2;  /* optional second slot: the bound is the larger of the two
                       * (A = a concat written by two producers) */
  float a_gain, a_bias; /* bound = a_gain * slot + a_bias (a_gain == 0 reads as 1, 0):
                       * A = a depthwise conv of the tensor the slot describes,
                       * a_gain = max_c sum_taps |w|, a_bias = max_c |bias| */
  int32_t a_presplit; /* A is already fp16 pairs (EposDepthwiseArgs.y_h2 wrote it with the
                       * same a_amax / a_amax2 / a_gain / a_bias): needs Wh and a_amax */
  uint32_t* c_amax;   /* optional [device]: slot that receives max|C| over the elements
                       * this call writes (atomic max). Needs the float4 epilogue:
                       * N % 4 == 0, ldc % 4 == 0, C (and R) 16-byte aligned, relu_in == 0,
                       * M > 8; EPOS_E_INVALID otherwise */
  /* ---- ABI 6 */
  float* col_sums;    /* optional [device]: [ceil(M / 32)][col_ld] -- the epilogue also writes,
                       * for every block of 32 consecutive rows, the column sums of what it
                       * stores (after bias / ReLU), in a fixed order. With rows = the pixels of
                       * an image (H*W % 32 == 0) epos_global_avg_pool_partial_f32 turns them
                       * into the per-image channel means (model.py:220) without re-reading
                       * the tensor. fp16-pair kernel only (EPOS_E_INVALID otherwise), no
                       * residual, N % 4 == 0 */
  int64_t col_ld;
  int32_t c_stream;   /* != 0: write C with streaming (non-temporal) stores -- for outputs that
                       * are not re-read soon (the 413 MB of dense heads would otherwise sweep
                       * the 256 MB Infinity Cache clean of the other images' working sets);
                       * fp16-pair kernel's float4 epilogue only, ignored elsewhere */
  int32_t reserved0;  /* 0 (ABI 6 carried a fused fragment softmax here; measured slower than
                       * its own launch, removed in ABI 7: profiles/r04/ab_head_softmax.txt) */
} EposPointwiseArgs;
int epos_pointwise_conv_f32(const EposPointwiseArgs* args, void* stream);

/* Grouped form: `count` (1..8) independent problems in ONE launch, so that small
 * problems (the four ASPP branches, the three logit heads, a shortcut next to a
 * separable conv) fill the chip together. All problems of a group must agree on
 * relu_in, on a_presplit and on whether a residual is present. On the fp16-pair kernel a
 * group WITH residuals is issued as `count` consecutive launches (same bits: an element's value
 * does not depend on the launch that computes it; the one-launch form with residuals measured
 * no better and left the library in ABI 7); if one of them fails the earlier ones are already
 * enqueued and epos_last_error() names the failing problem's index. */
int epos_pointwise_conv_grouped_f32(const EposPointwiseArgs* args, int count,
                                    void* stream);

/* The dense logits heads: the same contract and the same bits as
 * epos_pointwise_conv_grouped_f32. A group whose problems share one A (pointer, lda, M and
 * absmax slots / gain / bias; a_amax given), have K = 256, sub = 1, fp16-pair weights and no
 * residual, ReLU, pre-split A, c_amax or col_sums runs on an A-stationary kernel (each A
 * panel loaded and split once for many N tiles); any other group is passed on to
 * epos_pointwise_conv_grouped_f32. */
int epos_heads_gemm_f32(const EposPointwiseArgs* args, int count, void* stream);
/* Which way epos_heads_gemm_f32 would go (added without an ABI version change: nothing
 * existing moved). Returns 1 if it would launch the A-stationary kernel for this group, 0 if it
 * would pass the group on, < 0 for a bad count. With 1 and plan != NULL, plan[5] (host)
 * receives what the launch computes, through the same routine: {nt = 64-column tiles per
 * panel, panels = ceil(M / 128), range = tiles per work item, nr = ranges per panel, grid
 * blocks}. cus: compute units to balance for; 0 = the current device's. Host code: no pointer
 * in args is dereferenced, and with cus > 0 no device is needed. */
int epos_heads_gemm_plan(const EposPointwiseArgs* args, int count, int cus, int32_t* plan);

/* (ABI <= 6 also had a persistent stream-K form of the grouped GEMM on the fp32-MFMA ring,
 * epos_pointwise_conv_grouped_sk_f32 / _ws_f32 + a workspace: correct, tested, and slower
 * than the data-parallel kernels end to end (177 vs 213 images/s in round 1); removed in
 * ABI 7 -- DESIGN.md "Stream-K", history up to commit 1b05025.) */

/* Dense 3x3 conv + folded BatchNorm (+ ReLU) as an IMPLICIT GEMM: the im2col matrix
 * only exists as LDS tiles filled by LDS-DMA from the shifted input pixels. Semantics =
 * resnet_utils.conv2d_same (external/slim/nets/resnet_utils.py:77-122): stride 1 ->
 * 'SAME' with dilation `rate` (zero pad = rate); stride 2 -> zero pad `rate` on every
 * side + VALID. Output (y, x) reads input (y*stride + (ky-1)*rate, x*stride + (kx-1)*rate).
 * Replaces conv1_2 (net_xception.py:462-463) and the stride-1 root convs and the
 * bottleneck 3x3 convs of net_resnet_v1_beta.py:38-112. X [device]: [B, H, W] pixels,
 * rows of ldx floats, Cin channels used (Cin % 32 == 0); Wp [device]:
 * epos_pack_pointwise_weights of the [9*Cin][Cout] matrix whose row (ky*3+kx)*Cin + c is
 * TF's HWIO w[ky][kx][c][:]; bias [device]: round_up(Cout,128) floats or NULL; Y
 * [device]: [B, Ho, Wo] rows of ldy floats, Ho = (H-1)/stride + 1. */
typedef struct EposConv3x3Args {
  const float* X; int64_t ldx;
  const float* Wp; const float* bias;
  float* Y; int64_t ldy;
  int32_t B, H, W, Cin, Cout;
  int32_t stride, rate;
  int32_t relu;
  const void* Ws;     /* optional [device]: epos_pack_pointwise_weights_split of the same
                       * [9*Cin][Cout] matrix (NULL without Wh: refused -- the
                       * fp32-MFMA kernel is in the test build only) */
  /* ---- ABI 5, as in EposPointwiseArgs */
  const void* Wh;     /* optional [device]: epos_pack_pointwise_weights_h2 of that matrix */
  const uint32_t* x_amax;   /* optional [device]: slot bounding max|X| */
  uint32_t* y_amax;   /* optional [device]: receives max|Y| */
} EposConv3x3Args;
int epos_conv3x3_f32(const EposConv3x3Args* args, void* stream);

/* Depthwise 3x3 conv + folded BatchNorm (+ optional ReLU before and after):
 * the depthwise half of net_xception.py:167-182 / model.py:80-88. stride 1 ->
 * TF 'SAME' (zero pad `rate`); stride 2 -> fixed_padding (net_xception.py:74-93)
 * + VALID, i.e. zero pad 1 before / 1 after with rate 1. w9c [device]: [9][C]
 * tap-major, BN scale folded in; bias [device]: [C]. C % 4 == 0. */
typedef struct EposDepthwiseArgs {
  const float* X; int64_t ldx;     /* [B, Hi, Wi] pixels, rows of ldx floats */
  const float* w9c; const float* bias;
  float* Y; int64_t ldy;           /* [B, Ho, Wo] pixels */
  int32_t B, Hi, Wi, Ho, Wo, C;
  int32_t stride, rate;
  int32_t relu_in, relu_out;
  /* ---- ABI 5: fp16-pair OUTPUT for the fp16-pair GEMM that consumes Y (its A operand).
   * y_h2 != 0: instead of 4 fp32 values per 16 bytes the kernel writes, for the same 4
   * channels c..c+3, [hi(c) hi(c+1) hi(c+2) hi(c+3) | mid(c) .. mid(c+3)] (8 fp16 = the same
   * 16 bytes, same addresses, same ldy): hi = rn_fp16(y * s), mid = rn_fp16((y * s - hi) *
   * 2^11), s = the power of two that puts the BOUND  gain * max(x_amax, x_amax2) + bias0
   * into [2^14, 2^15). The bound must hold for |Y| (gain = max_c sum_taps |w|, bias0 =
   * max_c |bias| with x_amax bounding |X|); the GEMM (EposPointwiseArgs.a_presplit, same
   * slots / gain / bias) derives the same s. Each activation is then split ONCE instead of
   * once per column tile of the GEMM, and the GEMM's loop carries no conversion at all. */
  int32_t y_h2;
  const uint32_t* x_amax;
  const uint32_t* x_amax2;   /* optional second slot */
  float gain, bias0;
} EposDepthwiseArgs;
int epos_depthwise3x3_f32(const EposDepthwiseArgs* args, void* stream);

/* Separable conv as ONE call: depthwise 3x3 (+BN, ReLU before/after) followed by the
 * pointwise 1x1 (+BN, +residual, +ReLU) -- slim.separable_conv2d as net_xception.py:96-194
 * (separable_conv2d_same, stride 1) and model.py:58-97 (split_separable_conv2d) build it.
 * Requirements: pw.A == dw.Y, pw.lda == dw.ldy, pw.K == dw.C, pw.M == dw.B * dw.Ho * dw.Wo.
 * dw.Y [device] keeps the depthwise output (fp32, or fp16 pairs with dw.y_h2 +
 * pw.a_presplit). Since ABI 7 this is exactly epos_depthwise3x3_f32(&dw) followed by
 * epos_pointwise_conv_f32(&pw) on the stream: the single-launch forms of rounds 2 and 4
 * (depthwise as a producer phase of the GEMM's workgroups, on the bf16 x 6 and on the
 * fp16-pair kernel; both bit-identical to the two launches) measured slower on every
 * configuration (C2 351 vs 420, C3 359 vs 425 images/s; profiles/r02, r04, r05) and left the
 * product library in round 5 -- DESIGN.md (e), git history up to commit 1b05025. */
/* The fp16-pair GEMM takes 128 x 64 instead of 128 x 128 output tiles for a launch with at
 * most `max_tiles` 128 x 128 tiles (default 100; environment EPOS_H2_BN64_MAX_TILES; 0 =
 * never): launches that would leave most CUs idle (ASPP 1x1 of one image: 76 tiles) get
 * twice the workgroups. Results do not depend on the tile. Returns the previous limit.
 * Process-wide; meant for tuning and for the tests that run both tiles. */
int epos_set_h2_narrow_tile_limit(int max_tiles);
typedef struct EposSepConvArgs {
  EposDepthwiseArgs dw;
  EposPointwiseArgs pw;
} EposSepConvArgs;
int epos_separable_conv_f32(const EposSepConvArgs* args, void* stream);

/* im2col for a dense 3x3 conv (slim resnet_utils.conv2d_same,
 * external/slim/nets/resnet_utils.py:77-122, used at net_xception.py:460-463):
 * col[m, (ky*3+kx)*C + c] = X[b, y*stride - pad + ky*rate, x*stride - pad + kx*rate, c]
 * (zero outside), columns zero-padded to ldcol. With preprocess != 0 the input
 * is first mapped x -> x*(2/255) - 1 (feature.py:171-174) for in-bounds taps. */
typedef struct EposIm2colArgs {
  const float* X; int64_t ldx;
  float* col; int64_t ldcol;
  int32_t B, Hi, Wi, Ho, Wo, C;
  int32_t stride, rate, pad;
  int32_t preprocess;
  /* ---- ABI 6: optional [device] absmax slot table to zero in the same launch (amax_words
   * uint32 words; must not exceed the launch's thread count = B*Ho*Wo*ldcol): a plan whose
   * first launch is this one needs no epos_amax_clear launch of its own */
  uint32_t* amax_clear;
  int64_t amax_words;
} EposIm2colArgs;
int epos_im2col3x3_f32(const EposIm2colArgs* args, void* stream);

/* im2col for a dense k x k conv with a choice of fused input preprocessing (the root convs
 * of every backbone, feature.py:157-185; the 7x7 stride-2 conv1 of resnet_v1_50 / _101,
 * net_resnet_v1_beta.py:168-173):
 * col[m, (ky*k+kx)*C + c] = pre(X[b, y*stride - pad + ky*rate, x*stride - pad + kx*rate, c])
 * for in-bounds taps and 0 for padded ones (the reference preprocesses the image, then
 * conv2d_same pads it with zeros); columns k*k*C .. ldcol are zero-filled. Same output
 * contract as epos_im2col3x3_f32, which this equals bit for bit at k = 3.
 * pre: EPOS_PREPROCESS_NONE x; _UNIT_RANGE (2/255) x - 1 (_preprocess_zero_mean_unit_range);
 * _SUB_MEAN x - mean_rgb[c] for c < 3 and x for c >= 3 (_preprocess_subtract_imagenet_mean).
 * Needs ldcol % 4 == 0 and a 16-byte aligned col (one float4 store per thread).
 * amax_clear / amax_words: as in EposIm2colArgs; amax_words <= Wo*ldcol/4 * min(B*Ho, 65535). */
#define EPOS_PREPROCESS_NONE 0
#define EPOS_PREPROCESS_UNIT_RANGE 1
#define EPOS_PREPROCESS_SUB_MEAN 2
typedef struct EposIm2colKArgs {
  const float* X; int64_t ldx;
  float* col; int64_t ldcol;
  int32_t B, Hi, Wi, Ho, Wo, C;
  int32_t k, stride, rate, pad;
  int32_t preprocess;
  float mean_rgb[3];
  uint32_t* amax_clear;
  int64_t amax_words;
} EposIm2colKArgs;
int epos_im2col_f32(const EposIm2colKArgs* args, void* stream);

/* Per-image channel means from the 32-row block sums an fp16-pair GEMM wrote
 * (EposPointwiseArgs.col_sums): Y[b, c] = (sum over the `blocks` blocks of image b) / hw. */
int epos_global_avg_pool_partial_f32(const float* P, int64_t ldp, float* Y, int32_t B,
                                     int32_t blocks, int32_t C, int32_t hw, void* stream);

/* Global mean over H*W (model.py:220): X [B, HW, C] (ldx) -> Y [B, C].
 *
 * The glue launchers below (mean, resize, max pool, subsample, add+relu, argmax and their bf16
 * forms) refuse with EPOS_E_INVALID, before anything is launched, every call under which a
 * kernel would leave the tensors it was given: a pitch below the channel count (ldx < C,
 * ldy < C), a batch, map size or channel count below 1, a negative element count. These calls
 * were never valid; the refusals are additive (ABI version unchanged). */
int epos_global_avg_pool_f32(const float* X, int64_t ldx, float* Y, int B,
                             int HW, int C, void* stream);

/* Bilinear resize, align_corners=True (misc.py:94-107 -> tf.image.resize_bilinear):
 * X [B, Hi, Wi, C] (ldx) -> Y [B, Ho, Wo, C] (ldy). Hi = Wi = 1 broadcasts
 * (image-pooling branch, model.py:225-226). C % 4 == 0. */
int epos_resize_bilinear_f32(const float* X, int64_t ldx, float* Y, int64_t ldy,
                             int B, int Hi, int Wi, int Ho, int Wo, int C,
                             void* stream);

/* ResNet-v1-beta backbone helpers (BASELINE config C5). max pool 3x3 stride 2,
 * TF 'SAME' (slim.max_pool2d at net_resnet_v1_beta.py:190): X [B,Hi,Wi,C] ->
 * Y [B,ceil(Hi/2),ceil(Wi/2),C]. */
int epos_maxpool3x3_s2_f32(const float* X, int64_t ldx, float* Y, int64_t ldy,
                           int B, int Hi, int Wi, int C, void* stream);
/* slim resnet_utils.subsample (external/slim/nets/resnet_utils.py:59-74): keeps
 * every factor-th pixel, Y [B,(Hi-1)/f+1,(Wi-1)/f+1,C]. */
int epos_subsample_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int B,
                       int Hi, int Wi, int C, int factor, void* stream);
/* Y = relu(A + B) over n contiguous floats (net_resnet_v1_beta.py:86 when the
 * pre-sum conv3 output is itself an end point, feature.py:50-54). */
int epos_add_relu_f32(const float* A, const float* B, float* Y, int64_t n,
                      void* stream);

/* Sparse update: for b < n_blocks, dst[offsets[b] .. offsets[b] + width) = src[b * width ..]
 * (all pointers [device]; offsets in elements; blocks must not overlap). Synthetic-workload
 * support: bench.py --planted-poses overwrites the head values of the target objects with
 * values rendered from known poses, between the network and the correspondence stage. */
int epos_scatter_blocks_f32(float* dst, const int64_t* offsets, const float* src,
                            int64_t n_blocks, int width, void* stream);

/* uint8 -> float32, n values (both pointers [device], 16-byte aligned): the
 * tf.cast(decode_image(...), tf.float32) of the reference's input pipeline
 * (datagen.py:435-436) done on the device, so that decoded frames are uploaded as bytes.
 * Exact. */
int epos_u8_to_f32(const uint8_t* X, float* Y, int64_t n, void* stream);

/* In-place softmax over groups of `G` consecutive floats (model.py:677-678):
 * X holds n_groups * G floats, group g at X + g*G, 1 <= G <= 256 (the object head's
 * O + 1 classes, or the F fragments of one object); G > 256: EPOS_E_INVALID. */
int epos_softmax_groups_f32(float* X, int64_t n_groups, int G, void* stream);

/* Per-pixel argmax over C channels -> int64 label (model.py:683); first maximum
 * wins (tf.argmax / np.argmax tie rule). C >= 1, ldx >= C, P >= 0 (P == 0: nothing to do). */
int epos_argmax_i64(const float* X, int64_t ldx, int64_t* labels, int64_t P,
                    int C, void* stream);

/* ------------------------------------------------------------------------- *
 * Correspondence extraction (replaces epos_lib/corresp.py:9-101,
 * establish_many_to_many, and misc.py:14-26).
 * One "slot" = one (image, object) pair to extract.
 * ------------------------------------------------------------------------- */
typedef struct EposCorrSlot {
  int32_t image;     /* image index in the batch */
  int32_t obj_id;    /* 1-based object id: channel obj_id of obj_confs,
                        channel obj_id-1 of the fragment heads (corresp.py:46,60) */
} EposCorrSlot;

/* Fragment-confidence softmax (model.py:678) for the given slots only: X is the
 * dense frag_conf buffer f32 [B, P, O, F], 1 <= F <= 256 (F > 256: EPOS_E_INVALID);
 * slots [device]. Used by the sparse-head mode, where the fragment heads exist only for
 * the target objects. Same bits as epos_softmax_groups_f32 on those groups. */
int epos_softmax_slots_f32(float* X, const EposCorrSlot* slots, int S, int P,
                           int O, int F, void* stream);

/* Pass 1+2: per slot, count masked pixels and correspondences and compute the
 * raster-order exclusive offsets. All buffers [device].
 *   obj_confs  f32 [B, P, O+1]      (P = h*w pixels of the head map)
 *   frag_confs f32 [B, P, O, F]     (1 <= F <= 256; F > 256: EPOS_E_INVALID)
 *   px_off, corr_off  i32 [S, P]    scratch/outputs (exclusive scans)
 *   frag_mask  u64 [S, P, NW]       kept-fragment bitmask per pixel (all 0 = not masked),
 *                                   NW = ceil(F / 64) words; word k holds fragments
 *                                   64k..64k+63, bit f - 64k. For F <= 64: [S, P].
 *   totals     i32 [S, 2]           {masked pixels, correspondences} per slot
 */
int epos_corr_count(const float* obj_confs, const float* frag_confs,
                    const EposCorrSlot* slots /*[device]*/, int S, int B, int P,
                    int O, int F, float min_obj_conf, float min_frag_rel_conf,
                    int32_t* px_off, int32_t* corr_off, uint64_t* frag_mask,
                    int32_t* totals, void* stream);

/* Pass 3: fills the correspondence arrays (same F range and frag_mask layout as
 * epos_corr_count; rows of a pixel in ascending fragment id). slot_base i64[S] [device] gives each
 * slot's first row in the pooled output arrays (exclusive scan of totals[:,1],
 * computed by epos_corr_slot_bases or by the host); `capacity` rows are
 * available; rows beyond it are not written and *overflow is set to 1.
 *   frag_coords f32 [B, P, O, F, 3]
 *   frag_centers f64 [O, F, 3], frag_sizes f64 [O, F]  (model store, obj_id-1 major)
 * Outputs [device]: px_id i64[N], frag_id i64[N], coord_2d f64[N,2],
 * coord_3d f64[N,3], conf/conf_obj/conf_frag f32[N] with the exact arithmetic of
 * corresp.py:55-57,71-78,82-84 (see oracle/corresp_ref.py). W = head map width,
 * inv_scale = 1 / output_scale. */
typedef struct EposCorrOut {
  int64_t* px_id; int64_t* frag_id;
  double* coord_2d; double* coord_3d;
  float* conf; float* conf_obj; float* conf_frag;
} EposCorrOut;
int epos_corr_fill(const float* obj_confs, const float* frag_confs,
                   const float* frag_coords, const double* frag_centers,
                   const double* frag_sizes, const EposCorrSlot* slots, int S,
                   int B, int P, int W, int O, int F, double inv_scale,
                   const int32_t* px_off, const int32_t* corr_off,
                   const uint64_t* frag_mask, const int64_t* slot_base,
                   int64_t capacity, const EposCorrOut* out, int32_t* overflow,
                   void* stream);

/* slot_base[s] = sum_{t<s} totals[t][1]; slot_base[S] = grand total. [device]
 * S >= 0 in all three correspondence calls; B, P, O >= 1; epos_corr_fill wants all seven
 * output arrays when capacity > 0 (EPOS_E_INVALID otherwise). */
int epos_corr_slot_bases(const int32_t* totals, int S, int64_t* slot_base,
                         void* stream);

/* Confidence order, truncation and row-order permutation of the pooled correspondences
 * (scripts/infer.py:425-440: PROSAC order / top max_correspondences by confidence), between
 * epos_corr_fill and the fitting call, all buffers [device], nothing synchronises or
 * allocates. With n_s = slot_base[s+1] - slot_base[s] (both bounds clamped to
 * [0, capacity]: after an overflow of epos_corr_fill nothing at or beyond capacity is read),
 * K = max_corr (<= 0: no limit), per slot:
 *   - the confidence order -- conf descending, ties by ascending original row -- applies
 *     iff always_sort != 0 or (K > 0 and n_s > K); otherwise the rows keep their order;
 *   - the first n'_s = (K > 0 ? min(n_s, K) : n_s) rows of that order are kept.
 * Outputs (N' = sum of n'_s <= capacity; size them for capacity rows):
 *   slot_base_out i64[S+1]  exclusive scan of n'_s
 *   coord_2d_out f64[N',2], coord_3d_out f64[N',3]  the kept rows, gathered
 *   src_row_out i32[N']     slot-local original row of every kept row
 *   yorder, ypos i32[N']    slot-local positions of the kept rows sorted by (coord_2d y
 *                           ascending, position ascending) -- the stable sort by y of
 *                           epos_find6d_poses -- and the inverse: the permutations
 *                           epos_find6d_poses_device_ordered takes (identities for a slot
 *                           that kept its order).
 * PRECONDITION: the rows of every slot come in raster order (coord_2d y non-decreasing), as
 * epos_corr_fill writes them: a kept row's y is ranked by a binary search over its slot's
 * original rows. px_id and W are not read (px_id, as epos_corr_fill writes it, counts the
 * MASKED pixels and does not give the image row); they stay in the signature.
 * work: epos_corr_order_workspace_bytes(S, capacity) bytes. capacity < 2^31.
 * epos_corr_order_tile_rows(): slots of at most that many rows are ordered by one workgroup
 * in LDS; longer ones by merge passes in global memory on top (same result either way; the
 * passes that no slot of the call is long enough for leave at once). */
int epos_corr_order_tile_rows(void);
int64_t epos_corr_order_workspace_bytes(int S, int64_t capacity);
int epos_corr_order_by_conf(const float* conf, const int64_t* px_id, const double* coord_2d,
                            const double* coord_3d, const int64_t* slot_base, int S,
                            int64_t capacity, int W, int64_t max_corr, int always_sort,
                            void* work, int64_t* slot_base_out, double* coord_2d_out,
                            double* coord_3d_out, int32_t* src_row_out, int32_t* yorder,
                            int32_t* ypos, void* stream);

/* project_to_surface (corresp.py:87-88, datagen.py:128-154: igl::AABB::squared_distance):
 * out[i] = the point of the triangle mesh (verts [nv,3] f64, faces [nf,3] int32, all
 * device) closest to pts[i] ([n,3] f64); face_idx [n] int32 or NULL receives the face.
 * Exact sweep over all faces, ties -> lowest face index. */
int epos_project_to_mesh_f64(const double* pts, int64_t n, const double* verts,
                             int64_t nv, const int32_t* faces, int64_t nf, double* out,
                             int32_t* face_idx, void* stream);

/* project_to_surface inside the fused pipeline: the same closest points, bit for bit, for
 * the pooled rows of epos_corr_fill IN PLACE, through a mesh index built on the host
 * (epos_amd/mesh_index.py; DESIGN.md, "Mesh index"). All buffers [device], nothing
 * synchronises or allocates, the launch is sized from `capacity`.
 *
 * Index of one mesh: its faces in Morton order of their centroids, 64 to a leaf; level 0 of
 * the boxes bounds the leaves, node i of level l+1 covers nodes 64i .. 64i+63 of level l, the
 * top level has at most 64 nodes. Faces the pruning argument does not cover are kept out of
 * the tree, in `nalways` further blocks that every query sweeps.
 *   geom      f64: triangle blocks of 9 x 64 doubles ([k][lane], k = ax ay az bx .. cz), the
 *                  nleaf tree leaves first, then the always-swept blocks; box groups of
 *                  6 x 64 doubles ([k][lane], k = lo xyz, hi xyz), one group per parent
 *   face_ids  i32: 64 per triangle block, the ORIGINAL face index, -1 = empty place
 * recs[obj_id - 1], num_objs of them; nf == 0 = no mesh (rows of such a slot stay as they
 * are; the Python layer refuses them before the launch). */
typedef struct EposMeshRec {
  int64_t tri_off;          /* geom offset (doubles) of the triangle blocks           */
  int64_t fid_off;          /* face_ids offset of the same blocks                     */
  int64_t box_off[4];       /* geom offset (doubles) of the box groups of level l     */
  int32_t count[4];         /* nodes of level l (count[0] = nleaf)                    */
  int32_t nf, nleaf, nalways, top;   /* faces, tree leaves, always blocks, top level  */
  double near_lo[3], near_hi[3];     /* queries outside this box sweep every leaf     */
} EposMeshRec;
/* Rows r < min(slot_base[S], capacity) of coord_3d f64[N,3]; row r belongs to the slot s with
 * slot_base[s] <= r < slot_base[s+1] and is replaced by the closest point of the mesh of
 * slots[s].obj_id -- what epos_project_to_mesh_f64 returns for it (ties -> lowest original
 * face index; no finite distance -> (0,0,0), face nf). face_idx i32[N] or NULL: the face;
 * visited i32[N] or NULL: triangle blocks swept for the row (tests observe the pruning). */
int epos_project_rows_to_mesh_f64(double* coord_3d, const int64_t* slot_base,
                                  const EposCorrSlot* slots, int S, int64_t capacity,
                                  const EposMeshRec* recs, int num_objs, const double* geom,
                                  const int32_t* face_ids, int32_t* face_idx,
                                  int32_t* visited, void* stream);

/* ------------------------------------------------------------------------- *
 * Model preprocessing (replaces epos_lib/fragment.py:8-54, fragmentation_fps,
 * called once per object by ObjectModelStore.fragment_models, datagen.py:86-126).
 * vertices f64[V,3] [device]; outputs [device]: centers f64[F,3] (the FPS picks, in
 * order), center_idx i32[F] (their vertex indices), vertex_frag_ids i32[V] (nearest
 * centre of every vertex); nn_dist f64[V] is scratch. Bit-identical to the
 * reference (fp64, same operation order, lowest-index tie rule).
 * ------------------------------------------------------------------------- */
int epos_fragmentation_fps(const double* vertices, int64_t V, int num_frags,
                           double* nn_dist, double* centers, int32_t* center_idx,
                           int32_t* vertex_frag_ids, void* stream);

/* ------------------------------------------------------------------------- *
 * Pose fitting (replaces pyprogressivex.find6DPoses, scripts/infer.py:470-488;
 * the un-vendored danini/progressive-x pybind11 module).
 * ------------------------------------------------------------------------- */
typedef struct EposFitParams {
  double threshold;                 /* inlier_thresh, tau_r [px]   (infer.py:76-79)  */
  double neighborhood_ball_radius;  /* neighbour_max_dist, tau_d: two correspondences
                                     * are neighbours iff their distance in
                                     * (x, y, s X, s Y, s Z) is <= tau_d (infer.py:80-82) */
  double spatial_coherence_weight;  /* lambda of GC-RANSAC's labelling energy (0 = off) */
  double scaling_from_millimeters;  /* s above (0.1: mm -> cm, infer.py:106-110)     */
  double max_tanimoto_similarity;   /* infer.py:112-114                              */
  double conf;                      /* required_progx_confidence: a failed proposal of a
                                     * multi-instance search is retried until the samples
                                     * drawn reach this confidence (max two extra rounds) */
  double proposal_engine_conf;      /* required_ransac_confidence: RANSAC stops once
                                     * (1 - w^3)^it <= 1 - this (1.0 = always max_iters) */
  double min_coverage;              /* min_hypothesis_quality, tau_q                 */
  double min_triangle_area;         /* tau_t                                         */
  int32_t max_iters;                /* max_fitting_iterations (400)                  */
  int32_t min_point_number;         /* 6 (infer.py:483)                              */
  int32_t max_model_number;         /* num_instances; -1 = as many as found          */
  int32_t max_model_number_for_optimization;  /* joint refinement only up to this many
                                     * instances (max_model_number_for_pearl)        */
  int32_t use_prosac;               /* sample from a growing confidence-sorted prefix */
  int32_t lo_iters;                 /* Gauss-Newton refits per local-optimisation stage (8) */
  int32_t gc_sweeps;                /* relabelling sweeps of the spatial-coherence step
                                     * (default 2; 0 = thresholded inliers only)     */
  int32_t pearl_iters;              /* joint refinement iterations of multi-instance
                                     * results (default 2; 0 = off)                  */
} EposFitParams;
void epos_fit_params_default(EposFitParams* p);

/* Host-pointer drop-in for pyprogressivex.find6DPoses: xy f64[n,2] (pixels),
 * xyz f64[n,3] (mm), K f64[9] row-major. Outputs (caller-owned):
 *   poses  f64[max_k*12]: instance j occupies poses[12*j .. 12*j+11] as
 *          R row-major in [0..8] (R[r][c] = poses[12*j + 3*r + c]) followed by
 *          t in [9..11] -- NOT a row-major 3x4 [R|t]: reading the 12 doubles as a 3x4
 *          matrix gives wrong poses. (The reference's module returns the instances
 *          stacked as a [3k,4] array which infer.py:490-495 slices into R, t; the binding
 *          in INTEGRATION.md rebuilds exactly that from this layout.)
 *   labels i32[n] (instance index or -1), scores f64[max_k].
 * Returns k >= 0 (0 <=> the reference's `pose_ests is None`) or < 0. */
int epos_find6d_poses(const double* xy, const double* xyz, int64_t n,
                      const double* K, const EposFitParams* p, uint64_t seed,
                      double* poses_out, int32_t* labels_out, double* scores_out,
                      int32_t max_k);

/* Batched device entry: S independent fitting problems (slots) in one call, all
 * buffers [device], nothing synchronises.
 *   xy f64[N,2], xyz f64[N,3] pooled; slot s owns rows [slot_base[s], slot_base[s+1])
 *   Ks f64[S,9]; max_models i32[S] (per-slot num_instances, <= max_k)
 *   seeds u64[S]
 *   work: scratch of epos_fit_workspace_bytes(S, N_capacity, p) bytes
 * Outputs: poses f64[S,max_k,12] (per instance: R row-major [0..8], then t [9..11], as
 *          above), scores f64[S,max_k], num_models i32[S], labels i32[N] (instance index
 *          within the slot or -1). num_models[s] == -1: a device-side consistency check
 *          failed for that slot (a hand-off between the workgroups that fit it together
 *          timed out); its outputs are not valid and the call should be repeated --
 *          epos_find6d_poses returns EPOS_E_INTERNAL in that case.
 * PRECONDITION (not checked): the rows of every slot are in image-row order --
 * xy[.,1] non-decreasing within [slot_base[s], slot_base[s+1]) -- which is the raster order
 * epos_corr_fill writes. The spatial-coherence sweeps and the joint refinement find a
 * point's neighbours in a window of rows around it and stop at the first row farther than
 * neighborhood_ball_radius: with unsorted rows neighbourhoods are silently truncated and
 * the poses change. Callers with arbitrary row order use
 * epos_find6d_poses_device_ordered below, which lifts this requirement (it takes the
 * row-order permutation as an argument), or epos_find6d_poses (it sorts internally and
 * keeps the caller's order for PROSAC), or sort first; with
 * spatial_coherence_weight == 0 (or gc_sweeps == 0) and max_k == 1 no order is needed. */
int64_t epos_fit_workspace_bytes(int S, int64_t n_capacity, const EposFitParams* p,
                                 int32_t max_k);
int epos_find6d_poses_device(const double* xy, const double* xyz,
                             const int64_t* slot_base, int S, int64_t n_capacity,
                             const double* Ks, const int32_t* max_models,
                             const uint64_t* seeds, const EposFitParams* p,
                             int32_t max_k, void* work, double* poses,
                             double* scores, int32_t* num_models, int32_t* labels,
                             void* stream);

/* The same call for rows in the CALLER's order (use_prosac samples from a growing prefix of
 * it -- e.g. the confidence order of epos_corr_order_by_conf). yorder i32[N] [device]:
 * per slot, the slot-local row indices sorted by (xy[.,1] ascending, index ascending);
 * ypos i32[N]: its inverse (ypos[slot_base[s] + yorder[slot_base[s] + i]] = i). The
 * neighbourhood windows walk the rows through them. Both null = epos_find6d_poses_device
 * (and its precondition); exactly one null: EPOS_E_INVALID. */
int epos_find6d_poses_device_ordered(const double* xy, const double* xyz,
                                     const int64_t* slot_base, int S, int64_t n_capacity,
                                     const double* Ks, const int32_t* max_models,
                                     const uint64_t* seeds, const EposFitParams* p,
                                     int32_t max_k, void* work, double* poses,
                                     double* scores, int32_t* num_models, int32_t* labels,
                                     void* stream, const int32_t* yorder,
                                     const int32_t* ypos);

/* ------------------------------------------------------------------------- *
 * The OpenCV fitting method (replaces cv2.solvePnPRansac(objectPoints, imagePoints, K,
 * None, iterationsCount, reprojectionError, confidence=0.99, flags=cv2.SOLVEPNP_EPNP),
 * scripts/infer.py:505-528; OpenCV 3.4.2, README.md:29, is not vendored).
 * What is computed (the published behaviour of that call, restated):
 *   - points are rounded to float32 on entry; minimal sets of 5 correspondences drawn by
 *     cv::RNG (state 2^64 - 1, `next() % n`, repeated indices re-drawn);
 *   - EPnP (Lepetit et al., IJCV 2009) on each set -> one pose; its inliers: squared
 *     reprojection error, float32 arithmetic on the float32 projection, <= (float)err^2;
 *   - a set with strictly more inliers than the best so far (and > 4) becomes the best and
 *     the iteration cap becomes round(log(1 - confidence) / log(1 - w^5));
 *   - EPnP once more over ALL inliers of the best set: that pose is returned.
 * Own factorisations (cyclic Jacobi, Householder QR) instead of cv::SVD: poses agree with
 * an LAPACK-based statement of EPnP to ~1e-9, not bit for bit with OpenCV -- unpinned.
 * ------------------------------------------------------------------------- */
typedef struct EposPnpRansacParams {
  int32_t iterations_count;     /* max_fitting_iterations (400)       infer.py:515 */
  int32_t min_point_number;     /* slots / calls with fewer correspondences give no pose:
                                 * 6 in the script (infer.py:420-422 skips them before the
                                 * call); 0 = OpenCV's own rule (n >= 5)                */
  double reprojection_error;    /* inlier_thresh (4.0 px)             infer.py:516 */
  double confidence;            /* 0.99                               infer.py:517 */
} EposPnpRansacParams;
void epos_pnp_ransac_params_default(EposPnpRansacParams* p);

/* Host-pointer drop-in: xy f64[n,2] (imagePoints), xyz f64[n,3] (objectPoints), K f64[9]
 * row-major (fx, fy, cx, cy are used, as by OpenCV without distortion). Outputs
 * (caller-owned): pose_out f64[12] = R row-major in [0..8], then t in [9..11] (the layout of
 * epos_find6d_poses, NOT a row-major 3x4; R = Rodrigues(rvec) of the
 * reference), inlier_mask_out u8[n], info_out i32[4] or NULL = {index of the winning set,
 * its inlier count, the final iteration cap, sets evaluated}. Returns 1 (pose found),
 * 0 (`pose_est_success` false) or < 0. */
int epos_solve_pnp_ransac(const double* xy, const double* xyz, int64_t n, const double* K,
                          const EposPnpRansacParams* p, double* pose_out,
                          uint8_t* inlier_mask_out, int32_t* info_out);

/* Batched device entry (slots as for epos_find6d_poses_device), all buffers [device]:
 * poses f64[S,12] (R row-major [0..8], t [9..11]), success i32[S], inlier_mask u8[N],
 * info i32[S,4] or NULL;
 * work = epos_pnp_ransac_workspace_bytes(S, N_capacity, p) bytes. Nothing synchronises. */
int64_t epos_pnp_ransac_workspace_bytes(int S, int64_t n_capacity,
                                        const EposPnpRansacParams* p);
int epos_solve_pnp_ransac_device(const double* xy, const double* xyz,
                                 const int64_t* slot_base, int S, int64_t n_capacity,
                                 const double* Ks, const EposPnpRansacParams* p, void* work,
                                 double* poses, int32_t* success, uint8_t* inlier_mask,
                                 int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------
 * bf16 inference mode (EposNet(precision='bf16')). Activations are stored as bf16 (the top
 * 16 bits of an IEEE fp32, rounded to nearest even); products are bf16 x bf16 on the matrix
 * cores with fp32 accumulation; every epilogue (bias, residual, ReLU) runs in fp32 and rounds
 * once when it stores. Pointers typed uint16_t hold bf16 bit patterns.
 * --------------------------------------------------------------------------------------- */

/* Folded 1x1 weights W [K][N] (fp32, row-major) -> bf16 (RNE) in the layout of
 * epos_pointwise_conv_bf16: dst[((k / 8) * Npad + n) * 8 + k % 8] for k < round_up(K, 32),
 * n < Npad = round_up(N, 128), zero outside [K) x [N). Returns the element count
 * (round_up(K, 32) * Npad); dst == NULL only queries it. K, N >= 1. */
int64_t epos_pack_pointwise_weights_bf16(const float* W, int K, int N, uint16_t* dst);

/* C[m, n] = act(sum_{k<K} A[row(m), k] * W[k, n] + bias[n] (+ R[m, n])), bf16 x bf16 products,
 * fp32 accumulation and epilogue, ReLU last. A [device]: bf16 rows of lda elements (only
 * columns < K are read); row(m) as in EposPointwiseArgs (sub > 1: 1x1 stride-`sub` conv of a
 * [B, Hi, Wi] map, M = B*Ho*Wo). Wp: epos_pack_pointwise_weights_bf16; bias: N floats or
 * NULL; R: optional bf16 residual rows of ldr elements; C: rows of ldc elements, bf16
 * (c_f32 == 0, rounded to nearest even) or fp32 (c_f32 != 0; c_stream != 0: non-temporal
 * stores). K % 8 == 0, lda % 8 == 0, lda >= K, A 16-byte aligned. */
typedef struct EposPointwiseBf16Args {
  const uint16_t* A; int64_t lda;
  const uint16_t* Wp; const float* bias;
  const uint16_t* R; int64_t ldr;
  void* C; int64_t ldc;
  int32_t M, N, K;
  int32_t relu;
  int32_t sub;
  int32_t Ho, Wo, Hi, Wi;   /* only read when sub > 1 */
  int32_t c_f32;
  int32_t c_stream;
} EposPointwiseBf16Args;
/* 1..8 independent problems in one launch. */
int epos_pointwise_conv_bf16(const EposPointwiseBf16Args* args, int count, void* stream);

/* Depthwise 3x3 with the semantics of epos_depthwise3x3_f32 (stride 1 SAME with `rate`;
 * stride 2 fixed_padding + VALID; relu_in / relu_out) on bf16 X / Y: fp32 folded weights
 * w9c [9][C] and bias [C], fp32 math, one RNE rounding per output.
 * C, ldx, ldy multiples of 8; X, Y, w9c, bias 16-byte aligned. */
typedef struct EposDepthwiseBf16Args {
  const uint16_t* X; int64_t ldx;
  const float* w9c; const float* bias;
  uint16_t* Y; int64_t ldy;
  int32_t B, Hi, Wi, Ho, Wo, C;
  int32_t stride, rate;
  int32_t relu_in, relu_out;
} EposDepthwiseBf16Args;
int epos_depthwise3x3_bf16(const EposDepthwiseBf16Args* args, void* stream);

/* k x k im2col into bf16 columns: col[m, (ky*k+kx)*C + c] = bf16(pre(X[...])) as in
 * epos_im2col_f32, zero for padded taps and for the columns k*k*C .. ldcol. X is the fp32
 * image (x_bf16 == 0, with the three preprocess modes) or a bf16 activation (x_bf16 != 0,
 * preprocess must be EPOS_PREPROCESS_NONE). ldcol % 8 == 0, col 16-byte aligned. */
typedef struct EposIm2colBf16Args {
  const void* X; int64_t ldx;
  int32_t x_bf16;
  int32_t reserved0;
  uint16_t* col; int64_t ldcol;
  int32_t B, Hi, Wi, Ho, Wo, C;
  int32_t k, stride, rate, pad;
  int32_t preprocess;
  float mean_rgb[3];
} EposIm2colBf16Args;
int epos_im2col_bf16(const EposIm2colBf16Args* args, void* stream);

/* The glue layers of the bf16 plan: the fp32 kernels' semantics on bf16 tensors (fp32 math,
 * one RNE rounding per stored value). C, ld* multiples of 8 and 16-byte aligned rows. */
/* Bilinear resize, align_corners=True; X is bf16, or fp32 when x_f32 != 0 (the image-pooling
 * broadcast from its fp32 1x1 output). */
int epos_resize_bilinear_bf16(const void* X, int64_t ldx, int x_f32, uint16_t* Y,
                              int64_t ldy, int B, int Hi, int Wi, int Ho, int Wo, int C,
                              void* stream);
/* Global mean over H*W into fp32: X [B, HW, C] (ldx) -> Y [B, C]. */
int epos_global_avg_pool_bf16(const uint16_t* X, int64_t ldx, float* Y, int B, int HW, int C,
                              void* stream);
int epos_maxpool3x3_s2_bf16(const uint16_t* X, int64_t ldx, uint16_t* Y, int64_t ldy,
                            int B, int Hi, int Wi, int C, void* stream);
int epos_subsample_bf16(const uint16_t* X, int64_t ldx, uint16_t* Y, int64_t ldy, int B,
                        int Hi, int Wi, int C, int factor, void* stream);
/* Y = relu(A + B) over n contiguous bf16 values, n % 8 == 0. */
int epos_add_relu_bf16(const uint16_t* A, const uint16_t* B, uint16_t* Y, int64_t n,
                       void* stream);

/* ------------------------------------------------------------------------- *
 * Multi-scale inference (image_pyramid + merge_method, model.py:515-626; added
 * without an ABI version change: nothing existing moved).
 * ------------------------------------------------------------------------- */
#define EPOS_MERGE_MAX 0    /* merge_method 'max': reduce_max over the scales */
#define EPOS_MERGE_MEAN 1   /* merge_method 'avg': reduce_mean (sum in source order, then / S) */
typedef struct EposResizeSrc {
  const float* X;   /* [device] [B, Hi, Wi, C] with row pitch ldx >= C */
  int64_t ldx;
  int32_t Hi, Wi;   /* >= 1 */
} EposResizeSrc;
/* Y[b,y,x,c] = merge over s of resize_bilinear_align_corners(X_s)[b,y,x,c] (misc.py:94-107,
 * TF's arithmetic: scale = (in-1)/(out-1) as a float, lo = floor(o*scale),
 * hi = min(ceil(o*scale), in-1), top = tl + (tr-tl)*lx, top + (bot-top)*ly, no FMA). srcs is a
 * HOST array of S sources (1 <= S <= 8); Y [B, Ho, Wo, C] with ldy >= C; any C >= 1. S = 1 is
 * a plain resize (a same-size source is an exact copy). merge: EPOS_MERGE_MAX | _MEAN. Vector
 * accesses where every pitch and base pointer allows them. */
int epos_resize_merge_f32(const EposResizeSrc* srcs, int S, float* Y, int64_t ldy, int B,
                          int Ho, int Wo, int C, int merge, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh renderer (csrc/render.hip; added without an ABI version change: nothing
 * existing moved). A batched z-buffered triangle rasteriser and the ground-truth
 * maps built from its images. The three launchers only enqueue on `stream`: no host
 * synchronisation, no allocation. tests/helpers/render_ref.py restates every rule
 * below in numpy; the kernels equal it bit for bit.
 *
 * Geometry (a defined function of the input, not of the launch):
 *   camera-space vertex   Xc = R X + t, fp64, each row summed left to right, no FMA
 *   projection            u = fx Xc / Zc + cx, v = fy Yc / Zc + cy
 *   sample point          pixel (x, y) is sampled at image coordinates (x + .5, y + .5)
 *   near rule             a triangle with any vertex at Zc < near is dropped whole --
 *                         there is NO clipping: a surface that crosses the near plane
 *                         loses every triangle that touches it
 *   snapping              rint(u * 256), rint(v * 256) as int64 (1/256 pixel); a triangle
 *                         with any |snapped coordinate| >= 2^31 is dropped
 *   coverage              exact integer edge functions (64-bit while every |coordinate|
 *                         < 2^29, 128-bit above: both exact), top-left fill rule; a shared
 *                         edge gives its two triangles negated values, so a closed mesh has
 *                         neither cracks nor double hits; both windings are drawn;
 *                         zero-area triangles cover nothing
 *   depth                 b_i = E_i / (E_0 + E_1 + E_2) in fp64 (E_i the edge value opposite
 *                         vertex i; a 128-bit value converts as high half * 2^64 + low
 *                         half), z = 1 / (b_0/z_0 + b_1/z_1 + b_2/z_2), rounded once to fp32
 *   key                   (fp32 bits of z) << 32 | face index within the instance, combined
 *                         by a 64-bit unsigned atomic min: the nearest surface wins, equal
 *                         fp32 depth goes to the lowest face index, in every launch order
 * The sample point, the near rule and the shading are this build's definitions
 * (bop_renderer is not available to compare with): parity unpinned.
 * ------------------------------------------------------------------------- */
typedef struct EposRenderInst {
  int32_t vert_base;   /* first vertex of the instance's mesh in the pooled arrays */
  int32_t face_base;   /* first face; its vertex indices are relative to vert_base */
  int32_t n_faces;
  int32_t reserved0;
  double R[9];         /* row-major rotation, model -> camera */
  double t[3];         /* translation, mm */
  double fx, fy, cx, cy;
} EposRenderInst;
/* Bounding-box sample count above which a triangle is walked by its whole wavefront instead
 * of by one lane (the result does not depend on it). */
int epos_render_lane_max_pixels(void);
/* verts f64 [n_verts,3], faces i32 [n_faces,3] (pooled), insts [n_inst] -- all [device].
 * keys u64 [n_inst,h,w] is cleared to all ones on the stream, then rasterised into. near > 0
 * (mm). Faces or vertices outside the pooled arrays are skipped. h, w <= 32768 and
 * n_inst * h * w < 2^31 (here and in the resolve call); every refusal comes before the first
 * launch. */
int epos_render_raster(const double* verts, int64_t n_verts, const int32_t* faces,
                       int64_t n_faces, const EposRenderInst* insts, int n_inst, int h, int w,
                       double near, uint64_t* keys, void* stream);
/* Keys -> images, each output optional (NULL skips it), [device]:
 *   depth f32 [n_inst,h,w]        camera z in mm, 0 = background
 *   face i32 [n_inst,h,w]         winning face within the instance, -1 = background
 *   local_pos f32 [n_inst,h,w,3]  perspective-correct model-space position:
 *                                 (sum_i q_i X_i) / (sum_i q_i), q_i = b_i / z_i, 0 = background
 *   color u8 [n_inst,h,w,3]       the same interpolation of the vertex colours (colors u8
 *                                 [n_verts,3], required with this output), times the headlight
 *                                 term L = 0.3 + 0.7 nz^2 / (nx^2 + ny^2 + nz^2), n = (P1 - P0)
 *                                 x (P2 - P0) in camera space (L = 0.3 when n = 0); stored as
 *                                 floor(c L + 0.5) clamped to 0..255
 * The barycentrics are recomputed from the winning face exactly as in the raster pass; same
 * verts / faces / insts / near as the raster call. */
int epos_render_resolve(const uint64_t* keys, const double* verts, int64_t n_verts,
                        const int32_t* faces, int64_t n_faces, const uint8_t* colors,
                        const EposRenderInst* insts, int n_inst, int h, int w, double near,
                        float* depth, int32_t* face, float* local_pos, uint8_t* color,
                        void* stream);
/* Ground-truth maps of one image from per-instance renderings (datagen.py:570-604,
 * datagen_utils.py:161-232, knn_frags = 1). depth f32 [n_inst,h,w], local_pos f32
 * [n_inst,h,w,3], masks u8 [n_inst,h,w] or NULL, obj_ids i32 [n_inst] (1-based; an instance
 * whose id is outside 1..num_objs takes no pixel), centers f64 [num_objs,num_frags,3], sizes
 * f64 [num_objs,num_frags], 1 <= num_frags <= 256 (EPOS_E_INVALID otherwise).
 * Visibility: with masks, the instances are scanned from the last to the first and a pixel goes
 * to the first one with mask != 0 and depth > 0; without, the nearest depth > 0 wins, ties to
 * the higher index. Outputs (each optional): obj_label i32 [h,w] (0 = none), instance i32
 * [h,w] (-1 = none), frag_label i32 [h,w] (nearest centre by dx^2 + dy^2 + dz^2 summed in
 * that order in fp64, ties to the lowest index), frag_loc f32 [h,w,3] = (xyz - centre) / size
 * in fp64 on the fp32 xyz, rounded to fp32, frag_weight f32 [h,w] (1 where assigned). */
int epos_gt_fields(const float* depth, const float* local_pos, const uint8_t* masks,
                   const int32_t* obj_ids, int n_inst, int h, int w, const double* centers,
                   const double* sizes, int num_objs, int num_frags, int32_t* obj_label,
                   int32_t* instance, int32_t* frag_label, float* frag_loc,
                   float* frag_weight, void* stream);

/* ------------------------------------------------------------------------- *
 * Evaluation (csrc/eval.hip; added without an ABI version change: nothing existing
 * moved). Integer reductions over label maps; both launchers only enqueue on
 * `stream` and ADD into their tables, which they never clear: the caller zeroes a
 * table once per evaluation and accumulates over every batch. All sums are integer,
 * so the tables do not depend on the launch; tests/helpers/eval_ref.py restates
 * them in numpy and the kernels equal it exactly. Every refusal (EPOS_E_INVALID)
 * comes before the first launch; P == 0 does nothing and returns 0.
 * ------------------------------------------------------------------------- */
/* Largest num_cls whose confusion matrix a workgroup keeps privately in LDS (32-bit counters,
 * flushed with one 64-bit atomic per non-zero cell); above it the pixels go to the global table
 * directly. The result does not depend on it. */
int epos_eval_lds_max_cls(void);
/* Confusion matrix of eval_utils.py:52-87: gt_label i32 [P], pred_label i64 [P] (P = B*h*w,
 * 0 <= P <= 2^40), cm i64 [num_cls,num_cls] with row = ground truth, column = prediction,
 * bad i64 [1], all [device]. A pixel whose ground truth equals ignore_label is skipped (this
 * rule comes first, also for an ignore_label inside 0..num_cls-1). Any other pixel whose ground
 * truth or prediction lies outside 0..num_cls-1 adds 1 to *bad and nothing to cm (the reference
 * would raise IndexError there). 1 <= num_cls <= 256. */
int epos_eval_confusion(const int32_t* gt_label, const int64_t* pred_label, int64_t P,
                        int num_cls, int ignore_label, int64_t* cm, int64_t* bad, void* stream);
/* Fragment hit counts. THIS BUILD'S DEFINITION: the reference evaluates the object
 * segmentation only (its hook lists the fragment tensors commented out) and defines no
 * fragment metric. gt_obj_label, gt_frag_label i32 [P]; pred_obj_label i64 [P] or NULL;
 * pred_frag_conf f32 [P,num_objs,num_frags] (the dense head); counts i64 [num_objs+1,3]; all
 * [device]. For every pixel p whose ground-truth object o lies in 1..num_objs (0, ignore_label
 * and ids outside that range are skipped and read no confidence):
 *   f* = argmax_f pred_frag_conf[p,o-1,f], the first maximum wins; a NaN compares as -inf, so
 *        it never beats a number (a row without any number gives f* = 0)
 *   counts[o,0] += 1
 *   counts[o,1] += (f* == gt_frag_label[p])
 *   counts[o,2] += (f* == gt_frag_label[p] && pred_obj_label[p] == o)   (untouched when
 *                  pred_obj_label is NULL)
 * Row 0 stays as it was. 1 <= num_objs <= 4095, 1 <= num_frags <= 256. */
int epos_eval_frag_hits(const int32_t* gt_obj_label, const int32_t* gt_frag_label,
                        const int64_t* pred_obj_label, const float* pred_frag_conf, int64_t P,
                        int num_objs, int num_frags, int ignore_label, int64_t* counts,
                        void* stream);

/* ------------------------------------------------------------------------- *
 * Pose errors (csrc/pose_error.hip; added without an ABI version change: nothing
 * existing moved). MSSD, MSPD, ADD and ADI of (estimate, ground truth) pairs over
 * pooled model vertices and pooled symmetry sets. The launcher only enqueues on
 * `stream`: no host synchronisation, no allocation. tests/helpers/pose_error_ref.py
 * restates every rule below in element-wise numpy; the kernels equal it bit for bit.
 *
 * These are THIS BUILD'S DEFINITIONS. They follow the published BOP'19 formulas
 * (Hodan et al., "BOP Challenge 2020 on 6D Object Localization", section 2.2; Hinterstoisser
 * et al. 2012 for ADD / ADI), but bop_toolkit is not available to compare with: parity with
 * its numbers is unpinned.
 *
 * Arithmetic: fp64 throughout, built from + - * / sqrt only, no FMA. Every 3-term sum is
 * taken left to right and a translation is added last. A result is a function of the input
 * and never of the launch shape. Inputs are finite and of a size at which nothing overflows
 * (the caller keeps non-finite poses away: epos_amd/pose_error.py gives them +inf).
 *
 * A symmetry is 12 numbers: R_s row-major, then t_s (mm). The set of an object is built on
 * the host (epos_amd/pose_error.py: symmetry_transformations): the discrete part D =
 * [identity] + symmetries_discrete; the continuous part C = rotations by i * 2 pi / n about
 * `axis` through `offset`, i = 0..n-1, n = ceil(pi / max_sym_disc_step), max_sym_disc_step =
 * 0.01, t = offset - R offset; the set is every c o d (c outer, d inner), or D alone without
 * a continuous part. The identity is element 0. Including i = 0 is deliberate: the set then
 * holds the discrete symmetries themselves (the step, not the count, is what bounds the
 * discretisation error).
 *
 * For a pair (R_e, t_e; R_g, t_g; fx, fy, cx, cy) with vertices X_v and symmetries s:
 *   composition  R' = R_g R_s (each element (a0 b0 + a1 b1) + a2 b2),
 *                t' = ((R_g t_s, summed the same way) + t_g), composed FIRST; then
 *                G_sv = R' X_v + t', E_v = R_e X_v + t_e, each row ((r0 x + r1 y) + r2 z) + t
 *   MSSD         min_s max_v |E_v - G_sv|: max and min run over the squared norms
 *                (dx^2 + dy^2) + dz^2 and one sqrt is taken at the end (sqrt is monotone)
 *   MSPD         the same with u = (fx X) / Z + cx, v = (fy Y) / Z + cy and du^2 + dv^2; a
 *                point whose estimate-side or ground-truth-side Z <= 0 contributes +inf
 *   ADD          (sum_v |E_v - G_0v|) / n_verts, G_0 composed with element 0 of the set
 *   ADI          (sum_v sqrt(min_w |E_w - G_0v|^2)) / n_verts
 *   sum shape    p_j, j = 0..255, is the left-to-right sum of the terms with v = j (mod 256);
 *                then p_j += p_{j+128} for j < 128, the same with 64, ... 1; the total is p_0
 * ------------------------------------------------------------------------- */
typedef struct EposPosePair {
  int32_t vert_base;   /* first vertex of the object in the pooled vertices */
  int32_t n_verts;
  int32_t sym_base;    /* first symmetry of the object in the pooled symmetries */
  int32_t n_sym;
  double R_e[9];       /* estimate, row-major, model -> camera */
  double t_e[3];       /* mm */
  double R_g[9];       /* ground truth */
  double t_g[3];
  double fx, fy, cx, cy;
} EposPosePair;
/* Symmetries one workgroup of the MSSD / MSPD kernel owns (a set that is no multiple of it
 * ends in a partial group), and estimate-side points per LDS tile of the ADI kernel. The
 * results depend on neither. */
int epos_pose_error_group_syms(void);
int epos_pose_error_adi_tile(void);
/* verts f64 [n_verts_total,3], syms f64 [n_syms_total,12], err f64 [n_pairs,4] = (mssd,
 * mspd, add, adi), pairs_dev [n_pairs]: all [device]. pairs [n_pairs] is a HOST table: it is
 * checked here and copied into pairs_dev on the stream, so it stays alive and unchanged until
 * the stream has passed this call (pinned memory keeps the copy asynchronous). want_adi = 0
 * leaves column 3 as it was (ADI is O(n_verts^2) per pair). Refused with EPOS_E_INVALID
 * before the copy and the first launch: a pair with n_verts < 1 or n_sym < 1, a base or a
 * range outside the pools, n_pairs < 0, a null pointer, n_pairs * ceil(max n_sym /
 * epos_pose_error_group_syms()) >= 2^31. n_pairs == 0 does nothing and returns 0. */
int epos_pose_errors_f64(const double* verts, int64_t n_verts_total, const double* syms,
                         int64_t n_syms_total, const EposPosePair* pairs,
                         EposPosePair* pairs_dev, int n_pairs, int want_adi, double* err,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * VSD (csrc/vsd.hip; added without an ABI version change: nothing existing moved). The
 * pixel counts of BOP'19's Visible Surface Discrepancy for (ground truth, estimate) pairs,
 * from a test depth image and the depth renderings of the two poses (epos_render_*: camera z
 * in mm, 0 = background). The launcher only enqueues on `stream`: no host synchronisation,
 * no allocation. tests/helpers/vsd_ref.py restates every rule below in element-wise numpy;
 * the kernel equals it exactly.
 *
 * These are THIS BUILD'S DEFINITIONS. They follow the published BOP'19 formulas (Hodan et
 * al., "BOP Challenge 2020 on 6D Object Localization", section 2.2, and "On Evaluation of 6D
 * Object Pose Estimation", 2016, for the visibility masks), but bop_toolkit is not available
 * to compare with: parity with its numbers is unpinned. In particular the ray of a pixel goes
 * through x + .5, y + .5, the sample point of this build's renderer, which is not necessarily
 * bop_toolkit's.
 *
 * Per pixel (x, y) of the pair's window, fp64 throughout, built from + - * / sqrt only, no
 * FMA, in this order:
 *   zt = depth_test[image,y,x]; missing = !(zt > 0)       (0, negative, NaN: no measurement)
 *   zg = depth_model[gt_inst,y,x]; ze = est_inst < 0 ? 0 : depth_model[est_inst,y,x]
 *   rx = ((x + 0.5) - cx) / fx; ry = ((y + 0.5) - cy) / fy; s = sqrt((rx*rx + ry*ry) + 1.0)
 *   dt = zt * s; dg = zg * s; de = ze * s                 (distances along the pixel's ray)
 *   mask_g = zg > 0; mask_e = ze > 0
 *   vis_g = mask_g && (missing || dg - dt <= delta)       ('bop19' rule: missing depth is
 *                                                          visible)
 *   vis_e = mask_e && (missing || de - dt <= delta || vis_g)
 *   inter = vis_g && vis_e; uni = vis_g || vis_e
 *   for inter pixels: d = fabs(dg - de) / diameter; ge[k] += (d >= taus[k])
 * counts row = [#mask_g, #vis_g, #mask_e, #vis_e, #inter, #uni, ge[0..n_taus-1]].
 * The host turns a row into VSD(tau_k) = (ge[k] + (#uni - #inter)) / #uni (1 where #uni = 0)
 * and the visible fraction #vis_g / #mask_g (epos_amd/vsd.py). Every output is an integer
 * count: a result is a function of the input alone, never of the launch shape, of
 * epos_vsd_row_bands() or of the order in which partial sums arrive.
 * ------------------------------------------------------------------------- */
typedef struct EposVsdPair {
  int32_t image;      /* index into depth_test */
  int32_t gt_inst;    /* index into depth_model */
  int32_t est_inst;   /* index into depth_model, or -1: no estimate (an all-background image) */
  int32_t x0, y0, x1, y1;   /* pixel window, x0 <= x < x1, y0 <= y < y1 */
  int32_t reserved0;
  double fx, fy, cx, cy;
  double diameter;    /* mm, > 0 */
} EposVsdPair;          /* 72 bytes */
/* The most taus one call takes (16), and the number of rows of a window that are walked side
 * by side (workgroups per pair x wavefronts per workgroup; row r of a window belongs to
 * wavefront r mod this). The results depend on neither. */
int epos_vsd_max_taus(void);
int epos_vsd_row_bands(void);
/* depth_test f32 [n_images,h,w], depth_model f32 [n_inst,h,w], pairs_dev [n_pairs], counts i64
 * [n_pairs, 6 + n_taus]: all [device]. pairs [n_pairs] and taus [n_taus] are HOST arrays: the
 * table is checked here and copied into pairs_dev on the stream, so it stays alive and
 * unchanged until the stream has passed this call (pinned memory keeps the copy asynchronous);
 * taus is read before the call returns. Every counter of every pair is WRITTEN: the launcher
 * clears them on the stream before the kernel adds into them. Pixels outside a pair's window
 * are not looked at, so a window must contain both renderings (epos_amd/vsd.py: window).
 * Refused with EPOS_E_INVALID before the copy and the first launch: image outside
 * [0, n_images), gt_inst outside [0, n_inst), est_inst outside [0, n_inst) and not -1, a
 * window not inside [0, w] x [0, h] or with x1 < x0 or y1 < y0, a diameter that is not finite
 * and > 0, fx or fy zero or not finite, n_taus outside 1..epos_vsd_max_taus(), a non-finite
 * delta, n_pairs < 0, n_inst * h * w >= 2^31, a null pointer. n_pairs == 0 does nothing and
 * returns 0. */
int epos_vsd_counts(const float* depth_test, int n_images, const float* depth_model, int n_inst,
                    int h, int w, const EposVsdPair* pairs, EposVsdPair* pairs_dev, int n_pairs,
                    double delta, const double* taus, int n_taus, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------- *
 * Losses (csrc/loss.hip; added without an ABI version change: nothing existing moved). The
 * three training losses of epos_lib/loss.py:99-303 -- object cross-entropy, fragment
 * cross-entropy, fragment-localisation Huber loss -- as per-image, per-object sums taken from
 * the RAW LOGITS of the dense heads, for ground-truth fields with one assigned fragment per
 * pixel (epos_gt_fields, the reference's gt_knn_frags = 1). The launcher only enqueues on
 * `stream`: no allocation, no host synchronisation. tests/helpers/loss_ref.py restates every
 * rule below in element-wise numpy. Parity with TensorFlow's numbers is unpinned (DESIGN.md,
 * "Losses").
 *
 * Inputs, all [device], for B images of P = h*w pixels each (p runs over the B*P pixels):
 *   obj_logits f32, B*P rows of O+1 values with row stride ld_obj >= O+1;
 *   frag_logits f32 [B*P, O, F]; frag_loc f32 [B*P, O, F, 3] (the head buffers as EposNet lays
 *   them out); gt_obj i32 [B*P]; gt_frag i32 [B*P]; gt_loc f32 [B*P, 3]; gt_weight f32 [B*P];
 *   ignore_label. 1 <= O <= 4095, 1 <= F <= 256, 0 <= P <= 2^31.
 * Outputs, WRITTEN, not added, one row per image (the caller points them at rows of a larger
 * table): sums f64 [B, O+1, 3], counts i64 [B, O+1, 2], bad i64 [B]. counts[b,g,1] is 0 for
 * g >= 1.
 *
 * Per pixel p of image b, with g = gt_obj[p]:
 *   Ignored pixel. g == ignore_label: the pixel adds nothing anywhere, except
 *     counts[b,0,1] += 1. This rule comes first.
 *   Bad pixel. Any of the following makes the pixel add 1 to bad[b] and nothing else:
 *     g is outside 0..O;
 *     g is in 1..O and gt_frag[p] is outside 0..F-1;
 *     g is in 1..O and gt_weight[p] is not a finite number > 0 (the reference divides the
 *     weight by itself at loss.py:208-210 and would yield NaN there).
 *   Object term, every other pixel. x is the row of O+1 logits, m = max x, and
 *     s = sum_c exp(x_c - m) in index order; ce = log(s) + (m - x_g). All of this is in fp64 on
 *     the fp32 values. The two summands are taken as written: both are >= 0, so nothing
 *     cancels. sums[b,g,0] += ce and counts[b,g,0] += 1.
 *   Fragment terms, pixels with g in 1..O.
 *     The same ce over the F logits frag_logits[p,g-1,:] with target f = gt_frag[p], added to
 *     sums[b,g,1]. With one assigned fragment the normalised target distribution of
 *     loss.py:196-210 is one-hot, so the weight does not enter here.
 *     For the three values d_k = frag_loc[p,g-1,f,k] - gt_loc[p,k] in fp64:
 *     hub_k = |d_k| <= 1 ? 0.5 * d_k * d_k : |d_k| - 0.5. This is tf.losses.huber_loss with
 *     delta = 1. sums[b,g,2] += gt_weight[p] * (hub_0 + hub_1 + hub_2), summed left to right.
 *     No FMA in either formula.
 *   Reads. Background, ignored and bad pixels read no fragment logit. A foreground pixel reads
 *     only its object's F logits and three localisation values.
 * A NaN or Inf logit is not a bad pixel: it makes its sum non-finite, and the host reports that.
 *
 * Order of the sums (no floating-point atomics). An image's pixels are cut into shares of
 * epos_loss_share_pixels(P, O, F) consecutive pixels, the last one shorter; the share is a
 * function of P, O and F only, never of B, and no share straddles two images. A workgroup owns
 * one share: per cell it adds the share's terms in pixel order, starting from 0.0, and writes
 * its partial tables to `workspace` (epos_loss_workspace_bytes(B, P, O, F) bytes, 8-byte
 * aligned, contents undefined before and after). A closing launch adds an image's partial
 * tables in share order, starting from 0.0. So the same input gives the same bytes on every
 * run, and an image's rows are the same bytes alone and at any position of any batch.
 * The one freedom inside a pixel: the L lanes that share a row (L = 1 for F <= 4, else the
 * power of two with 2L < F <= 4L; lane j holds x_c for c mod 4L in 4j..4j+3) each add their
 * own exponentials in index order and the L partial sums are added as a butterfly, so s -- and
 * only s -- may differ from the index-order sum by the rounding of F (or O+1) additions.
 *
 * Refused with EPOS_E_INVALID before the first launch: O, F, P or B out of range (B < 0,
 * B > 65535, B * shares per image >= 2^31), ld_obj < O+1, a null pointer or a workspace that
 * is not 8-byte aligned when B > 0 and P > 0. B == 0 or P == 0 does nothing and returns 0.
 * ------------------------------------------------------------------------- */
/* Pixels per share, 0 for P == 0; EPOS_E_INVALID for sizes epos_loss_terms refuses. */
int64_t epos_loss_share_pixels(int64_t P, int num_objs, int num_frags);
/* Bytes of workspace one call needs: B * ceil(P / share) * (5 (O+1) + 1) * 8; 0 when B == 0
 * or P == 0; EPOS_E_INVALID for sizes epos_loss_terms refuses. */
int64_t epos_loss_workspace_bytes(int B, int64_t P, int num_objs, int num_frags);
int epos_loss_terms(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                    const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                    const float* gt_loc, const float* gt_weight, int B, int64_t P, int num_objs,
                    int num_frags, int ignore_label, void* workspace, double* sums,
                    int64_t* counts, int64_t* bad, void* stream);

/* Loss values and gradients (csrc/loss_grad.hip; added without an ABI version change).
 * tests/helpers/loss_grad_ref.py restates every rule below in element-wise numpy; through it
 * the formulas are pinned to torch's fp64 autograd. Parity with TensorFlow's gradients is
 * unpinned, as for the forward.
 *
 * epos_loss_reduce reads the tables epos_loss_terms wrote, sums f64 [B,O+1,3] and counts i64
 * [B,O+1,2] [device], and WRITES values f64 [4] -- obj_cls_loss, frag_cls_loss, frag_loc_loss,
 * total_loss of the batch, weighted -- and scales f64 [B,3], the per-image factors of the
 * gradient [device]. Per image P_b = sum_g counts[b,g,0] + counts[b,0,1] and
 * n_b = sum_{g>=1} counts[b,g,0]; objects are added in index order, the mean is taken first
 * and the weight applied last, as epos_amd/loss.py image_losses does.
 *   EPOS_LOSS_MEAN: the mean over the images of the per-image losses (a fragment loss of an
 *     image with n_b == 0 is 0): values[k] = (sum_b l_bk) / B, the images added in order from
 *     0.0, `/ B` last, for k = 0..2 and for the per-image totals (l_b0 + l_b1) + l_b2 (k = 3):
 *     bit-equal to loss.summarize(...)['mean'] on the same tables. So values[3] is the mean of
 *     the totals; it equals (values[0] + values[1]) + values[2] up to the rounding of B sums.
 *     scales[b] = { w_obj / (P_b * B), w_cls / (n_b * B), w_loc / (3 * n_b * B) }, each one
 *     fp64 division by the exactly representable integer product; the two fragment factors
 *     are 0 when n_b == 0.
 *   EPOS_LOSS_POOLED: the batch as one example set (what the reference's trainer does with a
 *     batch): per table cell the images added in order, then the objects in order;
 *     values[3] = (values[0] + values[1]) + values[2]; bit-equal to summarize(...)['pooled'].
 *     scales[b] = { w_obj / sum P, w_cls / N_fg, w_loc / (3 N_fg) } for every b, the fragment
 *     factors 0 when N_fg == 0.
 * One launch of one workgroup, no floating-point atomics, no allocation, no synchronisation.
 * Refused with EPOS_E_INVALID: B < 0, num_objs outside 1..4095, an unknown reduction, a null
 * pointer when B > 0. B == 0 returns 0 and writes nothing.
 *
 * epos_loss_grads WRITES the derivative of sum_k u_k * values[k]'s three losses with respect to
 * the three logit tensors: u_k = upstream[k] + upstream[3] (upstream f64 [4] [device], read on
 * the device; NULL means {0,0,0,1}) and s_k = scales[b,k] * u_k, one fp64 product. Inputs as
 * for epos_loss_terms; d_obj f32 with row stride ld_dobj >= O+1, d_frag f32 [B*P,O,F], d_loc
 * f32 [B*P,O,F,3]. The pixel rules are the forward's: ignored first, then bad, then
 * background, then foreground g in 1..O with fragment f and weight w. For every pixel p:
 *   d_obj[p,c], c in 0..O: +0.0 for an ignored or bad pixel, otherwise
 *     fl32( s_0 * (exp(x_c - m) / S - [c == g]) ) with m = max x and S = sum_c exp(x_c - m) in
 *     fp64 on the fp32 values, S added as in the forward (each lane its own values in index
 *     order, then a butterfly over the L lanes of the row): the only freedom in the result.
 *   d_frag[p,o,c]: the row o == g-1 of a foreground pixel is
 *     fl32( s_1 * (exp(x_c - m) / S - [c == f]) ) over that row's F logits; +0.0 elsewhere.
 *   d_loc[p,o,c,k]: the three values at (g-1, f) of a foreground pixel are
 *     fl32( s_2 * ( (double)w * clamp((double)q_k - (double)t_k, -1, 1) ) ), q = frag_loc,
 *     t = gt_loc, in that order of operations without FMA: the derivative of the Huber term,
 *     knee included (|d| <= 1 gives d); +0.0 elsewhere.
 * EVERY element is written -- the caller zeroes nothing -- except the ld_dobj - (O+1) padding
 * columns of d_obj, which are not touched. Any of d_obj, d_frag, d_loc may be NULL: that head
 * is skipped, neither loaded for nor stored to; all three NULL returns 0 and launches nothing.
 * A non-finite logit makes the elements of its own row non-finite and no others; that is not
 * an error. A workgroup owns epos_loss_grad_share_pixels(P, O, F) consecutive pixels of one
 * image -- a function of P alone, 0 for P == 0 -- and every element is computed from its own
 * pixel and s_k only: one launch, no allocation, no synchronisation, no atomics, capturable
 * in a graph, the same bytes in every run.
 * Refused with EPOS_E_INVALID before the launch: the sizes epos_loss_terms refuses, ld_obj or
 * ld_dobj < O+1, a null input (scales included) when B > 0 and P > 0, an output buffer that
 * starts at an input pointer. B == 0 or P == 0 does nothing and returns 0. */
#define EPOS_LOSS_MEAN 0
#define EPOS_LOSS_POOLED 1
int epos_loss_reduce(const double* sums, const int64_t* counts, int B, int num_objs,
                     double w_obj, double w_cls, double w_loc, int reduction,
                     double* values /* [4] */, double* scales /* [B,3] */, void* stream);
int64_t epos_loss_grad_share_pixels(int64_t P, int num_objs, int num_frags);
int epos_loss_grads(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                    const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                    const float* gt_loc, const float* gt_weight, int B, int64_t P,
                    int num_objs, int num_frags, int ignore_label, const double* scales,
                    const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                    float* d_obj, int64_t ld_dobj, float* d_frag, float* d_loc, void* stream);

/* Weight gradients (csrc/heads_wgrad.hip; added without an ABI version change). The gradient
 * of the losses with respect to the weights and biases of the three logits layers
 * (logits/pred_obj_conf, logits/pred_frag_conf, logits/pred_frag_loc: 1x1 convolutions on
 * EposNet.decoder_out), taken WITHOUT forming the dense logit gradients, and the optimiser
 * step of the reference's trainer. tests/helpers/heads_wgrad_ref.py restates both in numpy.
 *
 * epos_heads_wgrad_f32. A f32 [device]: the tensor the logits layers read, B*P rows of K
 * values with row stride lda >= K, 1 <= K <= 1024. The next sixteen arguments are exactly the
 * inputs of epos_loss_grads. Outputs f32 [device], row-major in the layout of the checkpoint
 * variables logits/<name>/weights [1,1,K,N] and biases [N]: dW_obj [K, O+1], db_obj [O+1],
 * dW_frag [K, O*F], db_frag [O*F], dW_loc [K, O*F*3], db_loc [O*F*3]. All outputs are WRITTEN,
 * not added, every element of them, +0.0 for an object or a fragment without a pixel. A head
 * whose dW and db are both NULL is skipped and nothing of it is loaded; dW NULL with db
 * non-NULL, and the reverse, are allowed.
 *   Definition. Let d_obj, d_frag, d_loc be the f32 values epos_loss_grads is specified to
 *   write for the same inputs (the fl32-rounded values, with its m, its S and its butterfly
 *   over the L lanes of a row). Then for each head h
 *     dW_h[k,n] = fl32( sum_p (double)A[p,k] * (double)d_h[p,n] )
 *     db_h[n]   = fl32( sum_p (double)d_h[p,n] )
 *   over the B*P pixels, accumulated in fp64 (the product of two fp32 values is exact in fp64)
 *   and rounded to f32 once, at the end. The sum runs over the pixels for which column n is
 *   ACTIVE only: the O+1 object values of a pixel that is neither ignored nor bad, the F values
 *   of the row g-1 and the three values at (g-1, f) of a foreground pixel. The other d values
 *   are +0.0 and are not multiplied: a non-finite feature or logit makes the columns its pixel
 *   touches non-finite and no others; ignored and bad pixels contribute nothing.
 *   Never dense. The kernels compute each pixel's active values themselves; neither a kernel
 *   nor the workspace holds a row of width O*F or O*F*3 per pixel. With N = O+1 + 4*O*F, the
 *   number of columns of the three heads together, an image's pixels are cut into
 *     R = 1 when N < 10, else min(8, max(1, floor(P / max(1024, 8 (K+1)))))
 *   ranges of epos_heads_wgrad_range_pixels(P, O, F, K) = ceil(P / R) consecutive pixels, the
 *   last one shorter: a function of its arguments only, never of B, and no range straddles two
 *   images. The workspace holds, per pixel, S of the object row and of the fragment row (f64)
 *   and m of the object row (f32), and, when R > 1, R partial slabs f64 [K+1, N]:
 *     epos_heads_wgrad_workspace_bytes(B, P, O, F, K) = 20 * B * P + (R > 1 ? R * 8 * (K+1) * N : 0),
 *   8-byte aligned, contents undefined before and after. The slabs are at most P * N bytes, a
 *   quarter of ONE image's dense gradients, so the whole stays below the 4 * B * P * N bytes of
 *   the dense gradients for every size.
 *   Order of the sums (no floating-point atomics, the same bytes in every run). A workgroup
 *   owns range r of EVERY image and adds image after image. Fragment and localisation columns
 *   of object g: the range's pixels of class g in pixel order, one accumulator per (k, n).
 *   Object columns: the i-th pixel of a range belongs to lane i mod 32; a lane adds its pixels
 *   in order; the 32 lanes are added in lane order, from 0.0. The bias row is the same sum with
 *   a feature of 1.0. With R == 1 these sums are rounded and written. With R > 1 they go to
 *   slab r, and a closing launch adds the slabs in range order, from 0.0, and rounds. The
 *   result depends on the batch as a whole: permuting the images changes the order.
 *   Launches. Up to four launches on `stream` in sequence (the per-pixel S and m; the object
 *   head; the fragment and localisation heads; the closing pass), no allocation, no host
 *   synchronisation, capturable in a graph without parallel branches.
 *   Refused with EPOS_E_INVALID before the first launch: the sizes epos_loss_terms refuses;
 *   K outside 1..1024; lda < K; ld_obj < O+1; when B > 0, P > 0 and some output is wanted, a
 *   null input (scales and workspace included; upstream may be NULL) or a workspace that is not
 *   8-byte aligned; an output that starts at an input pointer (the workspace counts as one).
 *   When B == 0 or P == 0 the wanted outputs are written as zeros (no input is read) and the
 *   call returns 0. All six outputs NULL returns 0 and launches nothing.
 *
 * epos_momentum_step_f32: tf.train.MomentumOptimizer without Nesterov on the gradient of the
 * reference's trainer (train.py:340-384; the l2 regulariser adds weight_decay * w, model.py:436;
 * the whole gradient is multiplied by the variable's multiplier, train_utils.py:84-114). In
 * place on w and accum, f32 [device], n values each; per element in fp32, each operation
 * rounded once, no FMA:
 *     g  = grad_mult * (grad + weight_decay * w)
 *     a' = momentum * accum + g
 *     w' = w - lr * a'
 * One launch for any n and any 4-byte alignment: a 16-byte body with up to three scalar
 * elements in front and behind where the three arrays reach a 16-byte boundary together,
 * scalar throughout otherwise. Refused with EPOS_E_INVALID: n < 0, n > 2^38, a null pointer
 * or a pointer that is not 4-byte aligned when n > 0. n == 0 does nothing and returns 0. */
int64_t epos_heads_wgrad_workspace_bytes(int B, int64_t P, int num_objs, int num_frags, int K);
int64_t epos_heads_wgrad_range_pixels(int64_t P, int num_objs, int num_frags, int K);
int epos_heads_wgrad_f32(const float* A, int64_t lda, int K, const float* obj_logits,
                         int64_t ld_obj, const float* frag_logits, const float* frag_loc,
                         const int32_t* gt_obj, const int32_t* gt_frag, const float* gt_loc,
                         const float* gt_weight, int B, int64_t P, int num_objs, int num_frags,
                         int ignore_label, const double* scales,
                         const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                         void* workspace, float* dW_obj, float* db_obj, float* dW_frag,
                         float* db_frag, float* dW_loc, float* db_loc, void* stream);
int epos_momentum_step_f32(float* w, float* accum, const float* grad, int64_t n, float lr,
                           float momentum, float weight_decay, float grad_mult, void* stream);

/* Input gradient (csrc/heads_dgrad.hip; added without an ABI version change). The gradient of
 * the losses with respect to the tensor the three logits layers read (EposNet.decoder_out),
 * dL/dX: what backpropagation below the logits starts from. Taken WITHOUT forming the dense
 * logit gradients. tests/helpers/heads_dgrad_ref.py restates it in numpy.
 *
 * epos_heads_dgrad_f32. The first sixteen arguments are exactly the inputs of epos_loss_grads,
 * under the same rules. Wt_obj f32 [O+1, K], Wt_frag f32 [O*F, K], Wt_loc f32 [O*F*3, K]
 * [device]: the three weight matrices TRANSPOSED (the checkpoint holds [1,1,K,N]; a pixel's
 * active columns n become contiguous rows of K values), all three with row stride ldwt >= K,
 * 1 <= K <= 1024. Y f32 [device] with row stride ldy >= K, or NULL: the forward activation, for
 * the ReLU mask. dX f32 [device]: B*P rows of K values with row stride ldx >= K.
 *   Definition. Let d_obj, d_frag, d_loc be the f32 values epos_loss_grads is specified to
 *   write for the same inputs (the fl32-rounded values, with its m, its S and its butterfly
 *   over the L lanes of a row). Then
 *     dX[p,k] = fl32( sum_h sum_{n active at p} (double)d_h[p,n] * (double)Wt_h[n,k] )
 *   accumulated in fp64 (the product of two fp32 values is exact in fp64) from 0.0 in a FIXED
 *   order -- the heads in the order obj, frag, loc, ascending n within a head, one accumulator
 *   per (p, k) -- and rounded to f32 once, at the end. ACTIVE as for epos_heads_wgrad_f32: the
 *   O+1 object values of a pixel that is neither ignored nor bad, the F values of the row g-1
 *   and the three values at (g-1, f) of a foreground pixel: at most O+1 + F + 3 of the
 *   O+1 + 4*O*F columns. The other d values are +0.0 and are not multiplied. An ignored or bad
 *   pixel gets a row of +0.0 and nothing of it but its labels is read. A non-finite logit or
 *   weight makes its own pixel's row non-finite (a weight: the rows of the pixels for which its
 *   column is active) and no others; that is not an error.
 *   ReLU mask. With Y non-NULL, dX[p,k] is written as +0.0 wherever Y[p,k] <= 0 (-0.0 counts,
 *   a NaN does not): the gradient with respect to the pre-activation of the layer that
 *   produced X (decoder_conv1_pointwise with its batch norm folded). With Y NULL it is the
 *   gradient with respect to X itself. Y may be the buffer of the features.
 *   EVERY element of dX is WRITTEN, not added; the ldx - K padding columns are not touched.
 *   Never dense, and no workspace: a wave computes a pixel's active d values itself, 64 at a
 *   time, one per lane; neither a kernel nor a buffer holds a row of width O*F or O*F*3.
 *   One launch on `stream`, a workgroup per 16 consecutive pixels of one image: no allocation,
 *   no host synchronisation, no atomics, capturable in a graph; the same bytes in every run,
 *   for an image alone and at any position of a batch, and for every alignment of the buffers.
 *   Refused with EPOS_E_INVALID before the launch: the sizes epos_loss_terms refuses; K outside
 *   1..1024; ldx or ldwt < K, ldy < K when Y is given; ld_obj < O+1; when B > 0 and P > 0, a
 *   null pointer (upstream and Y may be NULL); dX starting at an input pointer, Y included: the
 *   mask is read while other lanes write the row. B == 0 or P == 0 writes nothing and
 *   returns 0. */
int epos_heads_dgrad_f32(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                         const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                         const float* gt_loc, const float* gt_weight, int B, int64_t P,
                         int num_objs, int num_frags, int ignore_label, const double* scales,
                         const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                         const float* Wt_obj, const float* Wt_frag, const float* Wt_loc,
                         int64_t ldwt, int K, const float* Y /* or NULL */, int64_t ldy,
                         float* dX, int64_t ldx, void* stream);

/* k nearest fragments (csrc/render.hip, loss.hip, loss_grad.hip, heads_wgrad.hip,
 * heads_dgrad.hip; added without an ABI version change: no existing entry gains, loses or
 * reorders an argument). The reference's gt_knn_frags (train.py:82, datagen_utils.py:161-199,
 * loss.py:186-229 and 267-303): every foreground pixel is assigned to its knn nearest fragments
 * and the two fragment losses run over the n * knn (pixel, fragment) rows. Each entry below takes
 * the arguments of its sibling plus `int knn`, and the sibling is the same body called with
 * knn = 1: at knn = 1 every output of every entry is the same bytes. Everything the sections
 * above say holds, with the following changes. tests/helpers/knn_ref.py restates them in
 * element-wise numpy.
 *
 *   1 <= knn <= min(F, EPOS_LOSS_MAX_KNN); anything else is EPOS_E_INVALID before the first
 *   launch. The cap is 4: the fragment kernel of the weight gradient keeps a batch's slots in
 *   static LDS -- 64 pixels x knn x (fragment, weight, three localisation gradients), 20 bytes
 *   per slot -- next to its tables; that is 55.9 KB at one slot and 59.7 KB at four, and the
 *   next power of two would leave less than 1 KB of the 64 KB a static allocation may have.
 *
 *   Ground truth (epos_gt_fields_knn). frag_label i32 [h,w,knn], frag_loc f32 [h,w,knn,3],
 *   frag_weight f32 [h,w,knn]. Slot j of a pixel an instance takes holds the j-th nearest
 *   fragment centre: the distance dx^2 + dy^2 + dz^2 summed in that order in fp64 on the fp32
 *   xyz, the slots in ascending distance, ties to the lower fragment index. frag_loc[...,j,:]
 *   and frag_weight[...,j] are those of epos_gt_fields for that fragment. A pixel no instance
 *   takes gets label 0, location 0 and weight 0 in every slot.
 *
 *   The loss entries read gt_frag i32 [B*P, knn], gt_loc f32 [B*P, knn, 3] and gt_weight f32
 *   [B*P, knn].
 *   Pixel class. As above, and a foreground pixel is also bad if ANY slot's fragment is outside
 *   0..F-1, if any slot's weight is not a finite number > 0, or if two slots name the same
 *   fragment.
 *   Forward (epos_loss_terms_knn). With m and s of the row frag_logits[p,g-1,:] as above and
 *   slot j's fragment f_j and weight w_j:
 *     sums[b,g,1] += sum_j ( log(s) + (m - x_{f_j}) )
 *     sums[b,g,2] += sum_j w_j * ((hub_0 + hub_1) + hub_2), hub_k of frag_loc[p,g-1,f_j,k] -
 *     gt_loc[p,j,k]
 *   both sums over j ascending from 0.0, each summand taken exactly as with one slot. counts
 *   keep counting pixels.
 *   Reduce (epos_loss_reduce_knn). n_b is replaced by n_b * knn (N_fg by N_fg * knn) in the two
 *   fragment means and in scales[b,1] and scales[b,2]; the integer product is exact, and the
 *   result is 0 when n_b == 0. Bit-equal to loss.summarize(..., knn=knn). knn outside
 *   1..EPOS_LOSS_MAX_KNN is refused (the entry does not know F).
 *   Logit gradients (epos_loss_grads_knn).
 *     d_frag[p,g-1,c] = fl32( s_1 * ((double)knn * pr_c - t_c) ), pr_c = exp(x_c - m) / S and
 *     t_c = 1 when c is one of the pixel's fragments, else 0;
 *     d_loc at (g-1, f_j, .) is the value above with w_j and gt_loc[p,j,.], for every slot;
 *     everything else is +0.0.
 *   Weight gradient (epos_heads_wgrad_knn_f32). ACTIVE are the O+1 object values, the F values
 *   of the row g-1 and the 3 * knn localisation values at (g-1, f_j). A pixel contributes to a
 *   given (k, column) cell at most once, so the order per cell is still pixel order; ranges,
 *   slabs, closing pass and epos_heads_wgrad_workspace_bytes are unchanged.
 *   Input gradient (epos_heads_dgrad_knn_f32). The order stays "obj, frag, loc, ascending n
 *   within a head": a pixel's slots are visited in ascending fragment index, whatever their
 *   order in gt_frag. At most O+1 + F + 3 * knn active columns.
 *   Launches, workspaces, share, range and workspace functions: those of the siblings. */
#define EPOS_LOSS_MAX_KNN 4
int epos_gt_fields_knn(const float* depth, const float* local_pos, const uint8_t* masks,
                       const int32_t* obj_ids, int n_inst, int h, int w, const double* centers,
                       const double* sizes, int num_objs, int num_frags, int knn,
                       int32_t* obj_label, int32_t* instance, int32_t* frag_label,
                       float* frag_loc, float* frag_weight, void* stream);
int epos_loss_terms_knn(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                        const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                        const float* gt_loc, const float* gt_weight, int B, int64_t P,
                        int num_objs, int num_frags, int ignore_label, int knn, void* workspace,
                        double* sums, int64_t* counts, int64_t* bad, void* stream);
int epos_loss_reduce_knn(const double* sums, const int64_t* counts, int B, int num_objs,
                         double w_obj, double w_cls, double w_loc, int reduction, int knn,
                         double* values /* [4] */, double* scales /* [B,3] */, void* stream);
int epos_loss_grads_knn(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                        const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                        const float* gt_loc, const float* gt_weight, int B, int64_t P,
                        int num_objs, int num_frags, int ignore_label, int knn,
                        const double* scales,
                        const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                        float* d_obj, int64_t ld_dobj, float* d_frag, float* d_loc, void* stream);
int epos_heads_wgrad_knn_f32(const float* A, int64_t lda, int K, const float* obj_logits,
                             int64_t ld_obj, const float* frag_logits, const float* frag_loc,
                             const int32_t* gt_obj, const int32_t* gt_frag, const float* gt_loc,
                             const float* gt_weight, int B, int64_t P, int num_objs,
                             int num_frags, int ignore_label, int knn, const double* scales,
                             const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                             void* workspace, float* dW_obj, float* db_obj, float* dW_frag,
                             float* db_frag, float* dW_loc, float* db_loc, void* stream);
int epos_heads_dgrad_knn_f32(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                             const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                             const float* gt_loc, const float* gt_weight, int B, int64_t P,
                             int num_objs, int num_frags, int ignore_label, int knn,
                             const double* scales,
                             const double* upstream /* device [4], or NULL = {0,0,0,1} */,
                             const float* Wt_obj, const float* Wt_frag, const float* Wt_loc,
                             int64_t ldwt, int K, const float* Y /* or NULL */, int64_t ldy,
                             float* dX, int64_t ldx, void* stream);

/* Pointwise weight gradient (csrc/pointwise_wgrad.hip; added without an ABI version change). The
 * gradients of a 1x1 conv layer with a FROZEN batch norm -- decoder/decoder_conv1_pointwise,
 * the layer below the logits -- from its input A and the gradient G at its pre-activation
 * (epos_heads_dgrad_f32 with Y given writes G). tests/helpers/pointwise_wgrad_ref.py restates
 * it in numpy.
 *
 * The layer's forward is y = relu(scale (.) (A W) + bias) with, per output channel c,
 *     scale_c = fl32(gamma_c / sqrt(var_c + eps))   (the quotient in fp64, rounded once)
 *     bias_c  = beta_c - mean_c scale_c
 * A [M,K] the layer's input, W [K,N] the checkpoint's `weights`; mean and var are the moving
 * statistics and are constants (the reference's fine_tune_batch_norm=False), gamma and beta are
 * variables. With G [M,N] = dL/d(pre-activation), S = A^T G [K,N] and g_c = sum_p G[p,c]:
 *     dW[k,c]   = scale_c S[k,c]
 *     dbeta_c   = g_c
 *     dgamma_c  = rstd_c (sum_k W[k,c] S[k,c] - mean_c g_c),    rstd_c = 1 / sqrt(var_c + eps)
 * (sum_p G[p,c] z[p,c] = sum_k W[k,c] S[k,c] for z = A W: z is never stored, and nothing is
 * divided by gamma.) One GEMM and one column sum give all three.
 *
 * epos_pointwise_wgrad_f32: S f64 [K,N] and g f64 [N] [device], every element WRITTEN.
 *   A: M rows with row stride lda (in units of 4 bytes), either fp32, or with a_presplit != 0
 *   the fp16 pairs EposDepthwiseArgs.y_h2 writes: per 16 bytes [hi(c..c+3) | mid(c..c+3)], the
 *   scale s from a_amax / a_amax2 / a_gain / a_bias exactly as EposPointwiseArgs derives it; the
 *   value summed is the one the forward GEMM multiplied, (hi + mid 2^-11) / s, exact in fp64.
 *   G: fp32, M rows with row stride ldg. The padding columns of A and G are never read.
 *   Arithmetic. Every product is exact in fp64; the sums over rows are fp64 from +0.0 on the
 *   matrix pipe (v_mfma_f64_16x16x4_f64). The result is within (M + 16) 2^-52 sum_p |A||G| of
 *   the exact sum whatever the order. A non-finite value of A or G reaches, by IEEE rules, the
 *   elements of S and g that depend on it and no others.
 *   Order of the sums (no floating-point atomics, the same bytes in every run). M is cut into
 *   ranges of epos_pointwise_wgrad_range_rows(M, K, N) consecutive rows, the last one shorter: a
 *   function of its arguments only. With one range the sums are written to S and g. With more,
 *   range r writes its sums to slab r of the workspace, f64 [K*N + N], and a closing launch adds
 *   the slabs in range order, from +0.0. Within a range, S[k,c] adds the rows four at a time in
 *   ascending order (the matrix pipe's order within four); g_c adds every fourth row, then the
 *   four partial sums in their order.
 *   workspace [device]: epos_pointwise_wgrad_workspace_bytes(M, K, N) bytes (0 with one range:
 *   it may then be NULL), 8-byte aligned, contents undefined before and after.
 *   Launches: one, or two with more than one range, on `stream`; no allocation, no host
 *   synchronisation, capturable in a graph.
 *   Refused with EPOS_E_INVALID before the launch, nothing written: null args, A, G, S or g; M,
 *   K or N < 1; lda < K; ldg < N; A or G not 4-byte, S or g not 8-byte aligned; a missing or
 *   misaligned workspace when one is needed; a pre-split A without a_amax, or with K % 4 != 0,
 *   lda % 4 != 0 or A not 16-byte aligned.
 *
 * epos_pointwise_wgrad_close_f32: the checkpoint-shaped fp32 gradients from S and g. W f32
 * [K,N] contiguous; gamma, moving_mean, moving_variance f32 [N]; dW f32 [K,N], dgamma and
 * dbeta f32 [N] [device]. The three formulas above, each operation in fp64 and rounded once (no
 * FMA), sum_k in sixteen partial sums (k mod 16, ascending) added in their order, the result
 * rounded to fp32 once; a result of -0.0 is written as +0.0. With gamma NULL (a conv with
 * biases and no batch norm; moving_mean, moving_variance and dgamma must then be NULL, W is
 * not read): dW = fl32(S), dbeta = fl32(g) is the gradient of `biases`. One launch.
 *   It is also the closing of the depthwise gradients ("Depthwise gradients" below): the
 *   checkpoint's depthwise_weights [3,3,C,1] is a contiguous [9][C] matrix, and with K = 9,
 *   N = C, S = T and g = t the three formulas are dw = scale T, dbeta = t and dgamma = rstd
 *   (sum_tap w T - mean t). No other entry closes them.
 *   Refused with EPOS_E_INVALID: K or N < 1; a null S, g, dW or dbeta; with gamma, a null W,
 *   moving_mean, moving_variance or dgamma, or an eps that is negative or NaN; without gamma, a
 *   non-null moving_mean, moving_variance or dgamma; a misaligned pointer. */
typedef struct EposPointwiseWgradArgs {
  const void* A; int64_t lda;
  const float* G; int64_t ldg;
  int64_t M;
  int32_t K, N;
  int32_t a_presplit;
  int32_t reserved0;        /* 0 */
  const uint32_t* a_amax;   /* as in EposPointwiseArgs; read only with a_presplit */
  const uint32_t* a_amax2;
  float a_gain, a_bias;
  double* S;
  double* g;
  void* workspace;
} EposPointwiseWgradArgs;
int64_t epos_pointwise_wgrad_workspace_bytes(int64_t M, int K, int N);
int64_t epos_pointwise_wgrad_range_rows(int64_t M, int K, int N);
int epos_pointwise_wgrad_f32(const EposPointwiseWgradArgs* args, void* stream);
int epos_pointwise_wgrad_close_f32(const double* S, const double* g, const float* W, int K, int N,
                                   const float* gamma, const float* moving_mean,
                                   const float* moving_variance, double eps, float* dW,
                                   float* dgamma, float* dbeta, void* stream);

/* Pointwise input gradient (csrc/pointwise_dgrad.hip; added without an ABI version change). The
 * gradient that crosses a 1x1 conv layer with a folded batch norm --
 * decoder/decoder_conv1_pointwise -- from the gradient G at its pre-activation to the
 * pre-activation of the layer that produced its input: D = mask (.) (G Wf^T).
 * tests/helpers/decoder_backward_ref.py restates it in numpy.
 *
 * The layer's forward is y = relu(scale (.) (A W) + bias), scale_c = fl32(gamma_c / sqrt(var_c +
 * eps)) exactly as "Pointwise weight gradient" defines it. The forward multiplies by the FOLDED
 * matrix Wf[k,c] = fl32(W[k,c] * scale_c), a single fp32 product, as EposNet.set_weights and the
 * plan's host fold compute it; this entry multiplies by the same matrix. With gamma NULL the
 * layer is a conv with biases: Wf = W, and moving_variance must be NULL too.
 *
 * epos_pointwise_dgrad_f32. G f32 [M,N] with row stride ldg; W f32 [K,N] contiguous, the
 * checkpoint's layout; gamma, moving_variance f32 [N]; D f32 [M,K] with row stride ldd [device].
 *     D[p,k] = fl32( sum_c (double)G[p,c] * (double)Wf[k,c] )
 *   Arithmetic. Every product is exact in fp64; one fp64 accumulator per (p, k) from +0.0 on the
 *   matrix pipe (v_mfma_f64_16x16x4_f64), the c in an order that (K, N) alone fix, rounded to
 *   fp32 once. N is a layer width (<= 1024): no split over c, no slabs, no atomics. The same
 *   bytes in every run, for a row alone and at any position of M, and for every alignment of the
 *   buffers. Within 2^-24 |exact| + (N + 16) 2^-52 sum_c |G||Wf| of the exact sum.
 *   Mask. mask NULL, or M rows of K columns with row stride ldm: the layer's input A, that is
 *   the output of the layer below behind its ReLU. D[p,k] is written as +0.0 wherever the mask
 *   value is <= 0 (-0.0 counts, a NaN does not): D is then the gradient at the pre-activation of
 *   the layer below. With mask_h2 != 0 the mask holds the fp16 pairs EposDepthwiseArgs.y_h2
 *   writes, per 16 bytes [hi(k..k+3) | mid(k..k+3)], and its value is hi + mid 2^-11: only the
 *   sign matters, so no absmax slot is read. That is the value the forward GEMM multiplied: a
 *   y > 0 that the split flushed to zero is masked, as the forward saw a zero there.
 *   EVERY element of D is WRITTEN; the padding columns of G, mask and D are never read or
 *   written. A non-finite G[p,.] reaches row p only, a non-finite weight column k only (by IEEE
 *   rules, 0 * Inf included); a masked element is +0.0 whatever the sum.
 *   workspace [device]: epos_pointwise_dgrad_workspace_bytes(K, N) bytes, 16-byte aligned: Wf in
 *   fp64, its rows padded to a multiple of 64 and its columns to one of 16 with +0.0. Contents
 *   undefined before, Wf after.
 *   Launches: two on `stream`, the fold and the GEMM; no allocation, no host synchronisation,
 *   capturable in a graph.
 *   Refused with EPOS_E_INVALID before any launch, nothing written: null args, G, W, D or
 *   workspace; M, K or N < 1; K or N > 1024; ldg < N; ldd < K; ldm < K with a mask; gamma
 *   without moving_variance or the reverse; with gamma an eps that is negative or NaN; a pointer
 *   that is not 4-byte (the workspace: 16-byte) aligned; mask_h2 with K % 4 != 0, ldm % 4 != 0
 *   or a mask that is not 16-byte aligned; D starting at G or at mask. */
typedef struct EposPointwiseDgradArgs {
  const float* G; int64_t ldg;
  const float* W;               /* [K,N] */
  const float* gamma;           /* [N], or NULL with moving_variance NULL */
  const float* moving_variance;
  double eps;
  const void* mask; int64_t ldm;   /* or NULL */
  int32_t mask_h2;
  int32_t reserved0;            /* 0 */
  int64_t M;
  int32_t K, N;
  float* D; int64_t ldd;
  void* workspace;
} EposPointwiseDgradArgs;
int64_t epos_pointwise_dgrad_workspace_bytes(int K, int N);
int epos_pointwise_dgrad_f32(const EposPointwiseDgradArgs* args, void* stream);

/* Depthwise gradients (csrc/depthwise_grad.hip; added without an ABI version change). The
 * backward pass of a 3x3 depthwise layer with a FROZEN batch norm, stride 1 --
 * decoder/decoder_conv1_depthwise. tests/helpers/decoder_backward_ref.py restates both entries.
 *
 * The layer's forward is a = relu(scale_c sum_tap w[tap,c] X[b, y+(ky-1)r, x+(kx-1)r, c] +
 * bias_c), TF 'SAME' (zero) padding, r = rate, tap = 3 ky + kx as in EposDepthwiseArgs. D f32
 * [B,H,W,C] is dL/d(pre-activation): what epos_pointwise_dgrad_f32 writes with the mask.
 *
 * epos_depthwise_wgrad_f32: T f64 [9,C] and t f64 [C] [device], every element WRITTEN.
 *     T[tap,c] = sum_{b,y,x} X[b, y+(ky-1)r, x+(kx-1)r, c] * D[b,y,x,c]
 *     t[c]     = sum_{b,y,x} D[b,y,x,c]
 *   A tap in the padding adds nothing; a tap never reads a neighbouring image of the batch. X
 *   f32 with pixel stride ldx, D f32 with pixel stride ldd, C % 4 == 0 as in the forward; the
 *   padding columns are never read. Products exact in fp64, sums in fp64 from +0.0: within
 *   (B H W + 16) 2^-52 sum |X||D| of the exact sum whatever the order.
 *   Order of the sums (no atomics, the same bytes in every run). The B H W pixels, in (b, y, x)
 *   order, are cut into ranges of epos_depthwise_wgrad_range_pixels(B, H, W, C) pixels, the
 *   last one shorter: a function of its arguments only. With one range the sums are written to
 *   T and t; with more, range r writes slab r of the workspace, f64 [9*C + C], and a closing
 *   launch adds the slabs in range order from +0.0. Within a range: with s = 256 / min(C / 4,
 *   16) pixel slots, slot j adds the range's pixels j, j + s, j + 2 s, ... in ascending order
 *   from +0.0, then the slots' sums are added in slot order from +0.0.
 *   workspace [device]: epos_depthwise_wgrad_workspace_bytes(B, H, W, C) bytes (0 with one
 *   range: it may then be NULL), 8-byte aligned.
 *   The checkpoint-shaped gradients need NO kernel of their own: depthwise_weights [3,3,C,1] is
 *   a contiguous [9][C] matrix, and epos_pointwise_wgrad_close_f32(T, t, w, K = 9, N = C, gamma,
 *   moving_mean, moving_variance, eps, ...) is exactly dw = scale T, dbeta = t, dgamma = rstd
 *   (sum_tap w T - mean t).
 *   Launches: one, or two with more than one range; no allocation, no host synchronisation,
 *   capturable in a graph.
 *   Refused with EPOS_E_INVALID before the launch, nothing written: null args, X, D, T or t; B,
 *   H, W or C < 1; C % 4 != 0; stride != 1; rate < 1; ldx or ldd < C or not a multiple of 4; X
 *   or D not 16-byte, T or t not 8-byte aligned; a missing or misaligned workspace when one is
 *   needed.
 *
 * epos_depthwise_dgrad_f32: dX f32 [B,H,W,C] with pixel stride ldx [device].
 *     dX[b,y,x,c] = fl32( sum_tap (double)w9c[tap,c] * (double)D[b, y-(ky-1)r, x-(kx-1)r, c] )
 *   w9c f32 [9][C]: the FOLDED weights the forward reads (EposDepthwiseArgs.w9c). A tap whose
 *   source pixel lies outside the image is skipped. One fp64 accumulator per element from +0.0,
 *   the taps in ascending order, each product exact, rounded to fp32 once: reproducible bit for
 *   bit. With Y non-NULL (pixel stride ldy) dX is written as +0.0 wherever Y <= 0 (-0.0 counts,
 *   a NaN does not), the rule of epos_heads_dgrad_f32: Y is the activation the layer below
 *   produced, X itself, and dX is then the gradient at that layer's pre-activation -- for
 *   decoder_conv1_depthwise the G that epos_pointwise_wgrad_f32 takes for
 *   decoder_conv0_pointwise. EVERY element is WRITTEN; padding columns are not touched. One
 *   launch; the same bytes in every run, for an image alone and at any position of a batch.
 *   Refused with EPOS_E_INVALID: a null D, w9c or dX; B, H, W or C < 1; C % 4 != 0; rate < 1;
 *   ldd, ldx or (with Y) ldy < C or not a multiple of 4; a pointer that is not 16-byte aligned;
 *   dX starting at D. */
typedef struct EposDepthwiseWgradArgs {
  const float* X; int64_t ldx;
  const float* D; int64_t ldd;
  int32_t B, H, W, C;
  int32_t stride;               /* 1 */
  int32_t rate;
  double* T;
  double* t;
  void* workspace;
} EposDepthwiseWgradArgs;
int64_t epos_depthwise_wgrad_range_pixels(int B, int H, int W, int C);
int64_t epos_depthwise_wgrad_workspace_bytes(int B, int H, int W, int C);
int epos_depthwise_wgrad_f32(const EposDepthwiseWgradArgs* args, void* stream);
int epos_depthwise_dgrad_f32(const float* D, int64_t ldd, const float* w9c,
                             const float* Y /* or NULL */, int64_t ldy, float* dX, int64_t ldx,
                             int B, int H, int W, int C, int rate, void* stream);

/* Resize input gradient (csrc/resize_grad.hip; added without an ABI version change). The adjoint
 * of the align-corners bilinear resize -- decoder/resize, from the decoder's size back to the
 * encoder's. tests/helpers/resize_grad_ref.py restates it operation for operation.
 *
 * The forward it is the adjoint of (bilinear_sample, csrc/nhwc.h), per axis in -> out:
 *   s = float(in - 1) / float(out - 1) in fp32, 0 for out == 1; f = o s in fp32;
 *   i0 = min(floor f, in - 1), i1 = min(ceil f, in - 1); l = f - i0 in fp32;
 *   out = top + (bot - top) ly with top = tl + (tr - tl) lx.
 * The weight of source index i on output index o, in fp64 from the fp32 l, every term exact:
 *   w(o, i) = [i0 == i](1 - l) + [i1 == i] l, and exactly 1 where i0 == i1 == i (l == 0, and the
 *   clamped last coordinate).
 *
 * epos_resize_bilinear_dgrad_f32: dX f32 [B,Hi,Wi,C] with pixel stride ldx [device] from D f32
 * [B,Ho,Wo,C] with pixel stride ldd [device], the gradient at the resize's output.
 *     dX[b,yi,xi,c] = fl32( sum_{yo,xo} (wy(yo,yi) wx(xo,xi)) * (double)D[b,yo,xo,c] )
 *   over the output pixels whose row has a tap at yi and whose column has a tap at xi.
 *   Footprint. Which (yo, xo) those are is decided by the forward's own fp32 expressions above,
 *   evaluated per output index, never by a closed form of (i +- 1) / s: where fp32 rounding moved
 *   a sample into the neighbouring cell (it does at 59 / 119), the adjoint follows the forward.
 *   i0 and i1 do not decrease with o and differ by at most 1, so the outputs of a source index
 *   are one interval [first o with i1(o) >= i, last o with i0(o) <= i], found by binary search
 *   over those expressions; it may be empty (downscaling), and dX is then +0.0.
 *   Order and arithmetic. One fp64 accumulator per element from +0.0; the output pixels of the
 *   footprint in (yo, xo) order, rows ascending, columns ascending within a row: an order fixed
 *   by the sizes alone. Per pixel w = wy * wx, p = w * (double)D, acc += p, each rounded once
 *   (the library is built with -ffp-contract=off); the sum is rounded to fp32 once. Within
 *   2^-24 |exact| + (n + 16) 2^-52 sum |w||D| of the exact sum, n = the pixels of the footprint.
 *   The identity (Hi == Ho, Wi == Wo) yields the bytes of D (a -0.0 of D becomes +0.0: the sum
 *   starts from +0.0).
 *   Mask. With Y non-NULL (f32 [B,Hi,Wi,C], pixel stride ldy: the source activation) dX is
 *   written as +0.0 wherever Y <= 0 (-0.0 counts, a NaN does not), the rule of
 *   epos_depthwise_dgrad_f32: dX is then the gradient at the pre-activation of the layer that
 *   produced the source -- for decoder/resize, concat_projection.
 *   C % 4 == 0, pitches multiples of 4, rows 16-byte aligned; padding columns are never read or
 *   written, EVERY element of dX is WRITTEN. A thread owns four channels of one source pixel
 *   (16-byte loads and store, consecutive threads along the channel axis). One launch, no
 *   workspace, no atomics, no host synchronisation, capturable in a graph; the same bytes in
 *   every run, for an image alone and at any position of a batch.
 *   Refused with EPOS_E_INVALID before the launch, nothing written: a null D or dX; B, Hi, Wi,
 *   Ho, Wo or C < 1; C % 4 != 0; Hi, Wi, Ho or Wo > 2^22; ldd, ldx or (with Y) ldy < C or not a
 *   multiple of 4; a pointer that is not 16-byte aligned; dX starting at D or at Y; in == 1 with
 *   out > 1 in either dimension -- the image-pooling broadcast, whose adjoint is a plain sum and
 *   not this entry. */
int epos_resize_bilinear_dgrad_f32(const float* D, int64_t ldd, const float* Y /* or NULL */,
                                   int64_t ldy, float* dX, int64_t ldx, int B, int Hi, int Wi,
                                   int Ho, int Wo, int C, void* stream);

/* ASPP gradients (csrc/aspp_grad.hip; added without an ABI version change). The two pieces the
 * backward pass through ASPP lacked: the adjoint of the image-pooling broadcast and the join of
 * the five branches' gradients at the encoder output. tests/helpers/aspp_grad_ref.py restates
 * both.
 *
 * epos_pool_broadcast_dgrad_f32: g f32 [B][ldg] [device] from D f32 [B*P][ldd] [device], the
 * gradient at a [B, C] tensor that was broadcast over the P pixels of each image.
 *     g[b,c] = fl32( sum_p (double)D[b P + p, c] )
 *   One fp64 sum per (b, c) from +0.0, rounded to fp32 once: within 2^-24 |exact| + (P + 16)
 *   2^-52 sum |D| of the exact sum. EVERY element of the C columns of g is WRITTEN; padding
 *   columns are not touched.
 *   Order of the sum (no atomics; the same bytes in every run and for an image at any position
 *   of a batch). The P pixels of an image are cut into ranges of
 *   epos_pool_broadcast_dgrad_range_pixels(B, P, C) pixels -- max(64, ceil(P / 64)), a function
 *   of P alone -- the last one shorter. Within a range: with s = 256 / min(C / 4, 16) pixel
 *   slots, slot j adds the range's pixels j, j + s, j + 2 s, ... in ascending order from +0.0,
 *   then the slots' sums are added in slot order from +0.0. With one range that sum is rounded
 *   and written; with more, range r of image b writes slab [b][r] of the workspace, f64 [C], and
 *   a closing launch adds an image's slabs in range order from +0.0.
 *   workspace [device]: epos_pool_broadcast_dgrad_workspace_bytes(B, P, C) bytes (0 with one
 *   range: it may then be NULL), 8-byte aligned.
 *   Launches: one, or two with more than one range; no allocation, no host synchronisation,
 *   capturable in a graph.
 *   Refused with EPOS_E_INVALID before the launch, nothing written: B, P or C < 1; C % 4 != 0;
 *   B > 65535 or B P > 2^40; ldd or ldg < C or not a multiple of 4; a null D or g; D or g not
 *   16-byte aligned; g starting at D; a missing or misaligned workspace when one is needed.
 *
 * epos_aspp_join_dgrad_f32: dX f32 [B,H,W,C] with pixel stride ldx [device], the gradient at a
 * tensor X that feeds n_plain 1x1 branches, n_dw 3x3 depthwise branches (stride 1, 'SAME') and,
 * through a global mean, a per-image branch. Per element (pixel i = (b, y, x), channel c) ONE
 * fp64 accumulator starts from +0.0 and adds, in this order:
 *   1. the plain terms in index order: (double)E_j[i, c] -- the gradient a 1x1 branch sent down;
 *   2. the depthwise terms in index order, within a term the taps in ascending tap = 3 ky + kx:
 *      (double)w9c[tap, c] * (double)D[b, y - (ky-1) rate, x - (kx-1) rate, c], the product
 *      exact -- the mirrored tap of epos_depthwise_dgrad_f32. A tap whose source pixel lies
 *      outside the image adds +0.0 (never 0 * d);
 *   3. the per-image term: (double)Pool[b, c] / (double)pool_div, an IEEE fp64 division --
 *      the adjoint of a mean over pool_div pixels.
 *   The accumulator is rounded to fp32 once. With Y non-NULL the result is written as +0.0
 *   wherever Y[i, c] <= 0 (-0.0 counts, a NaN does not), the rule of epos_depthwise_dgrad_f32.
 *   EVERY element of the C columns is WRITTEN; padding columns are not touched. With one
 *   depthwise term and nothing else the bytes are those of epos_depthwise_dgrad_f32.
 *   One launch, no workspace, no atomics, no host synchronisation, capturable in a graph; the
 *   same bytes in every run, for an image alone and at any position of a batch.
 *   partition: how the elements are dealt to workgroups -- never what they hold. 0 = the one this
 *   build ships (EPOS_ASPP_JOIN_SHIPPED); the others are there to be measured against it
 *(tools/bench_aspp_chain.py). PIXEL: all channels of a pixel together, as
 *   epos_depthwise_dgrad_f32. SLICE32 / SLICE64: a workgroup owns 32 / 64 channels of 32 / 16
 *   consecutive pixels, and the workgroups of a slice have ids congruent mod 8, which the
 *   dispatcher has been seen to give to one XCD: a slice's nine taps are then re-read from that
 *   XCD's L2. SLICE32X2 / SLICE32X4: SLICE32 with two / four pixels a thread, 32 apart, which
 *   share each tap's weights. Nothing about the results depends on any of that.
 *   Refused with EPOS_E_INVALID before the launch, nothing written: null args or dX; B, H, W or
 *   C < 1; C % 4 != 0; too many pixels (epos_depthwise_dgrad_f32's limits); n_dw outside 0..4,
 *   n_plain outside 0..2; no term at all; a null D, w9c or E of a term counted; rate outside
 *   1..2^20; any ld < C or not a multiple of 4; pool_div < 1 with a Pool; a pointer that is not
 *   16-byte aligned; dX starting at an input; an unknown partition. */
#define EPOS_ASPP_JOIN_PIXEL 1
#define EPOS_ASPP_JOIN_SLICE32 2
#define EPOS_ASPP_JOIN_SLICE64 3
#define EPOS_ASPP_JOIN_SLICE32X2 4
#define EPOS_ASPP_JOIN_SLICE32X4 5
#define EPOS_ASPP_JOIN_SHIPPED EPOS_ASPP_JOIN_SLICE64
typedef struct EposAsppJoinDw {
  const float* D; int64_t ldd;  /* f32 [B,H,W,C], the gradient at the branch's pre-activation */
  const float* w9c;             /* f32 [9][C], the folded weights the forward reads */
  int32_t rate;
  int32_t reserved0;
} EposAsppJoinDw;
typedef struct EposAsppJoinPlain {
  const float* E; int64_t lde;  /* f32 [B,H,W,C] */
} EposAsppJoinPlain;
typedef struct EposAsppJoinArgs {
  int32_t B, H, W, C;
  int32_t n_dw, n_plain;
  EposAsppJoinDw dw[4];
  EposAsppJoinPlain plain[2];
  const float* Pool; int64_t ldp;   /* f32 [B][ldp] or NULL */
  int64_t pool_div;                 /* >= 1 with a Pool */
  const float* Y; int64_t ldy;      /* or NULL */
  float* dX; int64_t ldx;
  int32_t partition;                /* 0, or EPOS_ASPP_JOIN_* */
  int32_t reserved0;
} EposAsppJoinArgs;
int64_t epos_pool_broadcast_dgrad_range_pixels(int B, int64_t P, int C);
int64_t epos_pool_broadcast_dgrad_workspace_bytes(int B, int64_t P, int C);
int epos_pool_broadcast_dgrad_f32(const float* D, int64_t ldd, float* g, int64_t ldg, int B,
                                  int64_t P, int C, void* workspace /* or NULL */, void* stream);
int epos_aspp_join_dgrad_f32(const EposAsppJoinArgs* args, void* stream);

/* Weight update (csrc/weight_pack.hip; added without an ABI version change). The three host
 * packers above restated as device kernels, so that weights updated on the device (the momentum
 * step) reach a built plan without a round trip through the host: a grouped call packs fp32
 * matrices that live on the device into the buffers the plan's launches already point at.
 *
 * One problem = one matrix: the column window [col0, col0 + N) of W f32 [K][ldw] (row-major,
 * the checkpoint layout [1,1,K,N'] of a logits layer; K a multiple of 4, 4..1024; N >= 1) and
 * of bias f32 (bias[col0 + n]). Up to four destinations, each NULL = not wanted:
 *   plain     what epos_pack_pointwise_weights writes for that K x N window,
 *   split     what epos_pack_pointwise_weights_split writes,
 *   h2        what epos_pack_pointwise_weights_h2 writes, the round_up(N, 128) inverse scales
 *             behind the fragments included,
 *   bias_pad  round_up(N, 128) floats: the bias, then zeros.
 * Every byte of a destination is written (the zero padding of K and N too) and equals the host
 * packer's byte for finite weights; fp32-subnormal weights and residuals are kept. The inverse
 * scale is built from the exponent. A non-finite weight is packed only without an h2
 * destination; the NaN payloads of its split pieces are unspecified.
 *   Acceptance. A problem WITH an h2 destination is refused exactly when the host fp16-pair
 *   packer returns 0 for the window: a weight that is not finite, a column maximum whose scale
 *   2^e leaves |e| <= 100, or a weight that fails the packer's self-check
 *   |hi + mid 2^-11 - t| <= max(2^-22 |t|, 2^-36). A problem without h2 is never refused.
 *   All or nothing. status i32 [device, count]: 0 = written, non-zero = refused. If ANY problem
 *   of the call is refused, no destination byte of ANY problem of the call is written. The
 *   caller reads status when it chooses; nothing here waits for the device.
 *   Launches. One clear of status, then per 32 problems one checking launch (only when some
 *   problem has an h2 destination) and, behind ALL of those, one writing launch, in sequence on
 *   `stream`: no allocation, no synchronisation, integer atomics only, the same bytes in every
 *   run. One workgroup per (problem, 128 columns) reads its columns once for the column maxima
 *   and once through LDS for all layouts, and stores whole 1 KB fragments.
 *   Refused with EPOS_E_INVALID before anything is enqueued: a null table, count outside 0..256,
 *   a null or misaligned status, K / N / ldw / col0 out of range, a null W, bias_pad without
 *   bias, W or bias not 4-byte aligned, plain / split / h2 not 16-byte aligned (the GEMMs read
 *   them with 16-byte loads) or bias_pad not 4-byte aligned. Source and destinations must not
 *   overlap. count == 0 returns 0 and launches nothing. */
typedef struct EposWeightPackArgs {
  const float* W;          /* device f32 [K][ldw] */
  int64_t ldw;             /* col0 + N <= ldw <= 2^31 */
  int64_t col0;
  const float* bias;       /* device f32, NULL allowed when bias_pad is NULL */
  float* plain;
  void* split;
  void* h2;
  float* bias_pad;
  int32_t K, N;
} EposWeightPackArgs;
int epos_pack_weights_device_f32(const EposWeightPackArgs* args, int count, int32_t* status,
                                 void* stream);

/* Augmentation (csrc/augment.hip; added without an ABI version change). The seven training-time
 * image operations of the reference (epos_lib/datagen.py:629-670, epos_lib/augment.py), in
 * place on images f32 [device, B,h,w,3] with values in [0,255]. The table holds DRAWN values,
 * not ranges: the call is a pure function of its arguments.
 *
 * ops [HOST, B][n_ops], 0 <= n_ops <= 8, is read during the call (it travels in kernel
 * arguments) and may be reused on return. The ops of an image run in the order given, on
 * x = value / 255 (fp32, before the first op; the result is multiplied by 255 after the last).
 * An image whose ops are all NONE (or n_ops == 0) keeps its bytes.
 *   NONE                   skipped
 *   BRIGHTNESS  a = delta  clip(x + a, 0, 1)
 *   CONTRAST    a = factor clip((x - m_c) a + m_c, 0, 1), m_c = the mean of channel c over the
 *                          image as the preceding ops left it: fp64 sums of 64 fixed pixel
 *                          ranges, added in their order (no floating-point atomics)
 *   SATURATION  a = factor RGB -> HSV (hexcone; h = 0 where max = min), s = clip(s a, 0, 1),
 *                          HSV -> RGB, clip
 *   HUE         a = delta  RGB -> HSV, h = (h + a) mod 1 in [0,1), HSV -> RGB, clip
 *   BLUR        a = sigma  ksize = round_half_even(8 sigma + 1) | 1, R = (ksize - 1) / 2;
 *                          w_i = exp(-i^2 / (2 sigma^2)) / sum in fp64, rounded to fp32; rows,
 *                          then columns, fp32 accumulation from -R to R, BORDER_REFLECT_101, no
 *                          clip. sigma == 0 or ksize == 1: skipped. R > 32 or
 *                          R > min(h, w) - 1: refused
 *   NOISE       a = sigma  clip(x + a z, 0, 1); value i = (y w + x) 3 + c of the image takes
 *                          z(i) from Philox4x32-10 at counter (i / 4, 0, 0, 0), key (key_lo,
 *                          key_hi): u1 = ((r0 >> 8) + 0.5) 2^-24, u2 = (r1 >> 8) 2^-24,
 *                          z(4j) = sqrt(-2 ln u1) cos(2 pi u2), z(4j+1) = ... sin(2 pi u2),
 *                          z(4j+2), z(4j+3) the same from (r2, r3)
 *   JPEG        a = quality (an integer, 1..100) a round trip through 8-bit baseline JPEG with
 *                          4:2:0 chroma: v = min(255, floor(x 255.5)), the IJG 16-bit fixed-point
 *                          colour transforms, luma padded to 16 by replication, 2x2 chroma
 *                          means with the alternating bias (of pixels replicated to 16 columns
 *                          and an even number of rows; below that the last chroma row is
 *                          replicated), the 8x8 DCT in fp64, the Annex K
 *                          tables at the IJG quality scaling, "fancy" triangle chroma
 *                          upsampling, x = v / 255 ("Augmentation", has each step)
 * Nothing synchronises and nothing is allocated: every launch is enqueued on `stream`, and
 * the number of launches does not depend on B up to 8 (images go into the grid in chunks of 8).
 * The same arguments give the same bytes in every run and at every position of a batch.
 * work: epos_augment_workspace_bytes(B, h, w) bytes on the device, 16-byte aligned; may be NULL
 * when no op is a CONTRAST, a BLUR or a JPEG.
 *   Refused with EPOS_E_INVALID before the first launch: B < 0, h or w < 1, h w 3 >= 2^31,
 *   n_ops outside 0..8, null images or ops (when B and n_ops are positive), images not 4-byte
 *   aligned, an unknown kind, a parameter that is not finite, a negative sigma, a blur radius
 *   out of range, a quality that is no integer in 1..100, a missing or misaligned workspace. */
#define EPOS_AUG_NONE 0
#define EPOS_AUG_BRIGHTNESS 1
#define EPOS_AUG_CONTRAST 2
#define EPOS_AUG_SATURATION 3
#define EPOS_AUG_HUE 4
#define EPOS_AUG_BLUR 5
#define EPOS_AUG_NOISE 6
#define EPOS_AUG_JPEG 7
typedef struct EposAugmentOp {
  int32_t kind;
  float a, b;              /* b: reserved, ignored */
  uint32_t key_lo, key_hi;
} EposAugmentOp;
int64_t epos_augment_workspace_bytes(int B, int h, int w);
int epos_augment_f32(float* images, int B, int h, int w, const EposAugmentOp* ops, int n_ops,
                     void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* EPOS_HIP_H_ */
