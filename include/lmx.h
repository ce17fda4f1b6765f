/*
 * lmx.h — C-ABI of liblmx.so, the MI355X (gfx950) feature-extraction kernels that sit behind the
 * yolo-pipeline / sam3-pipeline / dinov3-pipeline services of UBC-AWP/vision-sam3-yolo-lameless.
 *
 * The reference has no FFI of its own (it is pure Python: SURVEY.md §8b); the seam it offers is the three
 * third-party call sites
 *     services/yolo-pipeline/app/main.py:76      self.yolo_model(frame, verbose=False, conf=...)
 *     services/sam3-pipeline/app/main.py:80-88   predictor.set_image(image); predictor.predict(box=...)
 *     services/dinov3-pipeline/app/main.py:107-113  processor(images=...); model(**inputs).last_hidden_state.mean(1)
 * Every entry point below replaces a piece of the arithmetic that runs under one of those calls; the comment
 * on each one says which.  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no C++ or torch types; every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only enqueue work;
 *   - return 0 on success, <0 on error; lmx_last_error() returns the thread-local message;
 *   - activations are NHWC / token-major with the channel dimension contiguous, f16 unless said otherwise,
 *     accumulation is always f32 (MFMA f32 accumulators), the ViT residual stream is f32;
 *   - all "ld*" strides are in ELEMENTS of the tensor's dtype.
 */
#ifndef LMX_H
#define LMX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LMX_VERSION 100

/* error codes */
#define LMX_OK 0
#define LMX_EINVAL (-1)  /* bad argument / unsupported shape (message says which) */
#define LMX_EHIP (-2)    /* a HIP runtime call failed */

typedef void* lmx_stream_t;

int lmx_version(void);
const char* lmx_last_error(void);
/* number of visible HIP devices, <0 on error (used by the loader to fail loudly on a GPU-less box) */
int lmx_device_count(void);

/* ---- dtypes / activations -------------------------------------------------------------------------- */
enum { LMX_F16 = 0, LMX_F32 = 1 };
enum { LMX_ACT_NONE = 0, LMX_ACT_SILU = 1, LMX_ACT_GELU = 2 /* erf form */, LMX_ACT_RELU = 3,
       LMX_ACT_SWIGLU = 4 /* lmx_k_gemm only: gated epilogue, see there */ };

/* ---- K3/K12/K2: GEMM / 1x1 conv / 3x3 conv (implicit GEMM), f16 in, f32 MFMA accumulate ------------
 * C[m][n] = res[m][n] + scale[n] * act( sum_k A[m][k] * W[n][k] + bias[n] )
 * Replaces: torch Linear / Conv2d(+folded BN)+SiLU under ultralytics' C2f/Conv/Detect (yolo main.py:76),
 * the ViT qkv/proj/fc1/fc2 Linears under segment_anything's ImageEncoderViT (sam3 main.py:80) and under
 * transformers' Dinov2/DINOv3 layers (dinov3 main.py:110-111).
 *   a_mode 0: A is a row-major [M][K] f16 matrix with row stride lda.
 *   a_mode 1: A is generated on the fly from an NHWC f16 image batch X[n][H][W][*] (pixel stride lda,
 *             Cin channels used): kernel 3x3, pad 1, stride conv_stride; M = n*Ho*Wo, K = 9*Cin,
 *             k = (ky*3+kx)*Cin + ci  (weights must be packed in that order).
 *   a_mode 2: "pooled rows" — A is a row-major [M][K] matrix whose rows are an [n][H][W_] token grid (H, W_ even), and C is
 *             the 2 x 2 max-pool of the product over that grid: [M/4][N] (f32 or f16) in [n][H/2][W_/2] order, the bits of a_mode 0
 *             followed by lmx_k_maxpool2 without the full-size intermediate (Hiera's `do_pool(self.proj(x))` at the stage
 *             transitions, TF:models/sam2/modeling_sam2.py Sam2MultiScaleBlock, and of the pooled queries).  No
 *             residual / scale / activation; M >= 512, N >= 96, N%8==0 (the LDS-DMA kernel); A smaller than 2 GB.
 * W is f16 [N][K] (K contiguous).  Requirements: K%8==0, N%4==0, lda%8==0, Cin%8==0, 16-byte aligned bases.
 *
 * act = LMX_ACT_SWIGLU (the gated MLPs of DINOv3 ViT-S+/H+ `down(silu(gate(x)) * up(x))`, TF:models/dinov3_vit/modeling_dinov3_vit.py
 * DINOv3ViTGatedMLP, and of DINOv2 giant, TF:models/dinov2/modeling_dinov2.py Dinov2SwiGLUFFN): W holds the gate AND the up
 * projection, N = 2 I rows interleaved in blocks of 16 — rows 32t .. 32t+15 are gate rows 16t .. 16t+15, rows 32t+16 .. 32t+31
 * the up rows of the same channels (lmx/dino.py pack_gated) — and bias [N] is interleaved the same way.  Then
 *   C[m][j] = scale[j] * ( silu(acc[m][g(j)] + bias[g(j)]) * (acc[m][u(j)] + bias[u(j)]) ),  g(j) = 32 (j / 16) + j % 16, u(j) = g(j) + 16
 * N in the descriptor stays the GEMM's N (2 I); C HAS N / 2 COLUMNS (ldc >= N / 2) and scale, if given, N / 2 entries.  The
 * 2 I-wide intermediate is never written.  f32 accumulator + f32 bias, silu and the product in f32, ONE rounding to f16 — in
 * every kernel variant, so a row's bits do not depend on M.  a_mode 0 and f16 output only, N%32==0, no residual, a_rep or split_k.
 */
typedef struct {
  const void* A;
  const void* W;
  const float* bias;   /* [N] or NULL */
  const float* scale;  /* [N] or NULL (LayerScale) */
  const void* res;     /* [M][N] residual of dtype out_dtype, row stride ldr, or NULL; may alias C */
  void* C;
  int64_t lda, ldc, ldr;
  int32_t M, N, K;
  int32_t act;
  int32_t out_dtype;   /* LMX_F16 / LMX_F32 */
  int32_t a_mode;
  /* a_mode 1 (all six); a_mode 2 (H, W_: the token grid) */
  int32_t H, W_, Cin, conv_stride, Ho, Wo;
  /* residual broadcast: if res_rows > 0 the residual row is (m % res_rows) — e.g. a position table [tokens][N]
   * added to every image of the batch (Hiera patch embed + pos_embed, TF sam2 :661-662) */
  int32_t res_rows;
  /* a_mode 0 only: A's K columns are read a_rep times (0 / 1: once): K = a_rep * Ka, k-tile kt takes A columns (kt*BK) mod Ka
   * and W columns kt*BK.  With W = [whi | wlo] (a_rep 2) ONE launch accumulates a.whi + a.wlo: f16 activations against
   * 22-bit weights (the exact plan of the SAM ViT encoder, lmx/sam.py).  Ka % 64 == 0; the LDS-DMA kernel's shapes only. */
  int32_t a_rep;
  /* split-K for long-K, few-tile problems (the exact plan's 3 x 3 convolutions at 10 frames: K = 27 Cin against a few dozen
   * tiles on 256 CUs): split_k = S >= 2 cuts the k range into S parts, part s writes ITS partial sum to C + s * split_stride
   * (elements).  f32 output, no activation, a_mode 0 or 1 on the LDS-DMA kernel's shapes only; bias and residual enter partial 0,
   * `scale` applies to every partial (the epilogue is linear), and the consumer adds the S partials in a fixed order
   * (lmx_k_split3's `nsum`): deterministic, unlike atomics.  0 / 1: no split. */
  int32_t split_k;
  int64_t split_stride;
  /* the LayerNorm that reads the result, from the same launch (ln_out != NULL): besides C, the kernel writes
   *   ln_out[m][n] = f16( (C[m][n] - mean_m) * rstd_m * ln_gamma[n] + ln_beta[n] ),  rstd_m = 1 / sqrt(var_m + ln_eps)
   * (f16 [M][N], row stride ld_ln) from the f32 values it stores to C: mean first, then the centred squares, both summed in
   * lmx_k_layernorm's order — the bits of lmx_k_layernorm on C without the second pass over it.  A workgroup must hold whole
   * rows for this, so the request has a kernel of its own (route dma_128xrow_ln: 128 rows x N tiles) FOR EVERY M — a layer's
   * choice, never the batch's — and only for: f32 C with a residual (no res_rows), N <= 448, N%16==0, K <= 448, a_mode 0, no
   * activation / scale / a_rep / split_k.  C's bits are those of the same descriptor without ln_out.  Any other request that
   * carries ln_out is LMX_EINVAL.  (Hiera stage 3: the attention projection writes layer_norm2's rows.) */
  void* ln_out;
  const float* ln_gamma; /* [N], 16-byte aligned */
  const float* ln_beta;  /* [N], 16-byte aligned */
  int64_t ld_ln;
  float ln_eps;
} lmx_gemm_desc;
int lmx_k_gemm(const lmx_gemm_desc* d, lmx_stream_t stream);
/* development hook (tools/gemm_sweep.py): force one tiling of the LDS-DMA GEMM for every following launch; v = 0 restores
 * the launcher's per-shape choice, otherwise one of the letters documented at lmx_gemm2_launch (csrc/gemm2.hip) */
void lmx_dbg_set_gemm2_variant(int v);
/* ---- which kernel would run: lmx_h_gemm_route, lmx_h_attn_route (below, at lmx_k_attention) and lmx_h_layernorm_route.
 * lmx_k_gemm, lmx_k_attention and lmx_k_layernorm validate and choose their kernel in one pure host function each and launch in
 * another; these three entry points run the first half alone.  They NEVER touch the GPU and NEVER dereference the operand pointers
 * (null and alignment checks only: any non-null, suitably aligned address will do), so they work on a host without a device.
 * An invalid descriptor returns what the launcher returns for it, with the same lmx_last_error text; otherwise LMX_OK and, in
 * name[cap], the route: the kernel and the template arguments of the instantiation, e.g.
 *   GEMM        v1_128x64 (register-staged, BM x BN) | dma_256x256x64_s2, dma_256x128x64_s3_stag (LDS-DMA: BM x BN x BK, ring slots,
 *               staggered wave groups) | dma_128xrow_ln (ln_out: 128 rows x the whole row)
 *   attention   small | sp_qb2_ones | spp_dot2 | gp4_ones | tiled_q2_dot2_rel_hd64, tiled_q2_ones_dma_hd64 (ones / dot2: how the
 *               row sums are taken; q: 16-query blocks per wave; hd: the LDS row class)
 *   LayerNorm   narrow | rows_it2 | row_it16 (it: float4 per lane)
 * The development switches (LMX_GEMM_*, LMX_GEMM2_*, LMX_ATTN_*, LMX_LN_ONE_ROW, lmx_dbg_set_gemm2_variant) steer the answer as
 * they steer the launch.  LMX_EINVAL too if the name does not fit cap bytes. */
int lmx_h_gemm_route(const lmx_gemm_desc* d, char* name, int cap);

/* ---- K11: LayerNorm over the last dim, f32 or f16 in -> f16 or f32 out ------------------------------
 * Replaces torch.nn.LayerNorm inside the ViT blocks (TF:models/dinov3_vit/modeling_dinov3_vit.py:400-445,
 * TF:models/sam/modeling_sam.py:891-972).  One 64-lane wave per row, wave-shuffle reductions, two-pass
 * variance (mean first) in f32.  D%4==0, D<=4096.
 */
int lmx_k_layernorm(const void* x, int in_dtype, int64_t ldx, const float* gamma, const float* beta,
                    void* y, int out_dtype, int64_t ldy, int rows, int D, float eps, int act, lmx_stream_t stream);
/* (act = LMX_ACT_NONE or LMX_ACT_GELU applied after the affine: the SAM decoder's LayerNorm2d -> GELU, TF sam :523) */
int lmx_h_layernorm_route(int in_dtype, int out_dtype, int rows, int D, int act, char* name, int cap); /* see lmx_h_gemm_route */

/* ---- the gate of a gated MLP as its own pass: out[r][j] = f16( silu(gu[r][j]) * gu[r][I + j] ), gu f16 [rows][2 I] (gate columns
 * first, row stride ldg), out f16 [rows][I] (row stride ldo); I%8==0.  The unfused form of LMX_ACT_SWIGLU — plain GEMM to a 2 I-wide f16
 * buffer, then this — which rounds gate and up to f16 before the product: kept as the timing reference of the fused epilogue
 * (tools/swiglu_timing.py); the DINO plan always uses the epilogue. */
int lmx_k_swiglu(const void* gu, int64_t ldg, void* out, int64_t ldo, int rows, int I, lmx_stream_t stream);

/* ---- K11 + K8-K10 + K14 for Hiera's 8 x 8-token windows: x += proj(window_attention(qkv(layer_norm1(x)))) as one kernel ---------
 * Replaces, for the blocks of Hiera-B+ stage 1 (D = 112, 2 heads; TF:models/sam2/modeling_sam2.py Sam2MultiScaleBlock.forward,
 * Sam2MultiScaleAttention :350-409 with window_partition / window_unpartition :412-455), the four launches LayerNorm -> qkv GEMM ->
 * window attention -> projection GEMM (+ residual) and their f16 intermediates: per token it reads the f32 stream (4D bytes) and
 * writes it (4D).  x f32 [rows, ldx] updated in place; rows = n_img * Gh * Gw, Gh and Gw multiples of 8 (no padded windows).
 * h = NULL: the kernel normalises x itself (gamma, beta f32 [D], eps: layer_norm1); h = f16 [rows, D] contiguous: layer_norm1(x) as
 * written by the previous block's lmx_k_ln_mlp (h_next), read instead (+ 2D bytes per token; wqkv_p's columns then in natural order:
 * cheaper when the rows exist anyway, because the kernel's first products then do not wait for the f32 rows).  Packed operands (lmx/sam.py pack_hiera_attn): wqkv_p f16 [3*heads*64, 128] — sections
 * q | k | v, each head padded from 56 to 64 rows; v's row 63 of every head is zero with bias 1 (the softmax sum rides the PV
 * product); columns in MFMA k-slot order (position 32s + 8g + 4h + i holds input feature 16(2s+h) + 4g + i, zeros past D) —
 * bqkv_p f32 [3*heads*64], wo_p f16 [D, heads*64] with the 64 columns of a head in the same order, bo f32 [D].
 * scale = head_dim ** -0.5.  Rounding points as in the unfused chain: LayerNorm output, q, k, v, P, attention output f16; sums f32. */
int lmx_k_hiera_attn8(const void* h, float* x, int64_t ldx, const float* gamma, const float* beta, float eps, const void* wqkv_p,
                      const float* bqkv_p, const void* wo_p, const float* bo, int n_img, int Gh, int Gw, int D, int heads, float scale,
                      lmx_stream_t stream);

/* The same for Hiera-B+ stage 2 (D = 224, 4 heads of 56, 4 x 4-token windows; blocks whose input and output widths are equal): the
 * three launches qkv GEMM -> window attention -> projection GEMM (+ residual) as one kernel whose weights stream through an LDS ring
 * (csrc/hiera.hip).  h f16 [rows, D] contiguous = layer_norm1(x) (the previous block's lmx_k_ln_mlp leaves it as h_next); x f32
 * [rows, ldx] updated in place; rows = n_img * Gh * Gw, Gh and Gw multiples of 4.  w_img f16 [16][16384]: per head h the LDS
 * images of its q, k, v (64 rows x 512 B, 16-byte chunk c of row r at c ^ (r & 15), rows >= 56 zero, v's row 63 zero with bias 1)
 * and projection (256 rows x 128 B, chunk c of row r at c ^ ((r >> 1) & 7), the head's 64 input columns in MFMA k-slot order)
 * matrices at index 4 h + {0, 1, 2, 3}; bias f32 [4][q | k | v][64] then the projection's [224] (lmx/sam.py pack_hiera_attn4). */
int lmx_k_hiera_attn4(const void* h, float* x, int64_t ldx, const void* w_img, const float* bias, int n_img, int Gh, int Gw, int D,
                      int heads, float scale, lmx_stream_t stream);

/* The blocks that open Hiera-B+ stage 2 (112 -> 224 channels, 4 heads of 56; keys / values the 64 tokens of an 8 x 8 window) and stage 3
 * (224 -> 448, 8 heads; 16 tokens of a 4 x 4 window), queries and shortcut the 2 x 2 max-pools of the window's tokens
 * (TF:models/sam2/modeling_sam2.py Sam2MultiScaleBlock.forward with dim != dim_out and q_stride): shortcut GEMM + pool, q GEMM + pool,
 * k | v GEMM, window attention with pooled queries, projection GEMM + residual as one kernel (csrc/hiera.hip; weights streamed).
 * h f16 [n_img*Gh*Gw, Din] contiguous = layer_norm1(x); out f32 [n_img*(Gh/2)*(Gw/2), Dout] contiguous (written, not accumulated);
 * Gh, Gw multiples of the window side.  w_img f16 [14 | 47][16384]: LDS images in streaming order — 112 -> 224: shortcut rows
 * 0..127, shortcut rows 128..223, then per head [q | k] (2 x 64 rows of 256 B), [v | unused], projection columns of the head (256
 * rows of 128 B, k-slot order); 224 -> 448: shortcut in 7 images of 64 rows (512 B rows), then per head q, k, v (64 rows each) and
 * the head's projection columns for output rows 0..223 and 224..447 —, bias f32 [shortcut + projection: Dout | heads x (q | k | v)
 * x 64 (| Dout zeros for 112 -> 224)] (lmx/sam.py pack_hiera_attn_pool). */
int lmx_k_hiera_attn_pool(const void* h, float* out, const void* w_img, const float* bias, int n_img, int Gh, int Gw, int Din, int Dout,
                          int heads, float scale, lmx_stream_t stream);

/* ---- K11+K12 for narrow widths: x += fc2(gelu(fc1(LayerNorm(x)))) without the 4D-wide hidden tensor ever reaching HBM ----
 * Replaces `hidden_states + self.mlp(self.layer_norm2(hidden_states))` of the Hiera blocks whose width is 112 or 224
 * (TF:models/sam2/modeling_sam2.py Sam2MultiScaleBlock.forward; stages 1-2 of Hiera-B+), where the unfused
 * LN -> GEMM -> GEMM chain is bound by its HBM intermediates (32*D bytes/token against 16*D here).
 * Two launches: the LayerNorm kernel (f32 stream -> f16 rows in `workspace`, rows*D*2 bytes), then the fused MLP + residual.
 * x f32 [rows, ldx] updated in place; w1 f16 [4D, D], b1 f32 [4D], w2 f16 [D, 4D], b2 f32 [D] (torch Linear layouts).
 * Rounding points match the unfused kernels: LN output and GELU output are rounded to f16, accumulation is f32.
 */
int lmx_k_ln_mlp(float* x, int64_t ldx, const float* gamma, const float* beta, const void* w1, const float* b1,
                 const void* w2, const float* b2, int64_t rows, int D, float eps, void* workspace, void* x16,
                 const float* gamma_next, const float* beta_next, void* h_next, lmx_stream_t stream);
/* The same operation with the weights as host-made LDS images streamed in steps of 64 hidden units by a workgroup of 8 waves x 32
 * tokens (csrc/hiera.hip hiera_mlp_kernel: half the L2 -> LDS traffic and a quarter to a half of the barriers of the kernel above;
 * layer_norm2 always inside).  w_img f16 [7 | 28][16384] for D = 112 | 224: per step the 64 rows of W1 (256 | 512-byte rows, the D
 * input columns in MFMA k-slot order, chunk c of row r at c ^ (r & 15)) and the D rows x 64 columns of W2 (128-byte rows, columns
 * in k-slot order, chunk c of row r at c ^ ((r >> 1) & 7); D = 112: in the same image at byte 16384, D = 224: the next image);
 * bias f32 [b1 (4D) | b2 | gamma2 | beta2 | gamma_next | beta_next (D each; the last two unused without h_next)] (lmx/sam.py
 * pack_ln_mlp).  x16, h_next: as below. */
int lmx_k_ln_mlp_img(float* x, int64_t ldx, const void* w_img, const float* bias, int64_t rows, int D, float eps, void* x16, void* h_next,
                     lmx_stream_t stream);
/* x16: NULL, or f16 [rows, D] (contiguous) that receives a copy of the updated x — the input of the FPN's lateral 1x1
 * convolution after a stage's last block, which otherwise costs a cast pass over the f32 stream.
 * h_next: NULL, or f16 [rows, D] that receives LayerNorm(updated x; gamma_next, beta_next, eps) — the NEXT block's
 * `layer_norm1(hidden_states)`, computed on the rows while they are still in registers instead of by a LayerNorm launch
 * that reads the f32 stream again */

/* ---- K13/K14: attention (flash-style, online softmax in f32, S and PV on MFMA) ----------------------
 * O[b,t,h,:] = softmax_j( scale * Q[b,t,h,:] . K[b,j,h,:] ) V[b,j,h,:]
 * Q/K/V/O are f16 with the head dim contiguous; element (row r, head h, d) sits at base + r*ld + h*hd + d
 * where r is the token row.  geometry:
 *   mode 0 (flat):    row = b*T + t                     (Tq queries, Tk keys per batch element)
 *   mode 1 (window):  K/V tokens live on a [Gh][Gw] grid per image, partitioned into ws x ws windows
 *                     (grid zero-padded up to a multiple of ws, as ImageEncoderViT.window_partition does);
 *                     b = (img, wy, wx); key t -> (wy*ws + t/ws, wx*ws + t%ws).  Keys that fall in the
 *                     padding take K = pad_k[h], V = pad_v[h] (= the qkv bias: what Linear(0) yields).
 *                     Queries use the same map on a grid subsampled by q_stride (1, or 2 for Hiera Q-pool):
 *                     grid [Gh/q][Gw/q]... see DESIGN.md §attention.
 * hd % 8 == 0, hd <= 96 (head dims up to 64 use 64-half LDS rows; 72..96 — SAM ViT-H's 80 — the 128-half class).
 * Three kernels behind the one entry point, chosen from the shape: tiles of 64 keys with an online softmax (any length;
 * LDS-DMA ring for long flat sequences), whole-sequence tiles for 128 < Tk <= 208 (single-pass softmax), one wave per
 * item for Tq, Tk <= 16.
 */
typedef struct {
  const void* Q; const void* K; const void* V; void* O;
  int64_t ldq, ldk, ldv, ldo;   /* token-row strides (elements) */
  int32_t B, H, Tq, Tk, hd;
  float scale;
  int32_t mode;
  /* mode 1 */
  int32_t Gh, Gw, ws, q_stride;
  const void* pad_k; const void* pad_v; /* f16 [H*hd] or NULL (zeros) */
  /* decomposed relative-position bias of SAM v1's ImageEncoderViT (TF sam :761-801): rel f16 [B*H*Tq][2*rel_S] from
   * lmx_k_relpos_tables; score(q, key (ky,kx)) += rel[q][ky] + rel[q][rel_S + kx], key t -> (t / rel_S, t % rel_S).
   * NULL = no bias.  Requires Tk == rel_S*rel_S and q_stride 1. */
  const void* rel; int32_t rel_S;
} lmx_attn_desc;
int lmx_k_attention(const lmx_attn_desc* d, lmx_stream_t stream);
int lmx_h_attn_route(const lmx_attn_desc* d, char* name, int cap); /* see lmx_h_gemm_route */
/* rel[(b*H+h)*T + t][j]      = sum_c q[b,t,h,c] * rel_pos_h[ty - j + S-1][c]        (j < S)
 * rel[(b*H+h)*T + t][S + j]  = sum_c q[b,t,h,c] * rel_pos_w[tx - j + S-1][c]        (t = ty*S + tx, T = S*S)
 * q addressed with the attention geometry of `d` (mode 0 or window mode; d->Q, ldq, B, H, Tq, hd, mode, Gh, Gw, ws used),
 * rel_pos_h / rel_pos_w f32 [2S-1][hd] (get_rel_pos without interpolation: q_size == k_size), out f16. */
int lmx_k_relpos_tables(const lmx_attn_desc* d, const float* rel_pos_h, const float* rel_pos_w, int S, void* out,
                        lmx_stream_t stream);

/* ---- DINOv3 RoPE on the patch tokens of Q and K, in place (TF dinov3_vit :238-268) ------------------
 * x[b, t, h, :] for t >= n_prefix is rotated: x' = x*cos + rotate_half(x)*sin with cos/sin f32 [T-n_prefix][hd].
 */
int lmx_k_rope(void* x, int64_t ld, int B, int T, int H, int hd, int n_prefix, const float* cos_t,
               const float* sin_t, lmx_stream_t stream);

/* ---- K9/K21: Pillow-exact separable u8 resize (two passes, 8bpc fixed-point coefficients) -----------
 * Reproduces PIL.Image.resize(..., BICUBIC|BILINEAR, reducing_gap=None) on RGB u8 — the resampler behind
 * AutoImageProcessor (dinov3 main.py:107) and SamPredictor.set_image -> ResizeLongestSide (sam3 main.py:80).
 * Coefficient tables are computed on the host by the caller (lmx/resample.py restates Pillow's
 * precompute_coeffs / normalize_coeffs_8bpc): bounds[2*out] = (xmin, xsize), kk[out*ksize] int32.
 * Pass H: src [n][sh][sw][3] u8 -> tmp [n][sh][dw][3] u8 ; pass V: tmp -> dst [n][dh][dw][3] u8.
 * swap_rb swaps channel 0 and 2 while reading src (cv2 BGR frame -> RGB, dinov3 main.py:98-99).
 */
int lmx_k_pil_resize_h(const uint8_t* src, uint8_t* dst, int n, int sh, int sw, int dw, const int32_t* bounds,
                       const int32_t* kk, int ksize, int swap_rb, lmx_stream_t stream);
int lmx_k_pil_resize_v(const uint8_t* src, uint8_t* dst, int n, int sh, int dh, int w, const int32_t* bounds,
                       const int32_t* kk, int ksize, lmx_stream_t stream);

/* crop + /255 + (x-mean)/std + write the ViT patch matrix directly (im2col of the k=P,s=P patch conv):
 * out[(n*gh + py)*gw + px][(ky*P + kx)*3 + c] f16 (row stride ldo >= P*P*3; columns beyond P*P*3 are not
 * written — the caller zeroes them once when ldo pads K to a multiple of 8), from u8 img [n][ih][iw][3] cropped
 * at (top,left) to gh*P x gw*P.  (BitImageProcessor center_crop/rescale/normalize + Dinov*PatchEmbeddings' conv as a GEMM.)
 * lut: DEVICE f32 [3][256], lut[c][u] = normalised value of byte u in channel c (built on the host with the
 * processor's own expression, so rescale+normalize is exact by construction). */
int lmx_k_patchify_norm(const uint8_t* img, void* out, int n, int ih, int iw, int top, int left, int gh, int gw,
                        int P, int64_t ldo, const float* lut, lmx_stream_t stream);

/* DINOv3ViTImageProcessor (`AutoImageProcessor.from_pretrained` of a dinov3_vit directory, dinov3 main.py:34 / :107) in ONE
 * pass: u8 -> float32, * rescale, antialiased float32 resize of the WHOLE frame to gh*P x gw*P (width, then height, f32
 * intermediate: torch F.interpolate(antialias=True) on a CPU float tensor, which torchvision's resize calls), (x - mean) / std,
 * rounded to f16 and written as the patch matrix in lmx_k_patchify_norm's layout (columns beyond P*P*3 are not written).
 * src u8 [n][sh][sw][3]; swap_rb: src is BGR (cv2), the model's channel order and mean / std are RGB.
 * Tables from the host (lmx/resample.py aa_tables, ATen's float32 arithmetic), on the DEVICE: bounds_*[2*out] = (first
 * source index, taps), kk_*[out*ksize_*] f32 weights; bounds_h / kk_h have gw*P rows over sw, bounds_v / kk_v gh*P rows over
 * sh.  A centre crop is a slice of the tables.  seg_cols: the most source columns any run of 256 consecutive output columns
 * (starting at a multiple of 256) reads — the LDS segment, at most 5460.  mean_std: HOST float[6] = mean[3], std[3]. */
int lmx_k_float_resize_patchify(const uint8_t* src, void* out, int n, int sh, int sw, int gh, int gw, int P, int64_t ldo,
                                const int32_t* bounds_h, const float* kk_h, int ksize_h, const int32_t* bounds_v,
                                const float* kk_v, int ksize_v, int seg_cols, float rescale, const float* mean_std,
                                int swap_rb, lmx_stream_t stream);

/* ---- frames from a decoder: YUV 4:2:0 (NV12 / I420) -> packed BGR u8 [n][h][w][3], the format every entry point here takes ------
 * Replaces the colour conversion `cv2.VideoCapture.read()` hides in front of yolo main.py:76, sam3 main.py:80 and dinov3 main.py:98-99:
 * a software H.264 decoder leaves planar I420, a hardware decoder (VCN through rocDecode or VA-API) a pitched NV12 surface.  The
 * arithmetic is the public integer form of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420) — limited range, 20-bit fixed point, nearest
 * chroma — and is defined HERE (cv2 is not installed: PARITY UNPINNED against real OpenCV and swscale).  For pixel (x, y), h and w even:
 *   Y = y[y * pitch_y + x];  NV12: U = u[(y >> 1) * pitch_c + 2 * (x >> 1)], V = the byte after it;
 *                            I420: U = u[(y >> 1) * pitch_c + (x >> 1)],     V = v[the same offset]
 *   yy = max(0, Y - 16) * CY;  B = sat8((yy + CUB * (U - 128) + 2^19) >> 20)                      (signed 32-bit, arithmetic shift)
 *   G = sat8((yy + CUG * (U - 128) + CVG * (V - 128) + 2^19) >> 20);  R = sat8((yy + CVR * (V - 128) + 2^19) >> 20);  out = (B, G, R)
 *   CY, CUB, CUG, CVG, CVR = round(c * 2^20) of 1.164, 2.018, -0.391, -0.813, 1.596 (LMX_YUV_BT601, cv2's constants: 1220542, 2116026,
 *   -409993, -852492, 1673527) or of 1.164, 2.112, -0.213, -0.533, 1.793 (LMX_YUV_BT709: 1220542, 2214593, -223347, -558891, 1880097).
 * Frame i of a plane starts stride_y (y) / stride_c (u, v) bytes behind frame i - 1.  Any pointer alignment and any pitch; where a
 * 2-row x 16-column block's addresses are 16-byte aligned it moves as 16-byte loads and stores (csrc/yuv.hip), the same bytes either
 * way.  The descriptor is HOST memory, read during the call; the pointers in it are device memory (lmx_k_) or host memory (lmx_h_,
 * csrc/host_yuv.cpp: the plain C++ restatement).  n = 0 launches nothing.  Refused with LMX_EINVAL, never approximated: odd sizes or
 * sizes below 2, a pitch below the row, a layout or matrix outside the enums (full range, NV21, 4:2:2 and 10-bit have no value here),
 * NV12 with v != NULL, I420 with v == NULL. */
enum { LMX_YUV_NV12 = 0, LMX_YUV_I420 = 1 };
enum { LMX_YUV_BT601 = 0, LMX_YUV_BT709 = 1 };
typedef struct { const uint8_t *y, *u, *v;      /* NV12: u = the interleaved plane, v = NULL */
                 int64_t pitch_y, pitch_c;      /* bytes per row; >= w, and >= w (NV12) or w/2 (I420) */
                 int64_t stride_y, stride_c;    /* bytes from frame i to frame i+1 in each allocation */
                 int32_t layout, matrix; } lmx_yuv_frames_t;
int lmx_k_yuv420_to_bgr(const lmx_yuv_frames_t* frames_host, int n, int h, int w, uint8_t* bgr /* [n][h][w][3] */, lmx_stream_t stream);
int lmx_h_yuv420_to_bgr(const lmx_yuv_frames_t* frames_host, int n, int h, int w, uint8_t* bgr_host /* [n][h][w][3] */);

/* ---- the crop window: a part of every frame of a 4:2:0 clip -> packed BGR u8 [n][roi.h][roi.w][3] ---------------------------------
 * What video-preprocessing main.py:112-119 (moviepy's crop) cuts out of the decode, without its libx264 re-encode and second decode:
 * the pipelines run on the window of the ORIGINAL frames.  A window is lmx_rect_t {x, y, w, h} inside the h x w source frame; output
 * pixel (i, j) of the window is EXACTLY pixel (x + i, y + j) of the text above, its chroma taken from ((y + j) >> 1, (x + i) >> 1) of
 * the source.  x, y, w and h may have any parity; the source frame still has even sizes.  The window that covers the whole frame
 * gives the bytes of lmx_k_yuv420_to_bgr.  PARITY UNPINNED against real OpenCV and swscale, as above.  The kernel lays its 2-row x
 * 16-column blocks on the source's chroma grid (columns at multiples of 16 of the source, row pairs 2k and 2k + 1), so the loads of an
 * aligned surface stay 16-byte loads for any window; a block on the window's rim has one live row or starts / ends inside a chroma
 * pair.  Refused with LMX_EINVAL: everything lmx_k_yuv420_to_bgr refuses, an empty window (w or h below 1) and a window that leaves
 * the frame (x or y below 0, x + w above the frame's w, y + h above its h).  n = 0 launches nothing. */
typedef struct { int32_t x, y, w, h; } lmx_rect_t;
int lmx_k_yuv420_to_bgr_roi(const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host,
                            uint8_t* bgr /* [n][roi.h][roi.w][3] */, lmx_stream_t stream);
int lmx_h_yuv420_to_bgr_roi(const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host,
                            uint8_t* bgr_host /* [n][roi.h][roi.w][3] */);

/* ---- frames to an encoder: packed BGR u8 -> YUV 4:2:0 (NV12 / I420) ---------------------------------------------------------------
 * What swscale does between a BGR frame and libx264 / a hardware encoder (video-preprocessing main.py:122-127, clip-curation's
 * writer): limited range, BT.601 or BT.709, 20-bit fixed point, chroma from the 2 x 2 BOX (not the top-left sample).  The arithmetic is
 * defined HERE (neither cv2 nor swscale is installed: PARITY UNPINNED against both).  h and w are even and at least 2; all arithmetic is
 * signed 32-bit and >> is an arithmetic shift (floor):
 *   Y(x, y) = sat8(((YB*B + YG*G + YR*R + 2^19) >> 20) + 16)
 *   SB, SG, SR = sums of B, G, R over pixels (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1)                       (0 .. 1020)
 *   U(i, j) = sat8(((UB*SB + UG*SG + UR*SR + 2^21) >> 22) + 128);  V(i, j) = sat8(((VB*SB + VG*SG + VR*SR + 2^21) >> 22) + 128)
 *   NV12: c[j * pitch_c + 2 * i] = U, the byte after it V;  I420: u[j * pitch_c + i] = U, v[the same offset] = V
 * Every coefficient is round(c * 2^20) of a three-decimal constant:
 *   LMX_YUV_BT601  YB, YG, YR = 0.098, 0.504, 0.257 (102760, 528482, 269484);  UB, UG, UR = 0.439, -0.291, -0.148 (460325, -305136,
 *                  -155189);  VB, VG, VR = -0.071, -0.368, 0.439 (-74449, -385876, 460325)
 *   LMX_YUV_BT709  YB, YG, YR = 0.062, 0.614, 0.183 (65012, 643826, 191889);  UB, UG, UR = 0.439, -0.338, -0.101 (460325, -354419,
 *                  -105906);  VB, VG, VR = -0.040, -0.399, 0.439 (-41943, -418382, 460325)
 * Both chroma rows sum to 0 (a grey 2 x 2 gives U = V = 128), white gives Y = 235, the chroma extremes are 16 and 240, and no sum of
 * products leaves 32 bits.  The source is PITCHED: row r of frame i starts at bgr + i * stride_bgr + r * pitch_bgr, so a crop needs no
 * copy — point bgr at byte (y0 * W + x0) * 3 of a frame W pixels wide and pass pitch_bgr = 3 * W.  The output descriptor is
 * lmx_yuv_frames_t with writable planes: any pointer alignment and any pitch; where a 2-row x 16-column block's pieces are 16-byte
 * (I420 chroma: 8-byte) aligned they move as vector loads and stores (csrc/yuv.hip), the same bytes either way, and nothing outside
 * the rows' w (w / 2) bytes is written.  The descriptor is HOST memory, read during the call.  n = 0 launches nothing.  Refused with
 * LMX_EINVAL, never approximated: odd h or w or sizes below 2, pitch_bgr < 3 * w, an output pitch below its row, a layout or matrix
 * outside the enums, NV12 with v != NULL, I420 with v == NULL. */
typedef struct { uint8_t *y, *u, *v;            /* NV12: u = the interleaved plane, v = NULL */
                 int64_t pitch_y, pitch_c;      /* bytes per row; >= w, and >= w (NV12) or w/2 (I420) */
                 int64_t stride_y, stride_c;    /* bytes from frame i to frame i+1 in each allocation */
                 int32_t layout, matrix; } lmx_yuv_out_t;
int lmx_k_bgr_to_yuv420(const uint8_t* bgr, int64_t pitch_bgr /* bytes per row, >= 3 * w */, int64_t stride_bgr /* bytes per frame */,
                        int n, int h, int w, const lmx_yuv_out_t* out_host, lmx_stream_t stream);
int lmx_h_bgr_to_yuv420(const uint8_t* bgr_host, int64_t pitch_bgr, int64_t stride_bgr, int n, int h, int w, const lmx_yuv_out_t* out_host);

/* ---- the crop box of a clip: video-preprocessing main.py:86-110 on the host ---------------------------------------------------------
 * boxes_host: the k detections (x1, y1, x2, y2 as float32, frame pixels) that passed the caller's confidence rule (the reference: the
 * model's default 0.25 in the detector, then conf > 0.5) on the first 10 frames of an h x w clip, every class.  Kept: boxes whose
 * float32 area (x2 - x1) * (y2 - y1) is STRICTLY above w * h * 0.1 (a double).  box_host = (x1, y1, x2, y2): per column the median
 * of the kept boxes as np.median takes it on float32 (an even count averages the two middle values in float32), truncated towards
 * zero, x1 / y1 lowered by `pad` and clamped at 0, x2 / y2 raised by `pad` and clamped at w / h (the reference's pad: 50).  No box
 * kept: (0, 0, w, h), the full frame.  lmx.services.preprocessing.crop_box_of is the same arithmetic in Python.  Refused: k < 0,
 * h or w below 1, pad < 0, null pointers. */
int lmx_h_crop_box(const float* boxes_host /* [k][4] xyxy */, int k, int h, int w, int pad, int32_t* box_host /* [4] */);

/* ---- per-frame blur and brightness sums: BGR u8 [n][h][w][3] -> int64 [n][4] ------------------------------------------------------
 * Replaces what clip-curation's compute_blur_score and compute_brightness_score (main.py:276-289) compute per sampled frame —
 * cv2.cvtColor(BGR2GRAY), cv2.Laplacian(gray, CV_64F).var() and np.mean(gray) — by one pass over every frame at the memory rate; the
 * scores themselves are host arithmetic on the four sums (lmx.services.curation.visual_scores).  The arithmetic is defined HERE (cv2 is
 * not installed: PARITY UNPINNED against real OpenCV).  For pixel (x, y) of a frame with bytes B, G, R:
 *   g(x, y)   = (3735 * B + 19235 * G + 9798 * R + 16384) >> 15          OpenCV 4's 8-bit BGR2GRAY: round(2^15 * 0.114 / 0.587 / 0.299),
 *                                                                        rounded descale; 0 .. 255
 *   lap(x, y) = g(x-1, y) + g(x+1, y) + g(x, y-1) + g(x, y+1) - 4 * g(x, y)      cv2.Laplacian, ksize 1; |lap| <= 1020
 *   an index outside the frame is reflected without repeating the edge sample: -1 -> 1, w -> w - 2, -1 -> 1, h -> h - 2
 *   (BORDER_REFLECT_101, cv2's BORDER_DEFAULT)
 *   out[i] = { sum g, sum lap, sum lap^2, h * w } over frame i: exact 64-bit integer sums, so the result depends neither on the launch
 *   geometry nor on n nor on the order of any partial sum.
 * Frames are contiguous and may start at ANY byte address (h * w * 3 is odd for odd sizes); where a thread's run of 16 columns is
 * 16-byte aligned it moves as three 16-byte loads (csrc/quality.hip), the same values either way.  `out` is 8-byte aligned and needs no
 * clearing: the call zeroes it on `stream` and every one of its 4 n words is defined when the call completes there.  `workspace`:
 * lmx_frame_quality_workspace_bytes(n, h, w) bytes, which is 0 — the partial sums meet in `out` through 64-bit integer atomics — so it
 * may be NULL.  n = 0 launches nothing.  Refused with LMX_EINVAL before anything is read, written or launched: n < 0, h or w below 2
 * (the reflection needs two samples) or above 32768, a null bgr or out with n > 0.  lmx_h_frame_quality is the plain C++ restatement on
 * HOST memory (csrc/host_quality.cpp). */
int64_t lmx_frame_quality_workspace_bytes(int n, int h, int w);
int lmx_k_frame_quality(const uint8_t* bgr /* [n][h][w][3] */, int n, int h, int w, int64_t* out /* [n][4] */, void* workspace,
                        lmx_stream_t stream);
int lmx_h_frame_quality(const uint8_t* bgr_host /* [n][h][w][3] */, int n, int h, int w, int64_t* out_host /* [n][4] */);

/* tokens: out[b][0..n_prefix) = prefix[t][:] (+pos), out[b][n_prefix + p] = patch[b*np + p][:] + pos[n_prefix+p]
 * (f32 residual stream; pos may be NULL — DINOv3 has no learned position table). */
int lmx_k_assemble_tokens(const void* patch_f16, const float* prefix, const float* pos, float* out, int B, int np,
                          int n_prefix, int D, lmx_stream_t stream);

/* K22: mean over all T tokens of a f16/f32 [B][T][D] tensor -> f32 [B][D]  (dinov3 main.py:113) */
int lmx_k_token_mean(const void* x, int in_dtype, float* out, int B, int T, int D, lmx_stream_t stream);

/* ---- K8: NMS (ultralytics non_max_suppression as invoked at yolo main.py:76) ------------------------
 * pred f32 [n][A][4+nc] rows = (cx,cy,w,h, cls scores...) in letterboxed pixels.
 * Per image: keep candidates with max class score > conf; best class; sort by score descending (ties: lower
 * anchor index first); boxes offset by cls*max_wh; greedy IoU > iou suppression (torchvision.ops.nms
 * semantics, IoU computed exactly as torchvision's CPU kernel: f32, no FMA contraction, compared against the
 * DOUBLE threshold as `ovr > iou_threshold` does there); first max_det.  A <= 16384.
 * Outputs (row-major, caller allocated): boxes f32 [n][max_det][4] xyxy in letterboxed pixels (before
 * scale_boxes), scores f32 [n][max_det], cls int32 [n][max_det], src int32 [n][max_det] (anchor index),
 * counts int32 [n].  workspace: lmx_nms_workspace_bytes(n, A) bytes.
 */
int64_t lmx_nms_workspace_bytes(int n, int A);
int lmx_k_nms(const float* pred, int n, int A, int nc, float conf, double iou, int max_det, float max_wh,
              float* boxes, float* scores, int32_t* cls, int32_t* src, int32_t* counts, void* workspace,
              lmx_stream_t stream);

/* ---- YOLOv8 non-GEMM pieces (ultralytics predictor under yolo main.py:76) ---------- */
/* K1: LetterBox = cv2.resize(INTER_LINEAR, u8 fixed point) to rh x rw + constant-114 border to oh x ow at
 * (top,left) + BGR->RGB (swap_rb).  src u8 [n][sh][sw][3] -> dst u8 [n][oh][ow][3].  Tables from the host
 * (lmx/letterbox.py restates OpenCV's resizeGeneric_ table build): xofs i32 [rw], ialpha i16 [rw][2], yofs i32 [rh],
 * ibeta i16 [rh][2]; ignored (may be NULL) when rh==sh && rw==sw (LetterBox then skips the resize). */
int lmx_k_letterbox(const uint8_t* src, uint8_t* dst, int n, int sh, int sw, int rh, int rw, int top, int left,
                    int oh, int ow, const int32_t* xofs, const int16_t* ialpha, const int32_t* yofs,
                    const int16_t* ibeta, int swap_rb, lmx_stream_t stream);
/* stem Conv(3->Cout,k3,s2,p1)+bias+SiLU straight from the u8 letterboxed RGB frame (x = u8/255 in f32):
 * w f32 [3][3][3][Cout] (ky,kx,c,co), out f16 NHWC [n][H/2][W/2][Cout]; Cout%8==0. */
int lmx_k_stem_conv(const uint8_t* img, const float* w, const float* bias, void* out, int n, int H, int W, int Cout,
                    lmx_stream_t stream);
/* K5: max_pool2d(5, stride 1, pad 2) on an NHWC f16 channel slice (pixel strides lds/ldd in elements). */
int lmx_k_maxpool5(const void* src, int64_t lds, void* dst, int64_t ldd, int n, int H, int W, int C,
                   lmx_stream_t stream);
/* K6: nearest x2 upsample of an NHWC f16 slice [n][H][W][C] into a slice of a [n][2H][2W][*] buffer. */
int lmx_k_upsample2(const void* src, int64_t lds, void* dst, int64_t ldd, int n, int H, int W, int C,
                    lmx_stream_t stream);
/* K7: Detect decode of one level: head f32 [n][H][W][ldh >= 64+nc] (box logits side*16+bin, then class logits)
 * -> pred f32 [n][A][4+nc] rows a_off + y*W + x: DFL softmax expectation, dist2bbox(xywh), *stride, sigmoid. */
int lmx_k_detect_decode(const float* head, int64_t ldh, float* pred, int n, int H, int W, int nc, float stride,
                        int a_off, int A, lmx_stream_t stream);
/* ops.scale_boxes: boxes f32 [total][4] xyxy in place: (x - pad)/gain clipped to [0,w] x [0,h]. */
int lmx_k_scale_boxes(float* boxes, int total, float padx, float pady, float gain, float w, float h,
                      lmx_stream_t stream);

/* ---- EXACT-precision plan of the YOLO conv stack (lmx/yolo.py precision="exact"; csrc/exact.hip) -------------------------
 * north_star asks for NMS keep-sets bit-exact against the fp32 CPU path of yolo main.py:76; f16 activations deviate 3e-3 in
 * score.  The exact plan keeps lmx_k_gemm and feeds it operands with 22 mantissa bits: a value x travels as the f16 channel
 * triple [hi | lo | hi] per channel group of width g ("x3": hi = f16(x), lo = f16((x - hi) * 2048)), a weight row as
 * [whi | whi/2048 | wlo] over the same groups (rows pre-scaled by a power of two, undone by lmx_k_gemm's `scale`), so ONE
 * lmx_k_gemm launch over K' = 3K with f32 output yields x.w up to the dropped (x-hi)(w-whi) term (2^-22 relative).
 * lmx_k_split3: y = act(x) (+ the value of the x3 residual res3), written as x3 groups: f32 x [rows][ldx], N logical
 *   channels in groups of g (N % g == 0, g % 8 == 0): logical channel n = q*g + r sits at out3[m*ldo + q*3g + r] (hi),
 *   + g (lo), + 2g (hi again); res3 has the same grouping with pixel stride ldr.  act: NONE / SILU / GELU / RELU in torch's CPU forms: SiLU as
 *   x / (1 + exp(-x)) with a true division, GELU as 0.5 x (1 + erf(x / sqrt 2)).  Replaces the activation half of ultralytics' Conv and the
 *   shortcut add of Bottleneck under the exact plan.
 * lmx_k_maxpool5_x3: lmx_k_maxpool5 on an x3 slice of C logical channels (maximum by value; the pair travels with it).
 * lmx_k_stem_conv_x3: lmx_k_stem_conv writing x3: out3 f16 [n][H/2][W/2][3*Cout].
 * (nearest upsampling of an x3 slice is lmx_k_upsample2 over 3C channels.) */
int lmx_k_split3(const float* x, int64_t ldx, int act, const void* res3, int64_t ldr, void* out3, int64_t ldo, int64_t rows,
                 int N, int g, int nsum, int64_t sum_stride, lmx_stream_t stream);
/* (nsum > 1: x is the sum of nsum partial tensors x + s * sum_stride (elements), s = 0 .. nsum-1 added in that order — the
 * partial outputs of a split-K lmx_k_gemm launch) */
int lmx_k_maxpool5_x3(const void* src3, int64_t lds, void* dst3, int64_t ldd, int n, int H, int W, int C, lmx_stream_t stream);
int lmx_k_stem_conv_x3(const uint8_t* img, const float* w, const float* bias, void* out3, int n, int H, int W, int Cout,
                       lmx_stream_t stream);
/* The exact plan of the SAM mask decoder (lmx/sam_decoder.py precision="exact": f32 activations, x3 operands for every Linear):
 * lmx_k_attention_f32: SamAttention's softmax(q k^T * scale) v in plain f32 (TF:models/sam/modeling_sam.py:205-268) for the
 *   decoder's tiny problems — 7 tokens against 4096 image positions and back, head dim 16 or 32; q/k/v/o f32 token rows
 *   (row = b*T + t, head h at columns h*hd ..), flat geometry.  exp is expf, the division a true one.
 * lmx_k_hyper_mask_f32: lmx_k_hyper_mask on an f32 upscaled embedding `up` f32 [n][G*G][4][4][C], with the upscaler's last
 *   activation (act = LMX_ACT_GELU: exact erf form, or LMX_ACT_NONE) applied on load. */
int lmx_k_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* o,
                        int64_t ldo, int B, int H, int Tq, int Tk, int hd, float scale, lmx_stream_t stream);
int lmx_k_hyper_mask_f32(const float* up, const float* hyper, float* logits, int n, int G, int C, int act, lmx_stream_t stream);

/* Pose head post-processing for the detections lmx_k_nms kept (ultralytics Pose.kpts_decode + ops.scale_coords +
 * clip_coords; the YOLOv8-pose consumer is services/tleap-pipeline/app/main.py:142-163, `result.keypoints[j].data`).
 * raw0..2: the three levels' cv4 outputs, f32 [n][h_l][w_l][ldk] (ldk >= K*ndim); hw = {h0,w0,h1,w1,h2,w2} and strides[3]
 * are HOST arrays; src / counts are lmx_k_nms's device outputs (anchor index per kept detection, detections per image).
 * out f32 [n][max_det][K][ndim]: x, y in frame pixels ((v*2 + cell)*stride, minus the UNROUNDED letterbox padding,
 * / gain, clipped to [0,w] x [0,h]) and sigmoid(visibility) when ndim == 3; rows >= counts[b] are zero. */
int lmx_k_pose_gather(const float* raw0, const float* raw1, const float* raw2, int64_t ldk, const int32_t* hw,
                      const float* strides, const int32_t* src, const int32_t* counts, int n, int max_det, int K, int ndim,
                      float padx, float pady, float gain, float w, float h, float* out, lmx_stream_t stream);

/* ---- SAM / Hiera non-GEMM pieces ------------------------------------------------------------------------ */
/* K9+K10: im2col of the Hiera patch-embed conv (k7 s4 p3, TF sam2 :120-136) fused with SamPredictor's
 * normalisation and zero padding: img u8 [n][rh][rw][3] (the PIL-resized frame) sits at the top-left of an
 * IH x IW canvas of zeros (in NORMALISED space); out f16 [n*OH*OW][ldo], column (ky*KW + kx)*3 + c =
 * lut[c][u8] or 0 outside the image.  OH = (IH + 2*pad - KH)/stride + 1.  ldo%8==0, ldo >= KH*KW*3 (tail zeroed). */
int lmx_k_im2col_u8(const uint8_t* img, const float* lut, void* out, int n, int rh, int rw, int IH, int IW, int KH,
                    int KW, int stride, int pad, int64_t ldo, lmx_stream_t stream);
/* 2x2 / stride-2 max pool on an NHWC grid (Hiera do_pool, TF sam2 :291-300), dtype f16 or f32, channel slices
 * allowed on both sides (pixel strides lds/ldd in elements).  H, W even. */
int lmx_k_maxpool2(const void* src, int64_t lds, void* dst, int64_t ldd, int dtype, int n, int H, int W, int C,
                   lmx_stream_t stream);
/* f32 -> f16 row-wise convert (stage outputs of the f32 residual stream feeding the FPN 1x1 convs). */
int lmx_k_cast_f32_f16(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int cols,
                       lmx_stream_t stream);
/* The band of token rows of a Hiera trunk that depends on the frame.  A frame resized to nh x nw sits at the top-left of the zero
 * canvas (4 * grid pixels a side); until the first global-attention block, tokens mix only inside windows and 2 x 2 pools, so a
 * token whose windows never reach a real pixel has a value that the weights alone decide.  window[i] / q_stride[i], i < n_blocks: the
 * block plan (window 0 = global attention, q_stride 2 = the block pools its queries; a block's windows tile the grid it READS).
 * *band = the number of stage-1 token rows (of `grid`) that the blocks in front of the first global one must compute per frame:
 * the smallest count that covers every row whose 7 x 7 / stride 4 / pad 3 patch touches a pixel row < nh — (nh + 2) / 4 + 1 rows —
 * and is a whole number of windows (and of pooled pairs) of each of those blocks at that block's resolution; 56 * ceil(.. / 56) for
 * Hiera-B+.  *band = 0 (no band: compute the whole grid) when that count is the whole grid or more, when block 0 is global or no
 * block is, and when nw < 4 * grid (padding on the right: columns are not cut).  Pure host arithmetic: no HIP call. */
int lmx_h_hiera_band(const int* window, const int* q_stride, int n_blocks, int grid, int nh, int nw, int* band);
/* The same band sized per block, not once for the trunk (arguments as lmx_h_hiera_band).  rows[i], i < n_blocks: the token rows, of
 * the grid block i READS (`grid` halved behind every pooling block), that block i has to run on.  d = min((nh + 2) / 4 + 1, grid)
 * rows carry a pixel into block 0; a block in front of the first global one runs on d rounded up to whole windows of its own, and to
 * an even count where it pools — the whole grid of its resolution once that count reaches it — and hands those rows on, halved
 * behind a pooling block: a block never has fewer rows than the one before it left, and where it has more the constant rows
 * between the two are joined in front of it (lmx_k_band_join).  From the first global block on rows[i] is the whole grid; so is
 * every entry where lmx_h_hiera_band answers 0 for want of a place to end: nw < 4 * grid, block 0 global, no global block.
 * Hiera-B+, 576 x 1024: 152 (blocks 0 - 2) / 76 (3 - 5) / 42 (6 - 11) against lmx_h_hiera_band's 168 / 84 / 42.  Pure host
 * arithmetic: no HIP call. */
int lmx_h_hiera_bands(const int* window, const int* q_stride, int n_blocks, int grid, int nh, int nw, int* rows);
/* out [n][H][W][D] = rows < Hb of each image from band [n][Hb][W][D], rows >= Hb from table [(H - Hb) * W][D], the same for every
 * image: the frame-dependent band of a Hiera token grid (lmx_h_hiera_band) joined with its constant rows.  dtype f16 or f32, dense
 * operands; a row of D elements must be a multiple of 16 bytes and 1 <= Hb <= H - 1. */
int lmx_k_band_join(const void* band, const void* table, void* out, int dtype, int n, int H, int Hb, int W, int D,
                    lmx_stream_t stream);
/* The Hiera encoder's block plan on the host: WHICH kernels each block runs, on which rows, and what happens at a stage end — what
 * lmx/sam.py's hiera_plan() and HieraEncoder._settle() compute per call, for an encoder built the default way (fused MLP, ln_out
 * projections).  These functions read no environment variable: they are the Python plan with none of the LMX_* development
 * switches set.  Pure host arithmetic: no HIP call (csrc/host_hiera_plan.cpp; tests/test_hiera_plan_c_host.py holds every field to
 * Python's).
 * lmx_hiera_config_t: lmx.sam.HieraConfig — per stage s < n_stages: blocks[s], dims[s], heads[s], windows[s]; global_blocks[i],
 * i < n_global: block indices with global attention; the first q_pool_stages stages behind stage 0 open with a pooling block.
 * hidden, pos_bkg, fpn_dim, fpn_top_down (n_top_down entries) and eps do not enter the plan; they make the structure the whole
 * configuration.
 * lmx_hiera_block_t: lmx.sam.BlockPlan, field for field, the strings as the enums below (a field hiera_plan leaves None is
 * LMX_HIERA_SHORTCUT_NONE / LMX_HIERA_QUERY_NONE), the booleans as 0 / 1. */
enum { LMX_HIERA_MAX_STAGES = 8, LMX_HIERA_MAX_GLOBAL = 32, LMX_HIERA_MAX_BLOCKS = 256 };
typedef struct {
  int32_t hidden, n_stages, blocks[LMX_HIERA_MAX_STAGES], dims[LMX_HIERA_MAX_STAGES], heads[LMX_HIERA_MAX_STAGES],
      windows[LMX_HIERA_MAX_STAGES], n_global, global_blocks[LMX_HIERA_MAX_GLOBAL], pos_bkg[2], q_pool_stages, fpn_dim, n_top_down,
      fpn_top_down[LMX_HIERA_MAX_STAGES], image;
  double eps;
} lmx_hiera_config_t;
enum { LMX_HIERA_ATTN8_LN = 0, LMX_HIERA_ATTN8 = 1, LMX_HIERA_ATTN_POOL = 2, LMX_HIERA_ATTN4 = 3, LMX_HIERA_LAUNCHES = 4 }; /* attn */
enum { LMX_HIERA_LN1_KERNEL = 0, LMX_HIERA_LN1_PREV = 1, LMX_HIERA_LN1_LAUNCH = 2 };                                         /* ln1 */
enum { LMX_HIERA_SHORTCUT_NONE = 0, LMX_HIERA_SHORTCUT_GEMM = 1, LMX_HIERA_SHORTCUT_GEMM_MAXPOOL = 2, LMX_HIERA_SHORTCUT_POOLED_GEMM = 3 };
enum { LMX_HIERA_QUERY_NONE = 0, LMX_HIERA_QUERY_QKV = 1, LMX_HIERA_QUERY_QKV_MAXPOOL = 2, LMX_HIERA_QUERY_POOLED_Q_KV = 3 };
enum { LMX_HIERA_MLP_IMG = 0, LMX_HIERA_MLP_FUSED = 1, LMX_HIERA_MLP_LAUNCHES = 2 }; /* mlp (FUSED: never chosen without a switch) */
typedef struct {
  int32_t H, W, Hf, Ho, Wo, Hfo, join, attn, ln1, shortcut, query, window, ln_out, mlp, emit_ln1, stage_end, keep, x16, join_out, clone;
} lmx_hiera_block_t;
/* *n_blocks_host = the number of blocks of `config` (the sum of blocks[s]): the length of the arrays below.  LMX_EINVAL, with the
 * field named, for a configuration outside the limits above. */
int lmx_h_hiera_blocks(const lmx_hiera_config_t* config, int* n_blocks_host);
/* hiera_plan(config, n, rows, lowest): records_host[i] for n frames with block i on rows_in_host[i] token rows of the grid it reads
 * (lmx_h_hiera_bands, or the whole grid everywhere).  Where a block has more rows than the one before it left, a join sits in front
 * of it; fewer, or more than its grid has, is LMX_EINVAL.  lowest: stage outputs below this index are not kept. */
int lmx_h_hiera_plan_rows(const lmx_hiera_config_t* config, int n, const int* rows_in_host, int lowest, lmx_hiera_block_t* records_host);
/* HieraEncoder(band="blocks")._settle(nh, nw, n, lowest) for n frames resized to nh x nw: rows_host[i] = lmx_h_hiera_bands' rows,
 * settled — the rows below the band come from the whole-grid plan of one frame, so a block in the band must run the kernels that
 * plan chose, and one whose shape check fails on the rule's rows gets whole windows added until it passes — and records_host = the
 * plan on those rows; where there is no band, the whole grid and its plan.  Computed per chunk from that chunk's n (the pooled
 * GEMM's rule sees n * H * W). */
int lmx_h_hiera_plan(const lmx_hiera_config_t* config, int n, int nh, int nw, int lowest, lmx_hiera_block_t* records_host, int* rows_host);

/* ---- SAM mask decoder glue (TF:models/sam/modeling_sam.py:432-543; K18/K19) --------------------------------------- */
/* out[r][:] = a[r][:] + b[r % b_rows][:]  (a, b f32; out f32 or f16): queries + point embeddings, keys + image PE,
 * image embedding + no-mask dense embedding. */
int lmx_k_add_bcast(const void* a, int a_dtype, int64_t lda, const float* b, int64_t ldb, int b_rows, void* out,
                    int out_dtype, int64_t ldo, int64_t rows, int D, lmx_stream_t stream);
/* SamPromptEncoder._embed_boxes (TF sam :650-659) on device: boxes f32 [n][4] xyxy in FRAME pixels are scaled to the
 * resized image (ResizeLongestSide.apply_boxes: x*nw/w, y*nh/h in double), +0.5, /S, 2c-1, @gauss [2][F], *2pi,
 * [sin|cos] -> sparse f32 [n][2][2F], + corner[0|1] (the point_embed[2|3] rows, f32 [2][2F]). */
int lmx_k_prompt_box(const float* boxes, int64_t ldb, float* sparse, int n, double sx, double sy, float S,
                     const float* gauss, const float* corner, int F, lmx_stream_t stream);
/* masks[:,0] = hyper_in[:,0] @ upscaled: up f16 [n][G*G][4][4][C] (the two ConvTranspose2d(k2,s2) outputs kept in
 * nested quadrant order: pixel (y,x) of the GxG grid, then (dy1,dx1), then (dy2,dx2)), hyper f32 [n][C] ->
 * logits f32 [n][4G][4G] in spatial order (Y = 4y + 2dy1 + dy2, X = 4x + 2dx1 + dx2).  C%8==0, C<=64. */
int lmx_k_hyper_mask(const void* up, const float* hyper, float* logits, int n, int G, int C, lmx_stream_t stream);
/* Sam.postprocess_masks + threshold + mask statistics: logits f32 [n][L][L] -> bilinear (align_corners=False) to
 * TxT, crop [:nh,:nw], bilinear to h x w, > 0  => mask u8 [n][h][w] (0/1);  stats int64 [n][8] =
 * (area, sum_x, sum_y, min_x, min_y, max_x, max_y, 0) over mask pixels (min/max = +-big when empty).
 * workspace: n*nh*nw floats (the cropped TxT intermediate, so each output pixel costs 4 taps instead of 16). */
int lmx_k_mask_post(const float* logits, int n, int L, int T, int nh, int nw, int h, int w, uint8_t* mask,
                    int64_t* stats, float* workspace, lmx_stream_t stream);
/* ---- SAM prompt paths beyond the box (segment_anything SamPredictor.predict with point_coords / mask_input /
 * multimask_output / return_logits; TF:models/sam/modeling_sam.py:596-698, :432-543; csrc/prompt.hip) ------------------ */
/* SamPromptEncoder._embed_points + _embed_boxes: points f32 [n][Np][2] xy and labels int32 [n][Np] (1 foreground, 0 background,
 * -1 not a point), boxes f32 [n][>=4] xyxy or NULL, all in FRAME pixels -> sparse f32 [n][Ns][2F], Ns = Np + (boxes ? 2 : 1),
 * tokens [points..., box corners] or [points..., pad].  Coordinates as lmx_k_prompt_box (apply_coords in double, f32, +0.5,
 * /S, random-Fourier PE); label 0 / 1 adds point_embed f32 [2][2F] row 0 / 1; label -1 and the pad token (no box) are
 * not_a_point f32 [2F] alone; corner as lmx_k_prompt_box.  Np = 0 with a box gives lmx_k_prompt_box's bits.  A label outside
 * {-1, 0, 1} makes its token NaN (callers check labels on the host first). */
int lmx_k_prompt_points(const float* points, const int32_t* labels, int Np, const float* boxes, int64_t ldb, float* sparse, int n,
                        double sx, double sy, float S, const float* gauss, const float* point_embed, const float* not_a_point,
                        const float* corner, int F, lmx_stream_t stream);
/* SamMaskEmbedding + the dense add, replacing lmx_k_add_bcast(emb, no_mask) when a mask is given: mask_input f32 [n][4G][4G]
 * (the low-res logits of an earlier call) -> Conv2d(1,4,k2,s2) -> LayerNorm2d -> GELU -> Conv2d(4,16,k2,s2) -> LayerNorm2d ->
 * GELU -> Conv2d(16,256,k1) = dense [n][G][G][256]; keys f32 [n*G*G][ldk] = emb (f32 or f16 rows [n*G*G][lde]) + dense.
 * LayerNorm2d eps 1e-6, GELU the erf form, plain f32.  params f32 [LMX_MASK_EMBED_PARAMS], the torch tensors flattened in
 * this order: conv1.weight [4][1][2][2], conv1.bias [4], layer_norm1.weight [4], .bias [4], conv2.weight [16][4][2][2],
 * conv2.bias [16], layer_norm2.weight [16], .bias [16], conv3.weight [256][16][1][1], conv3.bias [256]. */
#define LMX_MASK_EMBED_PARAMS 4684
int lmx_k_mask_embed(const float* mask_input, const void* emb, int emb_dtype, int64_t lde, const float* params, float* keys,
                     int64_t ldk, int n, int G, lmx_stream_t stream);
/* masks[:, m] = hyper_in[:, m] @ upscaled for M = 1..4 masks in one pass over `up` (read once, not M times): hyper f32
 * [n][M][C] -> logits f32 [n][M][4G][4G].  Slice m equals lmx_k_hyper_mask / lmx_k_hyper_mask_f32 with hyper[:, m] bit for
 * bit.  _multi: up f16 as lmx_k_hyper_mask; _multi_f32: up f32 and act as lmx_k_hyper_mask_f32. */
int lmx_k_hyper_mask_multi(const void* up, const float* hyper, float* logits, int n, int M, int G, int C, lmx_stream_t stream);
int lmx_k_hyper_mask_multi_f32(const float* up, const float* hyper, float* logits, int n, int M, int G, int C, int act,
                               lmx_stream_t stream);
/* Sam.postprocess_masks without the threshold (predict(return_logits=True)): logits f32 [n][L][L] -> out f32 [n][h][w] with
 * lmx_k_mask_post's interpolation arithmetic, so (out > 0) is lmx_k_mask_post's mask bit for bit.  out 16-byte aligned. */
int lmx_k_mask_logits(const float* logits, int n, int L, int T, int nh, int nw, int h, int w, float* out, lmx_stream_t stream);

/* ---- SamAutomaticMaskGenerator (segment_anything automatic_mask_generator.py; lmx/amg.py) ----------------------------------
 * lmx_k_mask_score replaces calculate_stability_score + (masks > mask_threshold) + batched_mask_to_box applied to the
 * full-resolution output of Sam.postprocess_masks in _process_batch, without writing any output pixel (csrc/amg.hip).
 * logits f32 [.][L][L]; row i scores logits[idx ? idx[i] : i] (idx int32 [n] on the device, entries in range, or NULL).
 * v is lmx_k_mask_logits' value at each of the h x w output pixels, bit for bit.  out int64 [n][8] =
 *   { count(v > f32(thr + off)), count(v > f32(thr - off)), count(v > f32(thr)) (the area),
 *     min_x, min_y, max_x, max_y of v > f32(thr) (inclusive; [0,0,0,0] for an empty mask, as batched_mask_to_box), 0 }.
 * The thresholds are rounded as torch compares an f32 tensor with a Python float.  n <= 65535 per launch. */
int lmx_k_mask_score(const float* logits, int n, int L, int T, int nh, int nw, int h, int w, double thr, double off,
                     const int32_t* idx, int64_t* out, lmx_stream_t stream);
/* lmx_k_nms_boxes replaces torchvision.ops.batched_nms with one category in _process_crop (scores = iou_preds) and
 * _generate_masks (scores = 1 / crop box area) (csrc/nms.hip).  boxes f32 [n][ldb] xyxy (first 4 columns), scores f32 [n]
 * of any sign, valid u8 [n] (0 = not a candidate) or NULL; n <= 16384.  Greedy suppression of IoU > iou in the order
 * descending score, ties to the lower index (a stable argsort of -scores; -0 == +0); IoU in f32 as torchvision's CPU
 * kernel, compared in double.  keep_out int32 [n]: kept indices in that order, then -1; count_out int32 [1].
 * workspace: n * 20 bytes, 16-byte aligned. */
int lmx_k_nms_boxes(const float* boxes, int64_t ldb, const float* scores, const uint8_t* valid, int n, double iou, int32_t* keep_out,
                    int32_t* count_out, void* workspace, lmx_stream_t stream);
/* Bit-pack a 0/non-0 byte image: dst[r][c] holds pixels 8c..8c+7 of row r, first pixel in the most significant bit
 * (numpy.packbits order); rows are padded to ceil(w/8) bytes.  Used for the mask persisted / gathered per frame
 * (services/sam3-pipeline/app/main.py:83-89 returns a bool[H,W] mask; SURVEY.md §8b `mask_bits [n, h, ceil(w/8)]`):
 * 8x less D2H and xGMI traffic than the byte mask. */
int lmx_k_pack_bits(const uint8_t* src, int64_t rows, int w, uint8_t* dst, lmx_stream_t stream);
/* The per-frame record matrix in ONE launch (csrc/records.hip): what lmx.dist.pack_records builds with a torch.zeros and one strided
 * copy per field, and FusedExtractor.step's reference schedule with an index_copy_ per field on top (lmx/pipeline.py; SURVEY.md §8b
 * `lmx_allgather_results`, §8e: one fixed-stride byte row per frame is what the gather moves).  out u8 [n_rows][stride]:
 *   out[r][0:8]   int64 1 for r < n_valid, else 0 (the `valid` word; rows from n_valid on are padding: zeros throughout);
 *   field f of row r < n_valid = the row_bytes bytes of source row s of fields_host[f].src at out[r][offset ...], where s = r under
 *                 the identity map (map = -1) and s = row_maps_host[map][r] otherwise; zeros where s < 0 or s >= the field's n_src;
 *   every other byte of the row is zero, the padding behind each field up to the next 8-byte boundary included.
 * Every byte of out is stored exactly once, whatever it held: no memset in front, no atomics.
 * fields_host: HOST array of n_fields <= LMX_RECORD_MAX_FIELDS descriptors, read during the call (they travel as kernel arguments);
 * src is DEVICE memory [n_src][row_bytes], dense rows, any byte alignment; offset >= 8, a multiple of 8, the fields ascending and
 * disjoint with offset + row_bytes <= stride.  row_maps_host: HOST array of n_maps <= LMX_RECORD_MAX_MAPS DEVICE pointers, each int32
 * [n_valid]: no map is read for a padding row (NULL with n_maps = 0).  stride: a multiple of 8; out: 8-byte aligned.  n_rows = 0 is legal and launches nothing.
 * (n_src lives in the field, not in the call: a scheduled step gathers n_det rows of one network and n_emb of the other.) */
enum { LMX_RECORD_MAX_FIELDS = 16, LMX_RECORD_MAX_MAPS = 4 };
typedef struct { const void* src; int64_t row_bytes, offset; int32_t map, n_src; } lmx_record_field_t;
int lmx_k_pack_records(const lmx_record_field_t* fields_host, int n_fields, const int32_t* const* row_maps_host, int n_maps, int64_t n_valid,
                       int64_t n_rows, int64_t stride, uint8_t* out, lmx_stream_t stream);

/* ---- HOST functions: the fused record (csrc/host_records.cpp; all pointers are HOST memory) ----
 * lmx_h_record_layout: lmx.dist.record_layout of the dict FusedExtractor.step returns for h x w frames (lmx/pipeline.py; the record of
 *                   SURVEY.md §8b): the fields in sorted name order — boxes f32 [max_det][4], cls i32 [max_det], counts i32,
 *                   embedding f32 [hidden], mask_bits u8 [h][ceil(w/8)], mask_contour i64 [8], mask_iou f32, mask_stats i64 [8],
 *                   scores f32 [max_det], and with scheduled != 0 ran_det i32, ran_emb i32 between mask_stats and scores — each at
 *                   the next multiple of 8 bytes behind the 8-byte `valid` word; stride = the end of the last one.
 * lmx_h_stream_plan: lmx.pipeline.stream_plan(n_chunks, max_streams, layout): *pool_host = max(3, min(2 + n_chunks, max_streams))
 *                   streams, YOLO on *det_host = 0, DINO on *emb_host = 1, sam_host int32 [n_chunks] = the stream of each SAM pass
 *                   (LMX_STREAMS_LANES: dealt over streams 2 .. pool - 1; LMX_STREAMS_RR: round-robin over all of them, from 2).
 * lmx_h_row_map:    the row scatter of FusedExtractor.step's reference schedule (`out[k].index_copy_(0, idx, part[k])`,
 *                   `ran.index_fill_(0, idx, 1)`; yolo main.py:74, dinov3 main.py:127) as a gather: map_host int32 [n] = j where
 *                   idx_host[j] = r, else -1; ran_host int32 [n] (may be NULL) = 1 there, else 0.  idx_host int32 [n_idx] must
 *                   ascend strictly inside 0 .. n - 1: LMX_EINVAL names the first index that is out of range, repeated or out of
 *                   order (`what`: the list's name for the message). */
enum { LMX_REC_U8 = 0, LMX_REC_I32 = 1, LMX_REC_I64 = 2, LMX_REC_F32 = 3 }; /* lmx_record_field_layout_t.dtype */
enum { LMX_STREAMS_LANES = 0, LMX_STREAMS_RR = 1 };                          /* lmx_h_stream_plan's layout */
typedef struct { char name[16]; int32_t dtype, ndim; int64_t shape[2], offset, nbytes; } lmx_record_field_layout_t;
typedef struct { int32_t n_fields, reserved; int64_t stride; lmx_record_field_layout_t fields[LMX_RECORD_MAX_FIELDS]; } lmx_record_layout_t;
int lmx_h_record_layout(int h, int w, int hidden, int max_det, int scheduled, lmx_record_layout_t* out_host);
int lmx_h_stream_plan(int n_chunks, int max_streams, int layout, int* pool_host, int* det_host, int* emb_host, int32_t* sam_host);
int lmx_h_row_map(int n, const int32_t* idx_host, int n_idx, const char* what, int32_t* map_host, int32_t* ran_host);

/* ---- contour features ON THE DEVICE ---------------------------------------------------------
 * The cv2 part of extract_segmentation_features (sam3 main.py:118-135): findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE),
 * max(contours, key=contourArea), arcLength(closed), boundingRect — for n masks [n][h][w] (0 / non-0 bytes) in HBM.
 * out int64 [n][8] = { 2 * contourArea (exact), unit steps, diagonal steps of the border chain (arcLength = unit + diag * sqrt 2),
 * min x, min y, max x, max y of the largest external contour, number of external contours (0: all other fields 0) }.
 * Parallel restatement of host_mask.cpp's border following as sums over boundary cracks (csrc/contour.hip); equal to it bit
 * for bit (tests/test_gpu_contour.py).  workspace: lmx_contour_workspace_bytes(n, h, w) bytes, 16-byte aligned. */
int64_t lmx_contour_workspace_bytes(int n, int h, int w);
int lmx_k_contour_features(const uint8_t* mask, int n, int h, int w, int64_t* out, void* workspace, lmx_stream_t stream);

/* ---- HOST function (mask pointer is HOST memory) ----------------------------------------------------------------------
 * extract_segmentation_features (sam3 main.py:102-145) on a 0/1 byte mask [h][w]: out[7] = mask_area, area_ratio,
 * circularity, aspect_ratio, centroid_x, centroid_y, perimeter.  Restates cv2.findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_SIMPLE) + contourArea/arcLength/boundingRect of the largest contour + cv2.moments (cv2 absent: parity
 * unpinned).  Sequential border following on the host; lmx_k_contour_features is the device form (same numbers: the
 * perimeter is unit steps + diagonal steps * sqrt 2 in both). */
int lmx_h_mask_features(const uint8_t* mask_host, int h, int w, double* out_host);

/* ---- HOST functions of the tracking service (all pointers are HOST memory) -------------------
 * The association arithmetic of services/tracking-service/app/tracker/matching.py, the consumer of pipeline.yolo /
 * pipeline.dinov3: per frame a detections x tracks IoU matrix and one minimum-cost assignment on it (tens of boxes,
 * sequential per frame: host code in the reference, host code here; lmx/services/tracking.py is the caller).
 * lmx_h_iou_matrix: iou_batch (matching.py:12-44): a [n][4], b [m][4] xyxy boxes -> out [n][m] = inter / (union + 1e-6).
 * lmx_h_assign: linear_assignment (matching.py:69-101) = lap.lapjv(cost, extend_cost=True, cost_limit=100000) on a finite
 *   cost [n][m]: the minimum-cost assignment matching min(n, m) pairs; row_to_col [n] / col_to_row [m] hold the partner or -1.
 *   (lap is absent: parity unpinned; optimality is tested against scipy.optimize.linear_sum_assignment.) */
int lmx_h_iou_matrix(const double* a, int n, const double* b, int m, double* out);
int lmx_h_assign(const double* cost, int n, int m, int* row_to_col, int* col_to_row);

/* ---- HOST functions: the coefficient tables of the preprocessing kernels (csrc/host_resample.cpp; all pointers are HOST memory) ----
 * What a caller of lmx_k_pil_resize_h / _v and lmx_k_float_resize_patchify computes once per frame size and uploads; the C++ twins
 * of lmx/resample.py, equal to it bit for bit (tests/test_native_dino_host.py).  One axis per call, in_size -> out_size samples,
 * filt = LMX_FILT_BILINEAR | LMX_FILT_BICUBIC (Pillow's `resample` codes).  bounds_host int32 [out_size * 2] = (first source index,
 * taps) per output, kk_host [out_size * ksize] (taps beyond a row's count are 0), *ksize_host = the row length.  cap = the entries
 * kk_host holds; with bounds_host and kk_host both NULL the call only reports *ksize_host.
 * lmx_h_pil_tables: Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) in double, int32 fixed-point weights.
 * lmx_h_aa_tables:  ATen's antialias weights (UpSampleKernel.cpp _compute_indices_min_size_weights_aa) for a float32 tensor: every
 *                   step in float32 in ATen's order, the bicubic polynomials with the fused multiply-adds an FMA build of torch makes.
 * lmx_h_identity_table: the table of an axis that keeps its size n (bounds (i, 1), weight 2^22, ksize 1): lmx_k_pil_resize_h then
 *                   only swaps the channels.
 * lmx_h_segment_cols: lmx_k_float_resize_patchify's seg_cols for a horizontal table of n_out rows: the most source columns any
 *                   run of `tile` (256) consecutive outputs, starting at a multiple of `tile`, reads; < 0 on error. */
enum { LMX_FILT_BILINEAR = 2, LMX_FILT_BICUBIC = 3 };
int lmx_h_pil_tables(int in_size, int out_size, int filt, int32_t* bounds_host, int32_t* kk_host, int64_t cap, int* ksize_host);
int lmx_h_aa_tables(int in_size, int out_size, int filt, int32_t* bounds_host, float* kk_host, int64_t cap, int* ksize_host);
int lmx_h_identity_table(int n, int32_t* bounds_host, int32_t* kk_host);
int lmx_h_segment_cols(const int32_t* bounds_host, int n_out, int tile);

/* ==== MODEL level: DINO embeddings from raw frames (csrc/dino_model.hip, csrc/model_handle.h, csrc/host_dino_image.cpp) =============
 * The whole of services/dinov3-pipeline/app/main.py:98-113 — cvtColor, processor(images=...), model(**inputs), last_hidden_state
 * .mean(dim=1) — behind one call, for a consumer that is not a Python process: the launch sequence of lmx/dino.py's DinoEmbedder
 * (preprocess + hidden_states + token_mean) written in C++ over the lmx_k_* entry points above, with the descriptors lmx/kernels.py
 * fills.  Same launches, same bits as DinoEmbedder.embed_frames (tests/test_gpu_native_dino.py).
 * The model comes from a WEIGHT IMAGE: one little-endian file that lmx.native.write_dino_image(embedder, path) writes from a loaded
 * DinoEmbedder (header, config block, tensor directory, tensors in final device form; layout in csrc/image.h, the config block in csrc/dino_image.h).  Loading
 * safetensors / Hugging Face directories stays in Python: export once, then open the image from C.
 * Handle rules: a handle belongs to the device that was current at lmx_dino_open_host; every call with another device current is
 * LMX_EINVAL.  ONE host thread and ONE stream in flight per handle: all calls write the handle's workspace, so a call on another
 * stream (or lmx_dino_embed_host, which uses a stream of the handle's) needs the previous one finished first.  Several handles are
 * independent.  Errors: LMX_EINVAL / LMX_EHIP with lmx_last_error(), as everywhere. */
typedef struct lmx_dino lmx_dino;
enum { LMX_DINO_V2 = 0, LMX_DINO_V3 = 1 };       /* lmx_dino_info_t.arch */
enum { LMX_RECIPE_PIL = 0, LMX_RECIPE_FLOAT = 1 }; /* lmx_dino_info_t.recipe_kind: BitImageProcessor | DINOv3ViTImageProcessor */
typedef struct { int32_t arch, hidden, heads, layers, tokens, image, patch, gated, recipe_kind, max_batch; } lmx_dino_info_t;
/* HOST only, touches no GPU (the model of services/dinov3-pipeline/app/main.py:98-113; `from_pretrained` at :34-35, the checking half):
 * parse and validate an image — magic, version,
 * kind, sizes against the real file, every tensor the config block calls for with the shape it calls for, a head dim the attention
 * kernels serve.  LMX_EINVAL names the offending field.  info_host (may be NULL) receives the configuration, max_batch 0. */
int lmx_dino_image_check_host(const char* path_host, lmx_dino_info_t* info_host);
/* SYNCHRONOUS (the model of services/dinov3-pipeline/app/main.py:98-113; `from_pretrained(...).to(device)` at :34-36): validate the image as above, then allocate and upload the
 * weights and the workspace of max_batch frames on the CURRENT device.  *out_host is NULL after any failure, with nothing left allocated. */
int lmx_dino_open_host(const char* path_host, int max_batch, lmx_dino** out_host);
/* the end of the model of services/dinov3-pipeline/app/main.py:98-113: waits for the device, then frees everything the handle owns;
 * NULL is allowed */
void lmx_dino_close(lmx_dino* m);
/* the configuration of the model behind services/dinov3-pipeline/app/main.py:98-113 (hidden = `last_hidden_state.shape[-1]`, :77) and
 * the handle's max_batch */
int lmx_dino_info(const lmx_dino* m, lmx_dino_info_t* info_host);
/* SYNCHRONOUS (services/dinov3-pipeline/app/main.py:98-113, what `processor(images=...)` at :107 derives from the frame size): build the resize tables of an h x w
 * frame on the host, allocate the resized-frame workspace, upload.  A size already prepared is a lookup.  LMX_EINVAL for a frame that
 * resizes below the network's input, and beyond 16 sizes per handle. */
int lmx_dino_prepare(lmx_dino* m, int h, int w);
/* services/dinov3-pipeline/app/main.py:98-113 for n frames: frames u8 [n][h][w][3] (BGR as cv2 delivers them; rgb != 0: already RGB) -> emb f32 [n][hidden],
 * the mean over ALL tokens of the final LayerNorm.  For a frame size already prepared the call ONLY ENQUEUES on `stream`: no allocation,
 * no synchronisation; the first call for a new size runs lmx_dino_prepare itself, and THAT call synchronises.  n > max_batch runs in
 * chunks of max_batch (a frame's bits do not depend on the batch it rides in, so the result is the same). */
int lmx_dino_embed(lmx_dino* m, const uint8_t* frames, int n, int h, int w, int rgb, float* emb, lmx_stream_t stream);
/* services/dinov3-pipeline/app/main.py:98-113 for a caller with no HIP code of its own: frames_host and emb_host are HOST memory; uploads, embeds,
 * downloads and synchronises (examples/dino_embed.c). */
int lmx_dino_embed_host(lmx_dino* m, const uint8_t* frames_host, int n, int h, int w, int rgb, float* emb_host);

/* ---- HOST functions: the host arithmetic of the YOLO predictor (csrc/host_letterbox.cpp; all pointers are HOST memory) ----------
 * What a caller of lmx_k_letterbox / lmx_k_scale_boxes / lmx_k_gemm's split_k computes once per frame size; the C++ twins of
 * lmx/letterbox.py and lmx.kernels.split_k_for, equal to them bit for bit (tests/test_native_yolo_host.py).
 * lmx_h_letterbox_geometry: ultralytics LetterBox(new_shape=imgsz, auto, scaleup=True, center=True, stride) for an sh x sw frame and
 *                   the gain / padding ops.scale_boxes re-derives from the shapes (the predictor under yolo main.py:76): roundings are
 *                   Python's round (half to even on a double).
 * lmx_h_letterbox_tables: OpenCV's resizeGeneric_ table build for INTER_LINEAR on 8U, sh x sw -> rh x rw (cv2.resize inside LetterBox,
 *                   yolo main.py:76): xofs int32 [rw], ialpha int16 [rw][2], yofs int32 [rh], ibeta int16 [rh][2] — lmx_k_letterbox's tables.
 * lmx_h_conv_split_k: the split_k of an f32-output 3 x 3 convolution of the exact plan (yolo main.py:76 under precision "exact"): a
 *                   function of the LAYER — pixels of ONE frame, N, K, Cin — never of the batch; 1 = no split; < 0 on error. */
typedef struct { int32_t sh, sw, rh, rw, top, left, oh, ow; double gain, pad_x, pad_y; } lmx_letterbox_geo_t;
int lmx_h_letterbox_geometry(int sh, int sw, int imgsz, int stride, int auto_, lmx_letterbox_geo_t* out_host);
int lmx_h_letterbox_tables(int sh, int sw, int rh, int rw, int32_t* xofs_host, int16_t* ialpha_host, int32_t* yofs_host, int16_t* ibeta_host);
int lmx_h_conv_split_k(int64_t px_per_frame, int N, int K, int cin);

/* ==== MODEL level: YOLOv8 detections from raw frames (csrc/yolo_model.hip, csrc/model_handle.h, csrc/host_yolo_image.cpp) ===========
 * The whole of services/yolo-pipeline/app/main.py:76 — `self.yolo_model(frame, verbose=False, conf=...)`: LetterBox, the fused
 * Conv-BN-SiLU stack, Detect, non_max_suppression, scale_boxes — and, for pose models, of services/tleap-pipeline/app/main.py:150
 * (`result.keypoints`), behind one call: the launch sequence of lmx/yolo.py's YoloDetector written in C++ over the lmx_k_* entry
 * points above, with the descriptors lmx/kernels.py fills.  Same launches, same bits as YoloDetector.detect / detect_pose on both
 * precision plans (tests/test_gpu_native_yolo.py).
 * The model comes from a weight image of kind YOLO that lmx.native.write_yolo_image(detector, path, plans) writes (layout in
 * csrc/image.h and csrc/yolo_image.h): the stem, and per convolution the packed tensors of the f16 plan and / or the x3 tensors of the exact plan.
 * Handle, image and error conventions as for lmx_dino: the handle belongs to the device current at open; ONE host thread and ONE
 * stream in flight per handle; several handles are independent; LMX_EINVAL / LMX_EHIP with lmx_last_error(). */
typedef struct lmx_yolo lmx_yolo;
enum { LMX_YOLO_F16 = 0, LMX_YOLO_EXACT = 1 }; /* `precision`; lmx_yolo_info_t.plans has bit (1 << precision) for each plan the image holds */
typedef struct { int32_t scale /* 'n' 's' 'm' 'l' 'x' */, nc, imgsz, kpt_k, kpt_ndim /* 0: no Pose head */, plans, max_batch; } lmx_yolo_info_t;
/* HOST only, touches no GPU (`YOLO(path)` of yolo main.py:76, the checking half): parse and validate an image — magic, version, kind,
 * sizes against the real file, the config block with its class names, and every tensor the configuration calls for (the layer table is
 * derived from scale, nc and the keypoint shape) with its dtype and shape.  LMX_EINVAL names the offending field or tensor.
 * info_host (may be NULL) receives the configuration, max_batch 0. */
int lmx_yolo_image_check_host(const char* path_host, lmx_yolo_info_t* info_host);
/* SYNCHRONOUS (`YOLO(path).to(device)` of yolo main.py:76): validate as above, then upload the weights to the CURRENT device.
 * Workspaces come with lmx_yolo_prepare.  *out_host is NULL after any failure, with nothing left allocated. */
int lmx_yolo_open_host(const char* path_host, int max_batch, lmx_yolo** out_host);
/* the end of the model of yolo main.py:76: waits for the device, then frees everything the handle owns; NULL is allowed */
void lmx_yolo_close(lmx_yolo* m);
/* the configuration of the model behind yolo main.py:76 and the handle's max_batch */
int lmx_yolo_info(const lmx_yolo* m, lmx_yolo_info_t* info_host);
/* `result.names[cls]` of yolo main.py:76: the class name (UTF-8, owned by the handle), NULL out of range */
const char* lmx_yolo_class_name(const lmx_yolo* m, int cls);
/* SYNCHRONOUS (what the predictor of yolo main.py:76 derives from the frame size): the letterbox geometry and tables of an h x w frame
 * and the whole workspace of max_batch frames under `precision` — letterboxed frames, every activation buffer of the plan, the f32
 * convolution outputs and split-K partials of the exact plan, heads, pred, the NMS workspace.  A pair already prepared is a lookup.
 * LMX_EINVAL for a plan the image does not hold, for a buffer of 2 GB or more (named: the GEMM kernels walk an operand with 32-bit byte
 * offsets, and for these launches only this call checks it), and beyond 16 (size, plan) pairs per handle. */
int lmx_yolo_prepare(lmx_yolo* m, int h, int w, int precision);
/* host arithmetic of yolo main.py:76's LetterBox: the network input oh x ow of an h x w frame and its A = anchors over strides 8, 16, 32 */
int lmx_yolo_anchors(const lmx_yolo* m, int h, int w, int* oh_host, int* ow_host, int* A_host);
/* the network of yolo main.py:76 without NMS: frames u8 [n][h][w][3] BGR -> pred f32 [n][A][4+nc] (xywh in letterboxed pixels, class
 * scores) = YoloDetector.forward_letterboxed(preprocess(frames)).  Enqueue-only after lmx_yolo_prepare, as lmx_yolo_detect. */
int lmx_yolo_predict(lmx_yolo* m, const uint8_t* frames, int n, int h, int w, int precision, float* pred, lmx_stream_t stream);
/* yolo main.py:76 for n frames (tleap main.py:150 with kpts): frames u8 [n][h][w][3] BGR -> boxes f32 [n][max_det][4] xyxy in FRAME
 * pixels, scores f32 [n][max_det], cls int32 [n][max_det], src int32 [n][max_det] (anchor index, -1 past counts), counts int32 [n];
 * rows past counts[b] are zero.  kpts f32 [n][max_det][K][ndim] (frame pixels, sigmoid visibility) for an image with a Pose head and
 * NULL otherwise; anything else is LMX_EINVAL.  For a (size, precision) already prepared the call ONLY ENQUEUES on `stream`: no
 * allocation, no synchronisation; the first call for a new pair runs lmx_yolo_prepare itself, and THAT call synchronises.
 * n > max_batch runs in chunks of max_batch, each writing its slice of the outputs. */
int lmx_yolo_detect(lmx_yolo* m, const uint8_t* frames, int n, int h, int w, int precision, float conf, double iou, int max_det,
                    float* boxes, float* scores, int32_t* cls, int32_t* src, int32_t* counts, float* kpts, lmx_stream_t stream);
/* yolo main.py:76 / tleap main.py:150 for a caller with no HIP code of its own: every pointer is HOST memory; uploads, detects,
 * downloads and synchronises (examples/yolo_detect.c). */
int lmx_yolo_detect_host(lmx_yolo* m, const uint8_t* frames_host, int n, int h, int w, int precision, float conf, double iou, int max_det,
                         float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* src_host, int32_t* counts_host,
                         float* kpts_host);

/* ==== MODEL level: SAM masks from raw frames and boxes (csrc/sam_model.hip, csrc/model_handle.h, csrc/host_sam_image.cpp) ===========
 * The whole of services/sam3-pipeline/app/main.py:74-92 — `predictor.set_image(frame)`, `predictor.predict(box=..., multimask_output=
 * False)` — behind one call: ResizeLongestSide, the SAM v1 ViT image encoder, the prompt encoder for one box per frame, the mask
 * decoder, Sam.postprocess_masks and the threshold, and what the service then takes from the mask (packed bits, statistics, contour
 * features).  It is the launch sequence of lmx/sam.py's SamVitEncoder.encode and lmx/sam_decoder.py's MaskDecoder.predict written in
 * C++ over the lmx_k_* entry points above, with the descriptors lmx/kernels.py fills.  Same launches, same bits as the Python classes
 * on both precision plans (tests/test_gpu_native_sam.py).
 * The model comes from a weight image of kind SAM that lmx.native.write_sam_image(encoder, decoder, path, plans) writes (layout in
 * csrc/image.h and csrc/sam_image.h): every tensor in final device form, per plan the image holds.
 * A weight image whose encoder is Hiera (write_sam_image on a lmx.sam.HieraEncoder; Hiera-B+ is BASELINE's headline configuration) is
 * served by the same calls (csrc/sam_hiera_model.h): lmx_sam_encode is then the launch sequence of HieraEncoder(band="blocks").encode(
 * frames, outputs="embedding")["fpn"][2] over the block plan lmx_h_hiera_plan computes per chunk, the embedding is f16 under BOTH
 * precisions (the trunk has one plan; `precision` selects the decoder plan and is checked against the image's plans mask), and
 * lmx_sam_prepare also builds, once per resized geometry and shared by both plans, the table of the token rows below the band that
 * depends on the frame (tests/test_gpu_native_sam_hiera.py).  lmx_sam_info_t of a Hiera image: encoder LMX_SAM_ENC_HIERA, hidden =
 * dims[0], heads = heads[0], layers = the number of blocks, mlp = 0, window = windows[0], patch = 16 (so that G = image / patch), image,
 * plans, max_batch.
 * OUT OF SCOPE, each refused or absent rather than approximated: point prompts, mask-input prompts and multimask output
 * (lmx/sam_decoder.py MaskDecoder.decode serves them from Python), SamAutomaticMaskGenerator (lmx/amg.py), outputs="all" of the Hiera
 * encoder (the high-resolution FPN levels and the stage outputs), and HIP graph capture of these calls.
 * Handle, image and error conventions as for lmx_yolo: the handle belongs to the device current at open; ONE host thread and ONE
 * stream in flight per handle; several handles are independent; LMX_EINVAL / LMX_EHIP with lmx_last_error(). */
typedef struct lmx_sam lmx_sam;
enum { LMX_SAM_F16 = 0, LMX_SAM_EXACT = 1 }; /* `precision`; lmx_sam_info_t.plans has bit (1 << precision) for each plan the image holds */
enum { LMX_SAM_ENC_VIT = 0, LMX_SAM_ENC_HIERA = 2 }; /* lmx_sam_info_t.encoder (1 is no encoder's and is refused) */
typedef struct { int32_t encoder, hidden, heads, layers, mlp, window, patch, image, plans, max_batch; } lmx_sam_info_t;
/* HOST only, touches no GPU (`sam_model_registry[...](checkpoint=...)` behind services/sam3-pipeline/app/main.py:74-92, the checking
 * half): parse and validate an image — magic, version, kind, sizes against the real file, the config block, every tensor the
 * configuration and the plan mask call for with its dtype and shape, a head dim the attention kernels serve, and for an image that
 * holds the exact plan the shapes at which every encoder Linear is ONE launch (hidden, mlp and 3 * patch^2 multiples of 64, every N at
 * least 96).  LMX_EINVAL names the offending field or tensor.  info_host (may be NULL) receives the configuration, max_batch 0. */
int lmx_sam_image_check_host(const char* path_host, lmx_sam_info_t* info_host);
/* SYNCHRONOUS (`SamPredictor(sam.to(device))` behind services/sam3-pipeline/app/main.py:74-92): validate as above, then upload the
 * weights to the CURRENT device.  Workspaces come with lmx_sam_prepare.  *out_host is NULL after any failure, with nothing left
 * allocated. */
int lmx_sam_open_host(const char* path_host, int max_batch, lmx_sam** out_host);
/* the end of the model of services/sam3-pipeline/app/main.py:74-92: waits for the device, then frees everything the handle owns; NULL
 * is allowed */
void lmx_sam_close(lmx_sam* m);
/* the configuration of the model behind services/sam3-pipeline/app/main.py:74-92 and the handle's max_batch */
int lmx_sam_info(const lmx_sam* m, lmx_sam_info_t* info_host);
/* host arithmetic of `set_image` (services/sam3-pipeline/app/main.py:74-92): ResizeLongestSide.get_preprocess_shape of an h x w frame,
 * int(x * image / max(h, w) + 0.5) per side */
int lmx_sam_resized(const lmx_sam* m, int h, int w, int* nh_host, int* nw_host);
/* SYNCHRONOUS (what `set_image` and `predict` of services/sam3-pipeline/app/main.py:74-92 derive from the frame size): the resize
 * tables of an h x w frame and ONE workspace of max_batch frames under `precision` — the resized frame, the patch matrix, every
 * activation of the encoder and of the decoder, the relative-position tables, the token buffer with its constant output-token rows,
 * lmx_k_mask_post's intermediate, the outputs a caller may leave NULL and the contour workspace.  A pair already prepared is a lookup.
 * LMX_EINVAL for a plan the image does not hold, for a buffer of 2 GB or more (named), and beyond 16 (size, plan) pairs per handle. */
int lmx_sam_prepare(lmx_sam* m, int h, int w, int precision);
/* `predictor.set_image(frame)` of services/sam3-pipeline/app/main.py:74-92 for n frames: frames u8 [n][h][w][3], consumed in the
 * channel order given (the service hands over its BGR frame; no swap) -> emb [n][G][G][out_ch], G = image / patch: f16 under
 * LMX_SAM_F16, f32 under LMX_SAM_EXACT = SamVitEncoder.encode(frames, precision)["fpn"][2]; f16 under both for a Hiera image.  Enqueue-only after lmx_sam_prepare, as
 * lmx_sam_segment. */
int lmx_sam_encode(lmx_sam* m, const uint8_t* frames, int n, int h, int w, int precision, void* emb, lmx_stream_t stream);
/* `predictor.predict(box=..., multimask_output=False)` of services/sam3-pipeline/app/main.py:74-92 on n embeddings of lmx_sam_encode
 * under the same precision: boxes f32 [n][4] xyxy in FRAME pixels (one per frame; an all-zero box stands for "no detection") ->
 * mask u8 [n][h][w] (0 / 1), stats int64 [n][8] (lmx_k_mask_post's), iou f32 [n], lowres f32 [n][4G][4G] =
 * MaskDecoder.predict(emb, boxes, (h, w), resized, precision); and, where asked for, mask_bits u8 [n][h][ceil(w/8)]
 * (lmx_k_pack_bits) and contour int64 [n][8] (lmx_k_contour_features: frames of 2 x 2 up to 2^21 - 1 pixels).  mask, mask_bits,
 * contour and lowres may each be NULL (what the decoder needs of them lives in the workspace); stats and iou may not. */
int lmx_sam_decode(lmx_sam* m, const void* emb, int n, int h, int w, const float* boxes, int precision, uint8_t* mask, uint8_t* mask_bits,
                   int64_t* stats, int64_t* contour, float* iou, float* lowres, lmx_stream_t stream);
/* services/sam3-pipeline/app/main.py:74-92 for n frames: lmx_sam_encode into the handle's workspace, then lmx_sam_decode.  For a
 * (size, precision) already prepared the call ONLY ENQUEUES on `stream`: no allocation, no synchronisation; the first call for a new
 * pair runs lmx_sam_prepare itself, and THAT call synchronises.  n > max_batch runs in chunks of max_batch, each writing its slice of
 * the outputs. */
int lmx_sam_segment(lmx_sam* m, const uint8_t* frames, int n, int h, int w, const float* boxes, int precision, uint8_t* mask,
                    uint8_t* mask_bits, int64_t* stats, int64_t* contour, float* iou, float* lowres, lmx_stream_t stream);
/* services/sam3-pipeline/app/main.py:74-92 for a caller with no HIP code of its own: every pointer is HOST memory; uploads, segments,
 * downloads and synchronises (examples/sam_segment.c). */
int lmx_sam_segment_host(lmx_sam* m, const uint8_t* frames_host, int n, int h, int w, const float* boxes_host, int precision,
                         uint8_t* mask_host, uint8_t* mask_bits_host, int64_t* stats_host, int64_t* contour_host, float* iou_host,
                         float* lowres_host);

/* ==== MODEL level: the fused per-frame path, frames to records (csrc/fused_model.hip, csrc/sam_lanes.h, csrc/records.hip) ===========
 * What a consumer of all three services does per frame — yolo main.py:74-76 (detect), sam3 main.py:199-206 (the first, highest-
 * confidence detection is SAM's box prompt) and :74-92 (mask), :118-135 (its statistics and contour features), dinov3 main.py:98-113
 * (embedding) — behind ONE handle and one call: the launch sequence of lmx/pipeline.py's FusedExtractor.step (BASELINE cfg#5) written in
 * C++ over the three model handles above, ending in the fixed-stride record of lmx.dist.pack_records (SURVEY.md §8b `lmx_init ..
 * lmx_allgather_results`: one context, frames in, per-frame results out).  Same launches on the same kind of streams, same bytes as
 * dist.pack_records(FusedExtractor.step(...)) without the byte masks, on both precision plans (tests/test_gpu_native_fused.py).
 * Streams: lmx_fused_step enqueues on internal streams of the handle, laid out as lmx_h_stream_plan(passes, min(max_streams,
 * 2 + sam_lanes), LMX_STREAMS_LANES): YOLO on one, DINO on one, the SAM passes of sam_chunk frames dealt over the rest.  Every internal
 * stream first waits for an event recorded on the caller's `stream`; a SAM pass runs its encoder at once and waits for YOLO's event in
 * front of its decoder, which reads each frame's top box straight from YOLO's boxes; `stream` then waits for every internal stream and
 * runs lmx_k_pack_records into `records`.  Each stream of SAM passes has a workspace lane of its own over ONE weight upload, so sam_lanes
 * passes are in flight together.  Streams and events are created at open (events without timing); a step creates nothing.
 * The record: lmx_fused_layout — the int64 `valid` word, then boxes f32 [300][4], cls i32 [300], counts i32, embedding f32 [hidden],
 * mask_bits u8 [h][ceil(w/8)], mask_contour i64 [8], mask_iou f32, mask_stats i64 [8], (scheduled: ran_det i32, ran_emb i32,) scores
 * f32 [300], each at the next multiple of 8 bytes.  max_det = 300 and the NMS IoU 0.7 are YoloDetector.detect's defaults.
 * Handle rules as for the model handles: the handle belongs to the device current at lmx_fused_open_host; ONE host thread and ONE STEP
 * in flight per handle — the previous lmx_fused_step must have FINISHED on the device (not merely been enqueued) before the next call,
 * lmx_fused_schedule or lmx_fused_prepare: all steps write the handle's workspaces.  Errors: LMX_EINVAL / LMX_EHIP with lmx_last_error().
 * OUT OF SCOPE: the byte masks, pose keypoints in the record (a Pose image is refused at open), point or mask prompts, RCCL inside the
 * library (the records are what a caller's gather moves), HIP graph capture of a step. */
typedef struct lmx_fused lmx_fused;
typedef struct { lmx_yolo_info_t yolo; lmx_sam_info_t sam; lmx_dino_info_t dino; int32_t hidden, max_det, max_frames, sam_chunk, sam_lanes, max_streams; } lmx_fused_info_t;
/* SYNCHRONOUS (the three `from_pretrained` / `YOLO(path)` / `sam_model_registry` loads behind yolo main.py:76, sam3 main.py:74-92 and
 * dinov3 main.py:34-36): validate and upload the three weight images on the CURRENT device (YOLO and DINO for max_frames frames a call,
 * SAM for passes of sam_chunk frames), create 2 + sam_lanes streams and their events.  sam_lanes 1 .. 16; max_streams 1 .. 64 bounds
 * the streams a step uses (FusedExtractor's LMX_MAX_STREAMS; at least 3 are used).  *out_host is NULL after any failure, with nothing
 * left allocated. */
int lmx_fused_open_host(const char* yolo_image, const char* sam_image, const char* dino_image, int max_frames, int sam_chunk, int sam_lanes,
                        int max_streams, lmx_fused** out_host);
/* the end of the models behind yolo main.py:76, sam3 main.py:74-92 and dinov3 main.py:98-113: waits for the device, then frees
 * everything the handle owns, the three model handles included; NULL is allowed */
void lmx_fused_close(lmx_fused* m);
/* the configurations of the three models (yolo main.py:76, sam3 main.py:74-92, dinov3 main.py:77 for hidden), max_det = 300 and the
 * handle's max_frames, sam_chunk, sam_lanes, max_streams */
int lmx_fused_info(const lmx_fused* m, lmx_fused_info_t* info_host);
/* host arithmetic only (the result rows the services return per frame: yolo main.py:74-76, sam3 main.py:83-89 and :118-135, dinov3
 * main.py:113): lmx_h_record_layout for this handle's hidden and max_det */
int lmx_fused_layout(const lmx_fused* m, int h, int w, int scheduled, lmx_record_layout_t* out_host);
/* SYNCHRONOUS (what yolo main.py:76, sam3 main.py:74-92 and dinov3 main.py:107 derive from the frame size): lmx_yolo_prepare,
 * lmx_dino_prepare, lmx_sam_prepare for EVERY lane, and the step's output buffers of max_frames rows.  LMX_EINVAL for a plan either
 * image does not hold (checked before anything is allocated), for frames outside 2 x 2 .. 2^21 - 1 pixels (the contour features' range),
 * and for what the three prepares refuse. */
int lmx_fused_prepare(lmx_fused* m, int h, int w, int precision);
/* SYNCHRONOUS (the reference schedule: yolo main.py:74 runs YOLO + SAM, dinov3 main.py:127 runs DINO, each on a subset of the sampled
 * frames): later steps of n frames gather the frames det_idx_host int32 [n_det] / emb_idx_host [n_emb] name, run the dense sequence on
 * them and scatter the rows back through row maps (lmx_h_row_map builds them here, this call uploads them); the record gains ran_det /
 * ran_emb, and a frame in neither list is a zero row with valid = 1, as in FusedExtractor.step.  A count of -1 leaves that list out
 * (every frame, read in place); n_det = n_emb = -1 clears the schedule: dense steps again.  LMX_EINVAL names an index that is out of
 * range, repeated or out of order. */
int lmx_fused_schedule(lmx_fused* m, int n, const int32_t* det_idx_host, int n_det, const int32_t* emb_idx_host, int n_emb);
/* yolo main.py:74-76, sam3 main.py:199-206, :74-92 and :118-135, dinov3 main.py:98-113 for n <= max_frames frames: frames u8
 * [n][h][w][3] BGR on the device -> records u8 [n_rows][stride] on the device, row r = frame r; n_rows >= n, the rows from n on are
 * padding (valid = 0, zeros: what a shard of a multi-GPU gather pads with); n = 0 writes padding only.  conf: YOLO's confidence
 * threshold; a frame without a detection is decoded against an all-zero box and has counts = 0.  For a (size, precision) already
 * prepared the call ONLY ENQUEUES (on `stream` and the internal streams): no allocation, no synchronisation; the first call for a new
 * pair runs lmx_fused_prepare itself, and THAT call synchronises.  `records` needs no clearing.  ONE step in flight per handle (above). */
int lmx_fused_step(lmx_fused* m, const uint8_t* frames, int n, int h, int w, int precision, float conf, uint8_t* records, int64_t n_rows,
                   lmx_stream_t stream);
/* the same (yolo main.py:74-76, sam3 main.py:74-92, dinov3 main.py:98-113) for a caller with no HIP code of its own: frames_host and
 * records_host are HOST memory; uploads, steps, downloads the records in ONE copy and synchronises (examples/fused_extract.c). */
int lmx_fused_step_host(lmx_fused* m, const uint8_t* frames_host, int n, int h, int w, int precision, float conf, uint8_t* records_host,
                        int64_t n_rows);
/* the same step (yolo main.py:74-76, sam3 main.py:74-92, dinov3 main.py:98-113) on frames as a decoder leaves them: frames_host
 * describes n NV12 / I420 frames on the device (lmx_k_yuv420_to_bgr's descriptor and checks).  The call converts them on `stream` into
 * a BGR buffer the handle owns — max_frames frames of this size — and then does exactly what lmx_fused_step does on that buffer, the
 * schedule of lmx_fused_schedule included: the records are those of lmx_k_yuv420_to_bgr followed by lmx_fused_step, byte for byte, on
 * both precision plans.  The buffer is allocated by the first _yuv call for a frame size (THAT call synchronises, as the first call
 * for a new size does anyway), freed at close and when a _yuv call brings another size; lmx_fused_prepare, lmx_fused_step and lmx_fused_step_host never allocate it.  The
 * three single-model handles have no _yuv twin: run lmx_k_yuv420_to_bgr in front of them. */
int lmx_fused_step_yuv(lmx_fused* m, const lmx_yuv_frames_t* frames_host, int n, int h, int w, int precision, float conf,
                       uint8_t* records, int64_t n_rows, lmx_stream_t stream);
/* the same (yolo main.py:74-76, sam3 main.py:74-92, dinov3 main.py:98-113) for a caller with no HIP code of its own: yuv_host is n
 * frames of tightly packed rawvideo in HOST memory, u8 [n][h * 3 / 2][w] — `nv12` (h luma rows, then h / 2 rows of interleaved U V) or
 * `yuv420p` (h luma rows, the U plane, the V plane; LMX_YUV_I420).  Uploads the blob in ONE copy (1.5 bytes per pixel against
 * lmx_fused_step_host's 3), converts, steps, downloads the records in ONE copy and synchronises (examples/fused_extract_nv12.c). */
int lmx_fused_step_yuv_host(lmx_fused* m, const uint8_t* yuv_host /* [n][h*3/2][w], rawvideo nv12 / yuv420p */, int layout, int matrix,
                            int n, int h, int w, int precision, float conf, uint8_t* records_host, int64_t n_rows);
/* the three pipelines on a crop window of the ORIGINAL decode (video-preprocessing main.py:112-127 cuts the window out and re-encodes;
 * its consumers then decode that file): frames_host describes n NV12 / I420 frames of h x w on the device, roi_host a window inside them
 * (lmx_k_yuv420_to_bgr_roi's descriptor, window and checks).  The call converts the window on `stream` into the BGR buffer the handle
 * owns for _yuv calls, sized max_frames x roi.h x roi.w x 3, and then does exactly what lmx_fused_step does on it at roi.h x roi.w: the
 * records are those of lmx_k_yuv420_to_bgr_roi followed by lmx_fused_step, byte for byte, on both precision plans; the window that
 * covers the frame gives lmx_fused_step_yuv's.  The buffer follows lmx_fused_step_yuv's rules with the WINDOW's size as its size: the
 * first call for a size allocates and synchronises, another size replaces it, lmx_fused_prepare(m, roi.h, roi.w, ...) prepares the
 * rest and never allocates it. */
int lmx_fused_step_yuv_roi(lmx_fused* m, const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host,
                           int precision, float conf, uint8_t* records, int64_t n_rows, lmx_stream_t stream);

/* ==== The TCN gait model: a lameness severity score with an MC-dropout spread from a pose series (csrc/tcn.hip, csrc/host_tcn.cpp) ====
 * Replaces services/tcn-pipeline/app/main.py:22-195, the temporal convolutional network over the pose series and its
 * predict_with_uncertainty (ten train-mode forwards at batch 1, about 45 launches each), by ONE launch for n clips and S samples: one
 * workgroup per (clip, sample), the activations resident in LDS from the input series to the sigmoid.
 * The network (batch-free, x [T][F]): block i = 0 .. n_blocks - 1 has dilation d = 2^i and channels[i] outputs;
 *   h   = drop_{2i}  ( relu( conv1(x) ) )          conv(x)[t][o] = b[o] + sum_{j < k, c} W[o][c][j] * x[t - (k - 1 - j) * d][c], x[t < 0] = 0
 *   y   = drop_{2i+1}( relu( conv2(h) ) )
 *   x'  = relu( y + res(x) )                       res = a 1 x 1 convolution where the channel count changes, the identity otherwise
 * then pooled[c] = mean over the T steps, hid = drop_{2 n_blocks}( relu( fc1 pooled + b ) ), pred = 1 / (1 + expf(-(fc2 hid + b))).
 * All arithmetic is f32 with f32 accumulation (the exact f32-input MFMA on the device), so the device, lmx_h_tcn_forward and torch in
 * float32 differ by summation order only.  The weights are the FOLDED weight-norm weights g * v / ||v|| (lmx.checkpoints.tcn_from_state_dict).
 *
 * MC dropout.  Torch's generator cannot be reproduced, so the keep decision is pinned HERE as integer arithmetic; each clip carries
 * its own 64-bit seed.
 *   Dropout sites are numbered 0 .. 2 * n_blocks (n_sites = 2 * n_blocks + 1): site 2i follows conv1 of block i, site 2i + 1 follows
 *   conv2 of block i, the last site is the head.
 *   Element u = c * T + t inside a block (torch's [C, T] order); in the head u = j.
 *   stream = sample * n_sites + site.
 *   Arithmetic mod 2^64:
 *     z = seed + 0x9E3779B97F4A7C15 * ((stream << 32) + u + 1)
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;
 *     z ^= z >> 27;  z *= 0x94D049BB133111EB;
 *     z ^= z >> 31;                                                                      (the splitmix64 finaliser)
 *   The element is kept iff (z >> 32) >= thr, thr = floor(p * 2^32) computed from the double p.
 *   Kept values are multiplied by float(1.0 / (1.0 - p)), dropped ones are 0.
 *   A clip's bits depend on its own seed, the sample, the site and the element, never on the clip's position in the batch.
 * lmx_h_tcn_keep_bits writes keep_host[u] = 0 / 1 for u = 0 .. count - 1 of one (seed, sample, site), on the host.
 *
 * lmx_tcn_weights_t describes one network to both forwards: DEVICE pointers for lmx_k_tcn_forward, HOST pointers for lmx_h_tcn_forward.
 *   conv_w[i][s]  convolution s (0: conv1, 1: conv2) of block i in the MFMA B-operand order, f32 [k * Q][N / 16][64][4], 16-byte aligned:
 *                 entry [j * Q + q][nt][l][e] = W[16 nt + (l & 15)][16 q + 4 (l >> 4) + e][j], 0 where that input channel is >= Cin;
 *                 Q = ceil(Cin / 16), N = channels[i], Cin = input_dim (block 0, conv1), channels[i - 1] (conv1) or channels[i] (conv2)
 *   conv_b[i][s]  f32 [N]
 *   res_w[i]      the 1 x 1 residual convolution in the same order with k = 1, NULL exactly where Cin == N;  res_b[i] f32 [N]
 *   fc1_w f32 [head][channels[n_blocks - 1]] (16-byte aligned), fc1_b [head], fc2_w [head], fc2_b [1]
 * Accepted: n_blocks 1 .. 8, channels multiples of 16 up to 64, input_dim 1 .. 64, k 2 or 3, head 1 .. 64, T 1 .. 256, one output class.
 *
 * lmx_k_tcn_forward: x f32 [n][T][input_dim] on the device; seeds_host u64 [n] on the HOST (may be NULL when S == 0), copied into
 * `workspace` (lmx_tcn_workspace_bytes(n) bytes on the device, 8-byte aligned; may be NULL when S == 0) on `stream`.  S >= 2: train mode, S
 * predictions per clip with dropout probability p in [0, 1); S == 0: eval mode, no dropout, ONE prediction per clip; S == 1 is refused
 * (its standard deviation is undefined).  pred f32 [n][max(S, 1)]; stats f32 [n][2] = the f32 mean of the clip's row of pred in sample
 * order and its two-pass unbiased (n - 1) f32 standard deviation ({pred, 0} when S == 0), written by a second kernel on the same
 * stream, so it cannot depend on which workgroup finished first; trunk (may be NULL; for tests) receives the last block's output
 * f32 [n][max(S, 1)][T][channels[last]].  Nothing else between the series and the prediction touches HBM.  Refused with LMX_EINVAL before
 * anything is launched: a configuration outside the list above (the field named), T or S out of range, tiles that do not fit the LDS
 * (the bytes in the message), null or misaligned pointers.  n = 0 launches nothing.
 * lmx_h_tcn_forward is the same network in plain C++ on HOST pointers with the same keep bits: f32, sequential sums. */
#define LMX_TCN_MAX_BLOCKS 8
typedef struct { int32_t input_dim, n_blocks, k, head; int32_t channels[LMX_TCN_MAX_BLOCKS];
                 const float* conv_w[LMX_TCN_MAX_BLOCKS][2]; const float* conv_b[LMX_TCN_MAX_BLOCKS][2];
                 const float* res_w[LMX_TCN_MAX_BLOCKS]; const float* res_b[LMX_TCN_MAX_BLOCKS];
                 const float *fc1_w, *fc1_b, *fc2_w, *fc2_b; } lmx_tcn_weights_t;
int lmx_h_tcn_keep_bits(uint64_t seed, int sample, int site, int n_sites, int64_t count, double p, uint8_t* keep_host);
int64_t lmx_tcn_workspace_bytes(int n);
int lmx_k_tcn_forward(const lmx_tcn_weights_t* w_host, const float* x /* [n][T][input_dim] */, const uint64_t* seeds_host /* [n] */,
                      int n, int T, int S, double p, float* pred /* [n][max(S,1)] */, float* stats /* [n][2] */,
                      float* trunk /* NULL or [n][max(S,1)][T][C] */, void* workspace, lmx_stream_t stream);
int lmx_h_tcn_forward(const lmx_tcn_weights_t* w_host, const float* x_host, const uint64_t* seeds_host, int n, int T, int S, double p,
                      float* pred_host, float* stats_host, float* trunk_host);
/* The feature arithmetic of services/tcn-pipeline/app/main.py:255-328 for one clip of T0 >= 1 pose frames, on the host: per frame
 * 20 keypoints as (x - bbox_x) / max(bbox_w, 1) and (y - bbox_y) / max(bbox_h, 1) with bbox = (x0, y0, x1, y1), bbox_w = x1 - x0,
 * bbox_h = y1 - y0, computed in doubles and cast to f32 (keypoints at and beyond n_kp_host[t] are 0); then (x0 + x1) / 2 / 1280,
 * (y0 + y1) / 2 / 720, bbox_w * bbox_h / (1280 * 720), and a velocity that is the difference of the FLOAT32 centroid-x column
 * (0 at the first step).  The series is then cropped at its centre (start = (T0 - target) / 2) or zero-padded at its centre
 * (pad_before = (target - T0) / 2, integer divisions) to `target` steps. */
int lmx_h_tcn_features(const double* keypoints_host /* [T0][20][2] */, const int* n_kp_host /* [T0] */, const double* bbox_host /* [T0][4] */,
                       int T0, int target, float* out_host /* [target][44] */);

/* ==== MODEL level: gait scores from pose series (csrc/gait_model.hip, csrc/tcn_image.h, csrc/host_tcn_image.cpp) =======================
 * services/tcn-pipeline/app/main.py:230-253 and :357-364 behind a handle: the model comes from a WEIGHT IMAGE (kind 4) that
 * lmx.native.write_tcn_image writes from the folded weights (csrc/tcn_image.h has the config block and the tensors); handle rules as for
 * lmx_dino.  lmx_tcn_score: x f32 [n][T][input_dim] on the device, seeds_host u64 [n] on the host -> pred f32 [n][max(S, 1)] and stats
 * f32 [n][2] on the device, lmx_k_tcn_forward with the image's dropout probability; it only enqueues on `stream`.  n <= max_clips,
 * S <= max_samples.  lmx_tcn_score_host takes and returns HOST memory, and synchronises (examples/tcn_score.c). */
typedef struct lmx_tcn lmx_tcn;
typedef struct { int32_t input_dim, n_blocks, k, head, receptive_field, max_clips, max_samples; int32_t channels[LMX_TCN_MAX_BLOCKS];
                 double p; } lmx_tcn_info_t;
int lmx_tcn_image_check_host(const char* path_host, lmx_tcn_info_t* info_host);
int lmx_tcn_open_host(const char* path_host, int max_clips, int max_samples, lmx_tcn** out_host);
void lmx_tcn_close(lmx_tcn* m);
int lmx_tcn_info(const lmx_tcn* m, lmx_tcn_info_t* info_host);
int lmx_tcn_score(lmx_tcn* m, const float* x, const uint64_t* seeds_host, int n, int T, int S, float* pred, float* stats,
                  lmx_stream_t stream);
int lmx_tcn_score_host(lmx_tcn* m, const float* x_host, const uint64_t* seeds_host, int n, int T, int S, float* pred_host,
                       float* stats_host);

/* ==== The gait transformer: score, MC-dropout spread and temporal saliency from a pose series (csrc/xfm.hip, csrc/host_xfm.cpp) ========
 * Replaces services/transformer-pipeline/app/main.py:24-237, the encoder-only pre-norm transformer over the TCN's 44 features per
 * frame, its predict_with_uncertainty (ten train-mode forwards at batch 1) and its get_attention_weights (an eleventh forward), by ONE
 * launch for n clips and S samples: one workgroup per (clip, sample), the residual stream resident in LDS from the series to the sigmoid.
 * The network (batch-free, x [T][F], T <= max_len; D = d_model, H = n_heads, dh = D / H, L = n_layers, FF = ff):
 *   h  = drop_0( x W_in^T + b_in + pe[t] )                                   pe: the table f32 [max_len][D] of the weights
 *   layer l = 0 .. L-1:
 *     a  = LN(h; g1, b1)                       eps 1e-5, biased variance, two passes (mean, then the squared deviations), 1.0f / sqrtf
 *     q, k, v = a Wq^T + bq, ...               rows 0..D-1, D..2D-1, 2D..3D-1 of in_proj_weight; head i = channels i*dh .. (i+1)*dh-1
 *     s[i][t][u] = (q_i[t] * c) . k_i[u]       c = float(1 / sqrt(dh)): 0.25 for dh 16, the rounded 0.17677669 for dh 32, applied to q
 *                                              after its bias; s = -inf where key u is masked
 *     P = drop_{1+4l}( softmax_u(s) )          max-subtracted, the accurate expf, ONE DIVISION PER ELEMENT by the row's sum
 *     o[t] = concat_i( P_i[t] . v_i )
 *     h  = h + drop_{2+4l}( o Wo^T + bo )
 *     a  = LN(h; g2, b2)
 *     h  = h + drop_{4+4l}( drop_{3+4l}( gelu( a W1^T + b1 ) ) W2^T + b2 )   gelu exact: 0.5 x (1 + erff(x * 0.70710678f))
 *   trunk = LN(h; gf, bf)
 *   pooled = sum over UNMASKED t of trunk[t] / max(count, 1)                 without a mask: the mean over T
 *   pred = 1 / (1 + expf(-( fc2 drop_{4L+1}( relu( fc1 pooled + b ) ) + b )))
 *   saliency[u] = sum_t (1/H) sum_i P_i[t][u]  of the LAST layer, eval mode only: the column sums of the head-averaged attention weights
 * All arithmetic is f32 with f32 accumulation (the exact f32-input MFMA on the device), so the device, lmx_h_xfm_forward and torch in
 * float32 differ in summation order and in the last places of expf and erff only.
 * Masking (mask u8 [n][T], nonzero = masked, NULL = none): a masked step is computed as a QUERY like any other (torch does, and trunk
 * shows it), it is never a key and never pooled.  A clip with NO unmasked step has no defined softmax: its pred is NaN, on the device
 * and on the host, as torch's is; lmx.services.TransformerPipeline refuses such a clip.
 * MC dropout: the keep decision of the TCN section above (the same mix, thr and scale), stream = sample * n_sites + site with
 * n_sites = 4 L + 2.  Element numbers follow torch's memory order:
 *   site 0 (after the positional table)         u = t * D + c
 *   site 1 + 4l (attention probabilities)       u = (i * T + t) * T + u_key
 *   sites 2 + 4l, 4 + 4l (out_proj, FFN output) u = t * D + c
 *   site 3 + 4l (FFN hidden)                    u = t * FF + j
 *   site 4L + 1 (classifier hidden)             u = j
 * lmx_h_tcn_keep_bits serves these sites as it takes n_sites.  Parity with torch's generator is statistical only.
 *
 * lmx_xfm_weights_t describes one network to both forwards: DEVICE pointers for lmx_k_xfm_forward, HOST pointers for lmx_h_xfm_forward.
 * A linear layer W [N][K] is stored as the TCN stores a convolution with one tap: f32 [Q][N / 16][64][4], Q = ceil(K / 16), entry
 * [q][nt][l][e] = W[16 nt + (l & 15)][16 q + 4 (l >> 4) + e], 0 where that input is >= K; 16-byte aligned.
 *   in_w [F -> D], in_b [D], pe [max_len][D]
 *   per layer: ln1_g, ln1_b [D]; qkv_w: H linear layers [D -> 3 dh] one after the other, layer i with the rows q_i | k_i | v_i of
 *   in_proj_weight; qkv_b [H][3 dh] in the same order; out_w [D -> D], out_b [D]; ln2_g, ln2_b [D]; ff1_w [D -> FF], ff1_b [FF];
 *   ff2_w [FF -> D], ff2_b [D]
 *   lnf_g, lnf_b [D]; fc1_w plain [head][D] (16-byte aligned), fc1_b [head], fc2_w [head], fc2_b [1]
 * Accepted: input_dim 1 .. 64, d_model in {16, 32, 48, 64}, d_model / n_heads in {16, 32}, n_layers 1 .. 8, ff a multiple of 16 up to
 * 256, head 1 .. 64, max_len 1 .. 160, T 1 .. max_len, S = 0 or 2 .. 65535, p in [0, 1).
 *
 * lmx_k_xfm_forward: x f32 [n][T][input_dim] and mask on the device, seeds_host u64 [n] on the HOST (NULL allowed when S == 0), copied
 * into `workspace` (lmx_xfm_workspace_bytes(n) bytes on the device, 8-byte aligned; NULL allowed when S == 0) on `stream`.  S as for the
 * TCN: S >= 2 train mode, S == 0 eval mode with one prediction per clip, S == 1 refused.  pred f32 [n][max(S, 1)]; stats f32 [n][2] = mean
 * and unbiased standard deviation of the clip's row of pred, by a second kernel; saliency (NULL or f32 [n][T]) only when S == 0, summed
 * without floating-point atomics in a fixed order; trunk (NULL or f32 [n][max(S, 1)][T][D]; for tests) the final LayerNorm's output.
 * Refused with LMX_EINVAL before anything is launched: a configuration outside the list (the field named), T or S out of range,
 * saliency with S > 0, tiles that do not fit the LDS (the bytes in the message), null or misaligned pointers.  n = 0 launches nothing.
 * lmx_h_xfm_forward is the same network in plain C++ on HOST pointers with the same keep bits: f32, sequential sums. */
#define LMX_XFM_MAX_LAYERS 8
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, ff, head, max_len, reserved;
                 const float *in_w, *in_b, *pe;
                 const float *ln1_g[LMX_XFM_MAX_LAYERS], *ln1_b[LMX_XFM_MAX_LAYERS], *qkv_w[LMX_XFM_MAX_LAYERS], *qkv_b[LMX_XFM_MAX_LAYERS];
                 const float *out_w[LMX_XFM_MAX_LAYERS], *out_b[LMX_XFM_MAX_LAYERS], *ln2_g[LMX_XFM_MAX_LAYERS], *ln2_b[LMX_XFM_MAX_LAYERS];
                 const float *ff1_w[LMX_XFM_MAX_LAYERS], *ff1_b[LMX_XFM_MAX_LAYERS], *ff2_w[LMX_XFM_MAX_LAYERS], *ff2_b[LMX_XFM_MAX_LAYERS];
                 const float *lnf_g, *lnf_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b; } lmx_xfm_weights_t;
int64_t lmx_xfm_workspace_bytes(int n);
int lmx_k_xfm_forward(const lmx_xfm_weights_t* w_host, const float* x /* [n][T][input_dim] */, const uint8_t* mask /* NULL or [n][T] */,
                      const uint64_t* seeds_host /* [n] */, int n, int T, int S, double p, float* pred /* [n][max(S,1)] */,
                      float* stats /* [n][2] */, float* saliency /* NULL or [n][T], S == 0 only */,
                      float* trunk /* NULL or [n][max(S,1)][T][D] */, void* workspace, lmx_stream_t stream);
int lmx_h_xfm_forward(const lmx_xfm_weights_t* w_host, const float* x_host, const uint8_t* mask_host, const uint64_t* seeds_host, int n,
                      int T, int S, double p, float* pred_host, float* stats_host, float* saliency_host, float* trunk_host);
/* The key-padding mask of services/transformer-pipeline/app/main.py:303-392 for one clip of T0 >= 1 pose frames, on the host: per frame
 * the 20 keypoint confidences (those at and beyond n_kp_host[t] count as 0) are added in index order in doubles, divided by 20,
 * multiplied by the detection confidence, cast to f32 and compared < 0.3f (1 = masked).  The mask is then cropped at its centre or padded
 * at its centre with 1 to `target` steps, with the integer divisions of lmx_h_tcn_features.  numpy's own np.mean may add in another order
 * and differ in the last place of the double: that matters only for a confidence within one such place of the threshold. */
int lmx_h_xfm_mask(const double* kp_conf_host /* [T0][20] */, const int* n_kp_host /* [T0] */, const double* det_conf_host /* [T0] */,
                   int T0, int target, uint8_t* mask_host /* [target] */);

/* ==== MODEL level: transformer gait scores from pose series (csrc/gait_model.hip, csrc/xfm_image.h, csrc/host_xfm_image.cpp) ============
 * services/transformer-pipeline/app/main.py:272-301 and :421-441 behind a handle: the model comes from a WEIGHT IMAGE (kind 5) that
 * lmx.native.write_xfm_image writes (csrc/xfm_image.h has the config block and the tensors); handle rules as for lmx_tcn.
 * lmx_xfm_score: x and mask (may be NULL) on the device, seeds_host on the host -> pred, stats and, when S == 0 and it is not NULL,
 * saliency f32 [n][T] on the device: lmx_k_xfm_forward with the image's dropout probability; it only enqueues on `stream`.
 * n <= max_clips, S <= max_samples.  lmx_xfm_score_host takes and returns HOST memory, and synchronises (examples/xfm_score.c). */
typedef struct lmx_xfm lmx_xfm;
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, ff, head, max_len, max_clips, max_samples, reserved; double p; } lmx_xfm_info_t;
int lmx_xfm_image_check_host(const char* path_host, lmx_xfm_info_t* info_host);
int lmx_xfm_open_host(const char* path_host, int max_clips, int max_samples, lmx_xfm** out_host);
void lmx_xfm_close(lmx_xfm* m);
int lmx_xfm_info(const lmx_xfm* m, lmx_xfm_info_t* info_host);
int lmx_xfm_score(lmx_xfm* m, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S, float* pred,
                  float* stats, float* saliency, lmx_stream_t stream);
int lmx_xfm_score_host(lmx_xfm* m, const float* x_host, const uint8_t* mask_host, const uint64_t* seeds_host, int n, int T, int S,
                       float* pred_host, float* stats_host, float* saliency_host);

/* ==== Pose series: the detector's outputs to tleap's pose records, the 125 x 44 series and the key-padding mask (csrc/tleap.hip,
 * csrc/tleap.h, csrc/host_tleap.cpp) ====
 * services/tleap-pipeline/app/main.py:173-313 and :479-486 in ONE launch for n clips, one workgroup per clip, on the buffers that
 * lmx_yolo_detect leaves in HBM: boxes f32 [F][max_det][4], scores f32 [F][max_det], cls i32 [F][max_det], counts i32 [F] (clamped to
 * 0 .. max_det) and, for a pose model, kpts f32 [F][max_det][K][ndim].  Clip c owns frames clip_first_host[c] .. clip_first_host[c + 1]
 * of the batch (n + 1 values from 0 to F that ascend strictly: a clip has at least one frame); h x w is the frame size.
 * ROWS.  pose_sequences holds one row per DETECTION, flattened over the frames (main.py:479-486): frames ascend, within a frame the rows
 * follow NMS order; row r of a clip comes from an exclusive scan of the per-frame row counts and rows[c] is their total T0.
 *   LMX_TLEAP_TRAINED (kpts given): every detection is a row; a frame without detections contributes nothing (main.py:152-154).
 *   LMX_TLEAP_HEURISTIC (kpts NULL): the detections whose class is one of cow_classes_host (at most LMX_TLEAP_MAX_COW_CLASSES ids,
 *     main.py:282) are rows; a frame with none contributes ONE assumed row (main.py:295-304): box [w * 0.1, h * 0.1, w * (1 - 0.1),
 *     h * (1 - 0.1)] in doubles, confidence 0.5, detection index -1.
 * RECORDS.  The caller allocates F * max_det records; clip c's rows start at record clip_first_host[c] * max_det, those at and beyond
 * rows[c] are not written.  A record holds the frame index RELATIVE to the clip's first frame, the detection index, the box (the four f32
 * widened to f64, or the assumed box), the detection confidence (f32 widened, or 0.5), n_kp and 20 keypoints (x, y, confidence) in f64,
 * zero at and beyond n_kp.
 * HEURISTIC KEYPOINTS (main.py:210-263).  x1, y1, x2, y2 = the box corners truncated toward zero (Python's int); width = x2 - x1,
 * height = y2 - y1; all arithmetic in doubles, one rounding per operation, in the reference's order: head_x = x1 + width * 0.1,
 * head_y = y1 + height * 0.3, front_x = x1 + width * 0.25, back_x = x1 + width * 0.75, ground_y = y2 - height * 0.05 are rounded before
 * they are used.  In slot order, (x; y; confidence):
 *    0 left_eye   head_x - width*0.02; head_y - height*0.05; 0.7      1 right_eye  head_x + width*0.02; head_y - height*0.05; 0.7
 *    2 nose       head_x; head_y + height*0.05; 0.8                   3 left_ear   head_x - width*0.05; head_y - height*0.1; 0.6
 *    4 right_ear  head_x + width*0.05; head_y - height*0.1; 0.6       5 / 6 left / right_front_elbow  front_x -/+ width*0.05; y1 + height*0.4; 0.7
 *    7 / 8 left / right_back_elbow  back_x -/+ width*0.05; y1 + height*0.4; 0.7
 *    9 left_front_knee  front_x - width*0.03; y1 + height*0.6; 0.7    10 right_front_knee  front_x + width*0.07; y1 + height*0.6; 0.7
 *   11 left_back_knee   back_x - width*0.07; y1 + height*0.6; 0.7     12 right_back_knee   back_x + width*0.03; y1 + height*0.6; 0.7
 *   13 left_front_paw   front_x - width*0.02; ground_y; 0.7           14 right_front_paw   front_x + width*0.08; ground_y; 0.7
 *   15 left_back_paw    back_x - width*0.08; ground_y; 0.7            16 right_back_paw    back_x + width*0.02; ground_y; 0.7
 *   17 throat  x1 + width*0.15; y1 + height*0.25; 0.8                 18 withers  x1 + width*0.3; y1 + height*0.15; 0.8
 *   19 tailbase  x1 + width*0.9; y1 + height*0.25; 0.7
 * TRAINED BLEND (main.py:177-188).  n_kp = min(K, 20); keypoint i < n_kp is the model's: x and y f32 widened, the confidence f32 widened
 * or 1.0 when ndim == 2; keypoints beyond 20 are dropped as the reference drops kp_{i}.  The only name the model's list and the heuristic
 * list share is withers, slot 2 of the model's list: when its widened confidence is not > 0.3 (the double), the heuristic withers
 * (x1 + width*0.3, y1 + height*0.15, 0.8) replaces it.
 * SERIES AND MASK.  series f32 [n][target][44] and mask u8 [n][target] are exactly lmx_h_tcn_features and lmx_h_xfm_mask of the clip's
 * records (divisions against the record's f64 box, the velocity differenced before the crop, padding masked); T0 = 0 gives a zero series
 * and a full mask.
 * Refused with LMX_EINVAL before anything is launched, the argument named: a null or misaligned pointer (4 bytes; records and workspace
 * 8), F < 1, max_det < 1, h or w below 1, n < 1, ndim outside {2, 3} or K < 3 or K > 4096 with kpts, kpts that do not fit the mode,
 * target outside 1 .. 65536, n_cow outside 0 .. LMX_TLEAP_MAX_COW_CLASSES, a mode that is neither, and clip_first_host that does not
 * start at 0, ascend strictly and end at F.  workspace: lmx_tleap_workspace_bytes(F, max_det) bytes on the device (the clip bounds and
 * the row maps), 0 for a size it refuses.  No atomics; bits do not depend on the batch a clip rides in.  lmx_h_tleap_series is the same
 * contract on HOST pointers in plain C++ (it calls lmx_h_tcn_features and lmx_h_xfm_mask for the second half). */
enum { LMX_TLEAP_TRAINED = 0, LMX_TLEAP_HEURISTIC = 1, LMX_TLEAP_KEYPOINTS = 20, LMX_TLEAP_MAX_COW_CLASSES = 16 };
typedef struct { int32_t frame, det; double bbox[4]; double confidence; int32_t n_kp, reserved; double keypoints[LMX_TLEAP_KEYPOINTS][3]; }
    lmx_tleap_record_t;  /* 536 bytes */
int64_t lmx_tleap_workspace_bytes(int F, int max_det);
int lmx_k_tleap_series(const float* boxes, const float* scores, const int32_t* cls, const int32_t* counts, const float* kpts /* or NULL */,
                       int K, int ndim, int F, int max_det, int h, int w, const int32_t* clip_first_host /* [n + 1] */, int n, int target,
                       int mode, const int32_t* cow_classes_host /* [n_cow] */, int n_cow, int32_t* rows /* [n] */,
                       lmx_tleap_record_t* records /* [F * max_det] */, float* series /* [n][target][44] */, uint8_t* mask /* [n][target] */,
                       void* workspace, lmx_stream_t stream);
int lmx_h_tleap_series(const float* boxes_host, const float* scores_host, const int32_t* cls_host, const int32_t* counts_host,
                       const float* kpts_host, int K, int ndim, int F, int max_det, int h, int w, const int32_t* clip_first_host, int n,
                       int target, int mode, const int32_t* cow_classes_host, int n_cow, int32_t* rows_host, lmx_tleap_record_t* records_host,
                       float* series_host, uint8_t* mask_host);
/* compute_locomotion_features (main.py:338-436) over one clip's records, on the host.  names_host: the 20 names the caller assigns to the
 * keypoint slots; the features look up nose, throat, withers, tailbase and left_front_paw, right_front_paw, left_back_paw, right_back_paw
 * BY NAME (the last slot with a name wins, as in a dict), so the heuristic names above yield every feature while a trained model's names
 * match withers only and yield NONE: the reference's quirk, kept.  Rows with n_kp < 20 are skipped (main.py:360); fewer than 2 rows give
 * nothing.  A keypoint counts when its confidence is > 0.3.  Sums are sequential, in doubles; a standard deviation is the population's,
 * sqrt(sum((v - mean)^2) / count); the spine angle is acos(clamp(dot / (|v1| * |v2| + 1e-6), -1, 1)) * (180 / pi) with |v| = sqrt(x*x + y*y);
 * head_bob_frequency is the sum of |sign(d[i + 1]) - sign(d[i])| over the differences d of the nose's y, halved; an asymmetry is
 * |a - b| / (a + b + 1e-6); lameness_score is the mean of the scores that exist.  The reference OMITS keys: bit i of `present` says that
 * field i (in the order below, back_arch_mean = bit 0) was computed, the others are 0.  numpy adds pairwise, so its last places may
 * differ from these sequential sums. */
typedef struct {
  double back_arch_mean, back_arch_std, back_arch_score, head_bob_magnitude, head_bob_frequency, head_bob_score, stride_fl_mean,
      stride_fl_std, stride_fr_mean, stride_fr_std, stride_rl_mean, stride_rl_std, stride_rr_mean, stride_rr_std, front_leg_asymmetry,
      rear_leg_asymmetry, lameness_score;
  uint32_t present, reserved;
} lmx_tleap_locomotion_t;
int lmx_h_tleap_locomotion(const lmx_tleap_record_t* records_host, int rows, const char* const* names_host /* [20] */,
                           lmx_tleap_locomotion_t* out_host);

/* ==== The graph transformer: a cow's lameness score, its MC-dropout spread, node scores and attention per graph (csrc/gfm.hip,
 * csrc/host_gfm.cpp) ====
 * Replaces services/graph-transformer-pipeline/app/model/{graphormer,encodings,attention,layers}.py: CowLamenessGraphormer over one
 * graph per cow (a node per video), its predict_with_uncertainty (ten train-mode forwards of several hundred launches each) and the
 * eleventh eval-mode forward for node scores and attention, each of which recomputes all-pairs shortest paths on the host.  Here the
 * graph is prepared ONCE on the host (lmx_h_gfm_graph), the attention bias ONCE per graph on the device, and n graphs x S samples run in
 * ONE launch: one workgroup per (graph, sample), the residual stream resident in LDS from the node features to the sigmoid.
 * The network (batch-free, x [N][F]; D = d_model, H = n_heads, dh = D / H, L = n_layers, FF = ff):
 *   h  = drop_0( LN( x W_in^T + b_in ) ) + enc                     the encoding is added AFTER the dropout
 *   enc[i] = ( deg_in[min(in_deg_i, max_degree)] + deg_out[min(out_deg_i, max_degree)] ) + ( pe_i W_t^T + b_t )
 *            the time term only when the graph has timestamps: days_i = min((t_i - min t) / 86400, 365) in f32 from f32 timestamps,
 *            pe_i[2k] = sinf(days_i * div_term[k]), pe_i[2k + 1] = cosf(days_i * div_term[k]); div_term comes from the weights
 *   bias[head][i][j] = spd[idx(i, j)][head] + edge_mlp(edge_attr[e])[head]    e = the edge i -> j; the edge term is 0 without an edge
 *            idx = min(spd, max_spd) + 1 over the UNDIRECTED graph; unreachable pairs and pairs beyond max_spd both map to max_spd + 1;
 *            idx = 1 on the diagonal.  edge_mlp = Linear(3 -> 2H), ReLU, Linear(2H -> H); no dropout touches it, so the bias is the same
 *            for every sample of a graph.  Where two edges share (src, dst) THE LATER EDGE IN EDGE ORDER WINS (lmx_h_gfm_graph lists
 *            kNN edges first, so a temporal edge wins).  The reference assigns bias[src, dst] = ... with duplicate indices, which torch
 *            leaves undefined; the rule is pinned by this text, not by torch.
 *   layer l = 0 .. L-1:
 *     a  = LN(h; g1, b1)                       eps 1e-5, biased variance, two passes (mean, then the squared deviations), 1.0f / sqrtf
 *     q, k, v = a Wq^T + bq, ...               separate q_proj / k_proj / v_proj; head i = channels i*dh .. (i+1)*dh-1
 *     s[i][t][u] = (q_i[t] . k_i[u]) * c + bias[i][t][u]      c = float(dh^-0.5): 0.25 for dh 16, the rounded 0.17677669 for dh 32
 *     P = drop_{1+6l}( softmax_u(s) )          max-subtracted, the accurate expf, ONE DIVISION PER ELEMENT by the row's sum
 *     h  = h + drop_{2+6l}( concat_i( P_i v_i ) Wo^T + bo )
 *     a  = LN(h; g2, b2)
 *     h  = h + drop_{4+6l}( drop_{3+6l}( gelu( a W1^T + b1 ) ) W2^T + b2 )    gelu exact: 0.5 x (1 + erff(x * 0.70710678f))
 *     the virtual-node attention: rows [vn_l ; h], N + 1 of them; vn_l is layer l's OWN parameter, not carried from the layer before.
 *       The same attention with its own weights, the bias extended by a zero row and a zero column, NO LayerNorm in front and NO
 *       residual: y = drop_{6+6l}( concat_i( drop_{5+6l}(softmax(s))_i v_i ) Wo^T + bo ), and rows 1 .. N of y REPLACE h.
 *       vn = LN( gelu( y[0] U1^T + c1 ) U2^T + c2 ) (D -> 2D -> D) is used of the LAST layer only: the earlier ones are dead and are
 *       not computed.
 *   trunk = LN(h; gf, bf)
 *   r  = LN( relu( [ mean_i trunk[i] ; vn ; sum_i a_i trunk[i] ] Wc^T + bc ) )      a = softmax over the nodes of
 *                                                                                    tanhf( trunk A1^T + a1 ) A2^T + a2  (D -> D/2 -> 1)
 *   pred = 1 / (1 + expf(-( P3 drop_{6L+2}( relu( P2 drop_{6L+1}( relu( P1 r + p1 ) ) + p2 ) ) + p3 )))       D -> D/2 -> D/4 -> 1
 *   node_pred[i] = 1 / (1 + expf(-( N2 relu( N1 trunk[i] + n1 ) + n2 )))            eval mode only (site 6L+3 is numbered, never drawn:
 *                                                                                    the reference discards its train-mode node scores)
 *   attn_to_target[i] = (1/H) sum_head P_head[i][target]   of the LAST layer's GRAPH attention (not its virtual-node attention), eval
 *                                                          mode only; the heads are added in ascending order
 * All arithmetic is f32 with f32 accumulation (the exact f32-input MFMA on the device), LayerNorm in two passes, the accurate expf /
 * erff / tanhf / sinf / cosf: the device, lmx_h_gfm_forward and torch in float32 differ in summation order and in the last places of
 * those functions only.
 * MC dropout: the keep decision of the TCN section above (the same mix, thr and scale), stream = sample * n_sites + site with
 * n_sites = 6 L + 4.  Element numbers u (i, j count nodes from 0; in the virtual-node attention row / column 0 is the virtual node):
 *   site 0 (input)                                  u = i * D + c
 *   site 1 + 6l (attention probabilities)           u = (head * N + i) * N + j
 *   sites 2 + 6l, 4 + 6l (out_proj, FFN output)     u = i * D + c
 *   site 3 + 6l (FFN hidden)                        u = i * FF + j
 *   site 5 + 6l (virtual-node attention probabilities)   u = (head * (N+1) + i) * (N+1) + j
 *   site 6 + 6l (virtual-node out_proj)             u = i * D + c over N + 1 rows
 *   sites 6L + 1, 6L + 2 (the graph head's hidden layers)   u = j
 *   site 6L + 3 (the node head)                     numbered but never drawn
 * lmx_h_tcn_keep_bits serves these sites unchanged.  Parity with torch's generator is statistical only.
 *
 * The graph a caller hands over is prepared by lmx_h_gfm_graph on the HOST from f32 embeddings [N][E], optional f32 timestamps [N] and k
 * (GraphormerGraphBuilder); N 1 .. LMX_GFM_MAX_NODES.  The rules are pinned HERE where numpy's cannot be:
 *   kNN edges first: cosine similarity in DOUBLE from the f32 embeddings (each row divided by its norm + 1e-8, the products added in
 *   ascending channel order); k = min(k, N - 1); the neighbours of i are the k most similar j != i, listed as edges i -> j in ASCENDING
 *   similarity (the reference's argsort[-k:]), EXACT TIES GOING TO THE LOWER INDEX FIRST; weight = max(0, sim) rounded to f32;
 *   attributes (weight, 1, 0).
 *   Temporal edges then, only with timestamps and N > 1: the nodes in ascending timestamp, STABLE IN INDEX for equal timestamps (the
 *   service defaults a missing one to 0.0); consecutive nodes a, b are joined a -> b, then b -> a; weight = exp(-|t_b - t_a| / 86400)
 *   in double from the f32 timestamps, rounded to f32; attributes (weight, 0, 1).
 *   deg_in / deg_out: incoming / outgoing edges counted with duplicates, clamped to max_degree.  win[i][j] = the LAST edge i -> j in
 *   edge order, or -1.  idx[i][j] as above, by a breadth-first search per node over the symmetrised edge set.
 *   Unpinned against numpy: the BLAS summation order and float32 products of its similarity matrix, its f32 exp, and argsort on ties
 *   (an unstable quicksort); a graph without similarity ties and with distinct timestamps comes out the same.
 * edges_host must hold N * min(k, N-1) + 2 * (N-1) pairs (src, dst), edge_attr_host as many triples.
 *
 * lmx_gfm_graphs_t describes n graphs of differing N to both forwards, nodes, edges and matrices concatenated in graph order:
 *   node_off_host, edge_off_host  i32 [n + 1] on the HOST, ascending from 0: graph g has N_g = node_off[g+1] - node_off[g] nodes and its
 *                                 edges are edge_off[g] .. edge_off[g+1] - 1
 *   x f32 [sum N][input_dim]; timestamps NULL or f32 [sum N]; has_time NULL (no graph has timestamps) or u8 [n];
 *   deg_in, deg_out u8 [sum N]; idx u8 [sum N^2] and win i32 [sum N^2] (graph g's [N_g][N_g] matrix starts at sum_{g' < g} N_g'^2; win
 *   counts from the graph's first edge); edge_attr f32 [sum E][3]; target NULL or i32 [n] (the node whose attention column is read)
 *   DEVICE pointers for lmx_k_gfm_forward, HOST pointers for lmx_h_gfm_forward (the two offset arrays are on the host for both).
 *   node_off_host, edge_off_host and seeds_host are copied to the device asynchronously: they must stay valid and unchanged until the
 *   work enqueued on `stream` has run (for a caller that frees or reuses them at once: until the stream is synchronised).  The device
 *   arrays must live on the stream's device.
 * lmx_gfm_weights_t describes one network to both forwards likewise.  A linear layer marked "packed" is stored as the gait transformer
 * stores one (f32 [Q][N / 16][64][4], 16-byte aligned); one marked "transposed" is the plain W^T, f32 [K][N].
 *   in_w packed [F -> D], in_b, in_g, in_beta [D]; deg_in, deg_out [max_degree + 1][D]; time_w packed [D -> D], time_b [D],
 *   div_term [D / 2]; spd [max_spd + 2][H]; e1_w plain [2H][3], e1_b [2H], e2_w plain [H][2H], e2_b [H]
 *   per layer: ln1_g, ln1_b; qkv_w: H packed layers [D -> 3 dh] one after the other (rows q_i | k_i | v_i), qkv_b [H][3 dh]; out_w packed
 *   [D -> D], out_b; ln2_g, ln2_b; ff1_w packed [D -> FF], ff1_b; ff2_w packed [FF -> D], ff2_b; vn [D]; vqkv_w, vqkv_b, vout_w, vout_b
 *   the virtual-node attention's, as qkv / out
 *   vu1_w transposed [D][2D], vu1_b [2D], vu2_w transposed [2D][D], vu2_b, vu_g, vu_beta [D]: vn_update of the LAST layer
 *   lnf_g, lnf_b; pool1_w packed [D -> PD], pool1_b [PD], pool2_w [PD], pool2_b [1], PD = D / 2 rounded up to 16 with zeros;
 *   comb_w transposed [3D][D], comb_b, comb_g, comb_beta [D]; ph1_w transposed [D][D/2], ph1_b; ph2_w transposed [D/2][D/4], ph2_b;
 *   ph3_w [D/4], ph3_b [1]; nh1_w packed [D -> PD], nh1_b [PD], nh2_w [PD], nh2_b [1]
 * Accepted: d_model a multiple of 16 up to 128; d_model / n_heads 16 or 32; n_layers 1 .. 8; ff a multiple of 16 up to 512; input_dim
 * 1 .. 64; edge_dim 3; max_degree 0 .. 255; max_spd >= 0 with max_spd + 2 <= 32; N 1 .. LMX_GFM_MAX_NODES per graph; S = 0 or
 * 2 .. 65535; p in [0, 1).  LMX_GFM_MAX_NODES = 95: with the virtual node 96 rows of the residual stream, the LayerNorm output (132
 * floats each) and the work tile (100 floats for a head width of 32) plus the waves' patches and the readout's vectors are 154,624 of
 * the 163,840 bytes of LDS; 112 rows would need 178 KB.
 *
 * lmx_k_gfm_forward: seeds_host u64 [n] on the HOST (NULL allowed when S == 0).  `workspace`: lmx_gfm_workspace_bytes(n, cells, H) bytes
 * on the device, 16-byte aligned, cells = sum N^2; it receives the seeds, the two offset arrays and bias f32 [H][N][N] per graph, filled
 * by a small kernel in front of the forward on the same stream.  pred f32 [n][max(S, 1)]; stats f32 [n][2] as for the TCN; with S == 0
 * only: node_pred f32 [sum N] and attn_to_target f32 [sum N] (NULL allowed; the latter needs target), summed in a fixed order without
 * floating-point atomics; for tests: trunk f32, graph g's [max(S, 1)][N_g][D] starting at node_off[g] * max(S, 1) * D, and vn f32
 * [n][max(S, 1)][D] (NULL allowed).  Rows beyond a graph's N stay finite, are never keys, are never pooled and never leave the LDS.
 * Refused with LMX_EINVAL before anything is launched: a configuration outside the list (the field named), offsets that do not ascend
 * from 0, an N outside 1 .. LMX_GFM_MAX_NODES, S or p out of range, node_pred / attn_to_target with S > 0, null or misaligned
 * pointers.  n = 0 launches nothing.
 * lmx_h_gfm_forward is the same network in plain C++ on HOST pointers with the same keep bits: f32, sequential sums. */
#define LMX_GFM_MAX_LAYERS 8
#define LMX_GFM_MAX_NODES 95
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd;
                 const float *in_w, *in_b, *in_g, *in_beta, *deg_in, *deg_out, *time_w, *time_b, *div_term, *spd, *e1_w, *e1_b, *e2_w, *e2_b;
                 const float *ln1_g[LMX_GFM_MAX_LAYERS], *ln1_b[LMX_GFM_MAX_LAYERS], *qkv_w[LMX_GFM_MAX_LAYERS], *qkv_b[LMX_GFM_MAX_LAYERS];
                 const float *out_w[LMX_GFM_MAX_LAYERS], *out_b[LMX_GFM_MAX_LAYERS], *ln2_g[LMX_GFM_MAX_LAYERS], *ln2_b[LMX_GFM_MAX_LAYERS];
                 const float *ff1_w[LMX_GFM_MAX_LAYERS], *ff1_b[LMX_GFM_MAX_LAYERS], *ff2_w[LMX_GFM_MAX_LAYERS], *ff2_b[LMX_GFM_MAX_LAYERS];
                 const float *vn[LMX_GFM_MAX_LAYERS], *vqkv_w[LMX_GFM_MAX_LAYERS], *vqkv_b[LMX_GFM_MAX_LAYERS], *vout_w[LMX_GFM_MAX_LAYERS];
                 const float *vout_b[LMX_GFM_MAX_LAYERS];
                 const float *vu1_w, *vu1_b, *vu2_w, *vu2_b, *vu_g, *vu_beta, *lnf_g, *lnf_b, *pool1_w, *pool1_b, *pool2_w, *pool2_b;
                 const float *comb_w, *comb_b, *comb_g, *comb_beta, *ph1_w, *ph1_b, *ph2_w, *ph2_b, *ph3_w, *ph3_b;
                 const float *nh1_w, *nh1_b, *nh2_w, *nh2_b; } lmx_gfm_weights_t;
typedef struct { int32_t n, reserved; const int32_t *node_off_host, *edge_off_host; const float *x, *timestamps; const uint8_t* has_time;
                 const uint8_t *deg_in, *deg_out, *idx; const int32_t* win; const float* edge_attr; const int32_t* target; } lmx_gfm_graphs_t;
int lmx_h_gfm_graph(const float* emb_host /* [N][E] */, const float* timestamps_host /* NULL or [N] */, int N, int E, int k, int max_degree,
                    int max_spd, int32_t* edges_host /* [cap][2] */, float* edge_attr_host /* [cap][3] */, int32_t* n_edges_host,
                    uint8_t* deg_in_host /* [N] */, uint8_t* deg_out_host /* [N] */, uint8_t* idx_host /* [N][N] */,
                    int32_t* win_host /* [N][N] */);
int64_t lmx_gfm_workspace_bytes(int n, int64_t cells, int n_heads);
int lmx_k_gfm_forward(const lmx_gfm_weights_t* w_host, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host /* [n] */, int S,
                      double p, float* pred /* [n][max(S,1)] */, float* stats /* [n][2] */, float* node_pred /* NULL or [sum N], S == 0 */,
                      float* attn_to_target /* NULL or [sum N], S == 0 */, float* trunk /* NULL or [sum N][max(S,1)][D] */,
                      float* vn /* NULL or [n][max(S,1)][D] */, void* workspace, lmx_stream_t stream);
int lmx_h_gfm_forward(const lmx_gfm_weights_t* w_host, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, double p,
                      float* pred_host, float* stats_host, float* node_pred_host, float* attn_to_target_host, float* trunk_host,
                      float* vn_host);

/* ==== MODEL level: graph scores from prepared graphs (csrc/graph_model.hip, csrc/gfm_image.h, csrc/host_gfm_image.cpp) ================
 * services/graph-transformer-pipeline/app/main.py behind a handle: the model comes from a WEIGHT IMAGE (kind 6) that
 * lmx.native.write_gfm_image writes (csrc/gfm_image.h has the config block and the tensors); handle rules as for lmx_tcn.  The handle
 * owns the workspace for max_graphs graphs of max_nodes_total nodes in all.  lmx_gfm_score: the graphs as for lmx_k_gfm_forward (DEVICE
 * arrays, the two offset arrays on the host), seeds_host on the host -> pred, stats and, when S == 0 and they are not NULL, node_pred and
 * attn_to_target on the device: lmx_k_gfm_forward with the image's dropout probability; it only enqueues on `stream`.  n <= max_graphs,
 * sum N <= max_nodes_total, S <= max_samples.  lmx_gfm_score_host takes the graphs' arrays and returns the outputs in HOST memory, and
 * synchronises (examples/gfm_score.c). */
typedef struct lmx_gfm lmx_gfm;
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd, max_nodes, max_graphs, max_nodes_total,
                 max_samples; double p; } lmx_gfm_info_t;
int lmx_gfm_image_check_host(const char* path_host, lmx_gfm_info_t* info_host);
int lmx_gfm_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_samples, lmx_gfm** out_host);
void lmx_gfm_close(lmx_gfm* m);
int lmx_gfm_info(const lmx_gfm* m, lmx_gfm_info_t* info_host);
int lmx_gfm_score(lmx_gfm* m, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* pred, float* stats,
                  float* node_pred, float* attn_to_target, lmx_stream_t stream);
int lmx_gfm_score_host(lmx_gfm* m, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* pred_host,
                       float* stats_host, float* node_pred_host, float* attn_to_target_host);

/* ==== GraphGPS: node scores, their MC-dropout spread and a cow score per graph (csrc/gnn.hip, csrc/host_gnn.cpp) ======================
 * Replaces EnhancedGraphGPS of services/gnn-pipeline/app/main.py: its predict_with_uncertainty (ten train-mode forwards, each of which
 * rebuilds a sparse Laplacian, runs an eigensolver and 16 dense matrix powers on the host) and the eleventh eval-mode forward.  Here
 * the graph and both raw encodings are prepared ONCE on the host (lmx_h_gnn_graph) and n graphs x S samples run in ONE launch, one
 * workgroup per (graph, sample), the residual stream resident in LDS.
 * ONLY THE LIVE NETWORK IS BUILT.  forward() returns pred_head(final_norm(h)) with h taken after pre_pool_layers (num_layers / 2 of
 * them); pool_layer, post_pool_layers and multi_scale_readout feed scale_representations, which nothing reads, and the e_new of the
 * last pre-pool layer (edge_update, bn_edge) feeds only that branch.  n_layers below counts the LIVE layers.
 * The network (x [N][F]; D = d_model, P = pe_dim, H = n_heads, dh = D / H, L = n_layers, FF = ff; edges e = (src, dst), E of them):
 *   h  = [ x W_in^T + b_in | LN_P( relu(|lap| L1^T) L2^T ) | LN_P( relu(rw R1^T) R2^T ) ]      D - 2P | P | P columns, biases as usual;
 *        lap f32 [N][8] and rw f32 [N][16] are the RAW encodings of lmx_h_gnn_graph (the absolute value is taken there)
 *   ea = LN_D( relu(attr W_e1^T + b_e1) W_e2^T + b_e2 )                     3 -> D/2 -> D, per edge; no dropout touches h or ea
 *   layer l = 0 .. L-1:
 *     a  = LN(h; norm1)                     eps 1e-5, biased variance, two passes, 1.0f / sqrtf everywhere
 *     Ax | Bx | Dx | Ex = a [A;B;D;E]^T + b
 *     Ce = ea C^T + c;  sigma = 1 / (1 + expf(-((Ce + Dx[dst]) + Ex[src])));  message = sigma * Bx[src]
 *     agg[i] = ( sum of the messages of the edges INTO i, IN EDGE ORDER, one running f32 sum ) / max(indeg_i, 1)
 *     l < L-1 only:  ea = BN_edge( relu( [Dx[dst] | Ex[src] | Ce] U1^T + u1 ) U2^T + u2 )
 *     h  = h + drop_{5l}( relu( BN_node( Ax + agg ) ) )
 *     a  = LN(h; norm2);  q | k | v = a Wqkv^T + b        nn.MultiheadAttention's in_proj rows: q, then k, then v; head i = channels
 *                                                          i dh .. (i+1) dh - 1 of each
 *     P  = drop_{5l+1}( softmax_u( (q_i[t] . k_i[u]) * c ) )     c = float(dh^-0.5); max-subtracted, ONE DIVISION PER ELEMENT
 *     g  = LN( a + drop_{5l+2}( concat_i(P_i v_i) Wo^T + bo ); global_attn.norm );   h = h + (g - a)
 *     a  = LN(h; norm3);  h = h + drop_{5l+4}( drop_{5l+3}( gelu(a W1^T + b1) ) W2^T + b2 )        gelu exact (erff)
 *   t  = LN(h; final_norm)
 *   node_pred[i] = 1 / (1 + expf(-( N2 drop_{5L}( relu(N1 t[i] + n1) ) + n2 )))                    D -> D/2 -> 1
 *   eval mode only: w = softmax over the nodes of ( tanhf(t A1^T + a1) A2^T + a2 ) (max-subtracted, e_i / sum) = attention_weights;
 *   graph_pred = 1 / (1 + expf(-( K3 relu( K2 relu( K1 [ mean_i t[i] | sum_i w_i t[i] ] + k1 ) + k2 ) + k3 )))   2D -> D -> D/2 -> 1;
 *   the sums over the nodes in ascending order.  The classifier's two dropout sites are never drawn: graph_pred is read in eval mode.
 * BatchNorm (eps 1e-5).  S > 0 is predict_with_uncertainty, which calls train(): bn_node normalises with the mean and BIASED variance
 * over the graph's N nodes, bn_edge over its E edges (two passes).  S = 0 normalises with the checkpoint's running_mean / running_var.
 * The reference's running statistics drift with every video it scores (momentum 0.1); that drift is NOT reproduced: a graph scores
 * to the same bytes whatever was scored before.  A graph of one node has no batch statistics: N < 2 (and, with L > 1, E < 2) is
 * refused with S > 0, as torch raises and the reference writes no result.
 * MC dropout: the keep decision of the TCN section (same mix, thr, scale), stream = sample * n_sites + site, n_sites = 5 L + 1, seeded
 * per graph.  Element numbers u (i, j count nodes from 0):
 *   site 5l (message passing), 5l+2 (out_proj), 5l+4 (FFN output)   u = i * D + c
 *   site 5l+1 (attention probabilities)                             u = (head * N + i) * N + j
 *   site 5l+3 (FFN hidden)                                          u = i * FF + j
 *   site 5L (node head)                                             u = i * (D / 2) + j
 * No floating-point atomics anywhere: every sum has a fixed order, so a graph gives the same bytes on every run, at every batch
 * position and for every S (sample s depends on (seed, s) only).
 *
 * lmx_h_gnn_graph prepares a graph on the HOST from f32 embeddings [N][E], optional f64 timestamps [N] (the reference keeps them as
 * Python floats) and k (GraphBuilder):
 *   kNN edges first: cosine similarity in DOUBLE (each row divided by its norm + 1e-8, products added in ascending channel order);
 *   k = max(1, N - 1) where N <= k; the neighbours of i are the k most similar j != i, edges i -> j in ASCENDING similarity, EXACT
 *   TIES TO THE LOWER INDEX FIRST; weight = the RAW cosine rounded to f32 (not clamped); attributes (weight, 1, 0).  N = 1: no edge.
 *   Temporal edges then, only with timestamps (a known cow) and N > 1: nodes in ascending timestamp, STABLE in index; consecutive a, b
 *   give a -> b then b -> a with weight tanh(|t_b - t_a| / 86400) in double, rounded to f32; (weight, 0, 1).
 *   Multi-edges stay multi-edges.  csr_ptr i32 [N + 1], csr_edge i32 [E]: the edges by DESTINATION, those of one destination in edge
 *   order.  deg i32 [N]: the in-degree, clamped to at least 1.
 *   RWPE: A counts multiplicities and carries one self-loop per node; P = D^-1 A in double (row sums); rw[i][k-1] = (P^k)[i][i] for
 *   k = 1 .. 16, every inner product summed in ascending index order, then rounded to f32.
 *   LapPE: the same A; deg its row sums; L = I - D^-1/2 A D^-1/2 in double (A is NOT symmetric: kNN edges are directed), then L IS
 *   SYMMETRISED FROM ITS LOWER TRIANGLE (what numpy's eigh reads); a cyclic Jacobi eigendecomposition in double runs until the
 *   off-diagonal Frobenius norm is <= 1e-14 times the matrix's (at most 64 sweeps); eigenvalues ascending, TIES BY THE LOWER ORIGINAL
 *   COLUMN; lap = |columns 1 .. 8|, zero columns where N <= 8, rounded to f32.  This equals the reference's np.linalg.eigh branch
 *   (N <= 9) wherever the spectrum is simple.  For N > 9 the reference runs eigsh(which='SM', tol=1e-3) from a random start vector on
 *   the non-symmetric matrix: parity there is unpinned and unattainable.
 *   Unpinned against numpy, as for the graph transformer: the BLAS order of its similarity matrix and tanh in the last place.
 * edges_host holds N * min(max(k, 1), N - 1) + 2 (N - 1) pairs at most.  LMX_GNN_MAX_NODES = 95 and E <= LMX_GNN_MAX_EDGES =
 * 5 * 95 + 2 * 94 = 663 per graph, the graph transformer's cows.  LDS at the limit: three tiles of 96 rows x 132 floats (residual
 * stream, LayerNorm output / aggregation, work tile) and 1,664 floats of vectors are 158,720 of 163,840 bytes.
 *
 * lmx_gnn_graphs_t: n graphs concatenated in graph order; node_off_host / edge_off_host i32 [n + 1] on the HOST, ascending from 0;
 *   x f32 [sum N][input_dim]; lap f32 [sum N][8]; rw f32 [sum N][16]; edge_src, edge_dst i32 [sum E] (nodes counted within the graph);
 *   edge_attr f32 [sum E][3]; csr_ptr i32 [sum N + n] (graph g's N_g + 1 entries start at node_off[g] + g); csr_edge i32 [sum E] (edges
 *   counted within the graph); deg i32 [sum N].  DEVICE pointers for lmx_k_gnn_forward, HOST pointers for lmx_h_gnn_forward.  The
 *   device forward clamps every index it reads into its graph; the host forward refuses an index outside.
 * lmx_gnn_weights_t: "packed" and "transposed" as for the graph transformer.
 *   in_w packed [F -> D - 2P], in_b; lap1_w plain [2P][8], lap1_b, lap2_w plain [P][2P], lap2_b, lap_g, lap_beta [P]; rw1_w plain
 *   [2P][16], rw1_b, rw2_w, rw2_b, rw_g, rw_beta likewise; ee1_w plain [D/2][3], ee1_b, ee2_w packed [D/2 -> D], ee2_b, ee_g, ee_beta
 *   per layer: ln1_g, ln1_b; abde_w packed [D -> 4D] (rows A | B | D | E), abde_b [4D]; c_w packed [D -> D], c_b; eu1_w packed
 *   [3D -> D], eu1_b, eu2_w packed [D -> D], eu2_b, bne_g, bne_b, bne_mean, bne_var (these eight NULL in the last layer); bnn_g, bnn_b,
 *   bnn_mean, bnn_var; ln2_g, ln2_b; qkv_w: H packed layers [D -> 3 dh] (rows q_i | k_i | v_i), qkv_b [H][3 dh]; out_w packed, out_b;
 *   lna_g, lna_b (global_attn.norm); ln3_g, ln3_b; ff1_w packed [D -> FF], ff1_b; ff2_w packed [FF -> D], ff2_b
 *   lnf_g, lnf_b; nh1_w packed [D -> D/2], nh1_b, nh2_w [D/2], nh2_b [1]; na1_w packed [D -> D/2], na1_b, na2_w [D/2], na2_b [1];
 *   cl1_w transposed [2D][D], cl1_b; cl2_w transposed [D][D/2], cl2_b; cl3_w [D/2], cl3_b [1]
 * Accepted: d_model a multiple of 32 up to 128; d_model / n_heads 16 or 32; pe_dim a multiple of 8 with 2 pe_dim < d_model; n_layers
 * 1 .. 4; ff a multiple of 16 up to 512; input_dim 1 .. 64; edge_dim 3; N 1 .. LMX_GNN_MAX_NODES and E 0 .. LMX_GNN_MAX_EDGES per
 * graph; S = 0 or 2 .. 65535; p in [0, 1).
 * lmx_k_gnn_forward: `workspace`: lmx_gnn_workspace_bytes(n, S, max N, max E, D, L) bytes on the device, 16-byte aligned: the seeds,
 * the offsets, and one slice per workgroup for Bx | Dx | Ex [N][3D] and, with L > 1, the first layers' ea [E][D] (written once, read
 * once; its batch statistics in a pass of their own): n x max(S, 1) x (max N x 3D + max E x D) x 4 bytes, 485,376 bytes per
 * (graph, sample) for the shipped network at the limits, 310 MB for 64 such graphs x 10 samples.  S > 0: node_mc f32 [sum N][S] and stats f32 [sum N][2] (mean, unbiased std).
 * S = 0: graph_pred f32 [n], node_pred f32 [sum N], attn_weights f32 [sum N].  The outputs of the other mode must be NULL.  trunk
 * (NULL allowed, for tests): t of graph g as [max(S,1)][N_g][D] starting at node_off[g] * max(S,1) * D.  n = 0 launches nothing.
 * lmx_h_gnn_forward is the same network in plain C++ on HOST pointers with the same keep bits: f32, sequential sums. */
#define LMX_GNN_MAX_LAYERS 4
#define LMX_GNN_MAX_NODES 95
#define LMX_GNN_MAX_EDGES 663
#define LMX_GNN_LAP_K 8
#define LMX_GNN_RW_K 16
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim, reserved;
                 const float *in_w, *in_b, *lap1_w, *lap1_b, *lap2_w, *lap2_b, *lap_g, *lap_beta, *rw1_w, *rw1_b, *rw2_w, *rw2_b, *rw_g, *rw_beta;
                 const float *ee1_w, *ee1_b, *ee2_w, *ee2_b, *ee_g, *ee_beta;
                 const float *ln1_g[LMX_GNN_MAX_LAYERS], *ln1_b[LMX_GNN_MAX_LAYERS], *abde_w[LMX_GNN_MAX_LAYERS], *abde_b[LMX_GNN_MAX_LAYERS];
                 const float *c_w[LMX_GNN_MAX_LAYERS], *c_b[LMX_GNN_MAX_LAYERS], *eu1_w[LMX_GNN_MAX_LAYERS], *eu1_b[LMX_GNN_MAX_LAYERS];
                 const float *eu2_w[LMX_GNN_MAX_LAYERS], *eu2_b[LMX_GNN_MAX_LAYERS], *bne_g[LMX_GNN_MAX_LAYERS], *bne_b[LMX_GNN_MAX_LAYERS];
                 const float *bne_mean[LMX_GNN_MAX_LAYERS], *bne_var[LMX_GNN_MAX_LAYERS], *bnn_g[LMX_GNN_MAX_LAYERS], *bnn_b[LMX_GNN_MAX_LAYERS];
                 const float *bnn_mean[LMX_GNN_MAX_LAYERS], *bnn_var[LMX_GNN_MAX_LAYERS], *ln2_g[LMX_GNN_MAX_LAYERS], *ln2_b[LMX_GNN_MAX_LAYERS];
                 const float *qkv_w[LMX_GNN_MAX_LAYERS], *qkv_b[LMX_GNN_MAX_LAYERS], *out_w[LMX_GNN_MAX_LAYERS], *out_b[LMX_GNN_MAX_LAYERS];
                 const float *lna_g[LMX_GNN_MAX_LAYERS], *lna_b[LMX_GNN_MAX_LAYERS], *ln3_g[LMX_GNN_MAX_LAYERS], *ln3_b[LMX_GNN_MAX_LAYERS];
                 const float *ff1_w[LMX_GNN_MAX_LAYERS], *ff1_b[LMX_GNN_MAX_LAYERS], *ff2_w[LMX_GNN_MAX_LAYERS], *ff2_b[LMX_GNN_MAX_LAYERS];
                 const float *lnf_g, *lnf_b, *nh1_w, *nh1_b, *nh2_w, *nh2_b, *na1_w, *na1_b, *na2_w, *na2_b;
                 const float *cl1_w, *cl1_b, *cl2_w, *cl2_b, *cl3_w, *cl3_b; } lmx_gnn_weights_t;
typedef struct { int32_t n, reserved; const int32_t *node_off_host, *edge_off_host; const float *x, *lap, *rw; const int32_t *edge_src, *edge_dst;
                 const float* edge_attr; const int32_t *csr_ptr, *csr_edge, *deg; } lmx_gnn_graphs_t;
int lmx_h_gnn_graph(const float* emb_host /* [N][E] */, const double* timestamps_host /* NULL or [N] */, int N, int E, int k,
                    int32_t* edges_host /* [cap][2] */, float* edge_attr_host /* [cap][3] */, int32_t* n_edges_host,
                    int32_t* csr_ptr_host /* [N + 1] */, int32_t* csr_edge_host /* [cap] */, int32_t* deg_host /* [N] */,
                    float* lap_host /* [N][8] */, float* rw_host /* [N][16] */);
/* the eigendecomposition behind lap, in double: eigenvalues ascending (ties by the lower original column), column c of eigenvectors
 * [N][N] belongs to eigenvalue c; lap[i][c] = (float)|eigenvectors[i][c + 1]| */
int lmx_h_gnn_laplacian(const int32_t* edges_host /* [E][2] */, int n_edges, int N, double* eigenvalues_host /* [N] */,
                        double* eigenvectors_host /* [N][N] */);
int64_t lmx_gnn_workspace_bytes(int n, int S, int max_nodes, int max_edges, int d_model, int n_layers);
int lmx_k_gnn_forward(const lmx_gnn_weights_t* w_host, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host /* [n] */, int S,
                      double p, float* node_mc /* [sum N][S], S > 0 */, float* stats /* [sum N][2], S > 0 */, float* graph_pred /* [n], S == 0 */,
                      float* node_pred /* [sum N], S == 0 */, float* attn_weights /* [sum N], S == 0 */,
                      float* trunk /* NULL or [sum N][max(S,1)][D] */, void* workspace, lmx_stream_t stream);
int lmx_h_gnn_forward(const lmx_gnn_weights_t* w_host, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, double p,
                      float* node_mc_host, float* stats_host, float* graph_pred_host, float* node_pred_host, float* attn_weights_host,
                      float* trunk_host);

/* ==== MODEL level: GraphGPS scores from prepared graphs (csrc/graph_model.hip, csrc/gnn_image.h, csrc/host_gnn_image.cpp) ===============
 * services/gnn-pipeline/app/main.py's model behind a handle: the weights come from a WEIGHT IMAGE (kind 7) that
 * lmx.native.write_gnn_image writes (csrc/gnn_image.h has the config block and the tensors; the last live layer's edge update is not in
 * it); handle rules as for lmx_tcn.  The handle owns the workspace: lmx_gnn_workspace_bytes(max_graphs, max_samples, min(95,
 * max_nodes_total), min(663, max_edges_total), D, L), i.e. up to 485,376 bytes per (graph, sample) for the shipped network — 310 MB for
 * 64 graphs x 10 samples; open with the limits the caller will really use.  lmx_gnn_score: the graphs as for lmx_k_gnn_forward (DEVICE
 * arrays, the two offset arrays on the host), seeds_host on the host -> with S > 0 node_mc and stats, with S == 0 graph_pred, node_pred
 * and attn_weights, on the device (the outputs of the other mode NULL): lmx_k_gnn_forward with the image's dropout probability; it only
 * enqueues on `stream`.  n <= max_graphs, sum N <= max_nodes_total, sum E <= max_edges_total, S <= max_samples.  lmx_gnn_score_host takes
 * the graphs' arrays and returns the outputs in HOST memory, and synchronises (examples/gnn_score.c). */
typedef struct lmx_gnn lmx_gnn;
typedef struct { int32_t input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim, max_nodes, max_edges, max_graphs, max_nodes_total,
                 max_edges_total, max_samples, reserved; double p; } lmx_gnn_info_t;
int lmx_gnn_image_check_host(const char* path_host, lmx_gnn_info_t* info_host);
int lmx_gnn_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, lmx_gnn** out_host);
void lmx_gnn_close(lmx_gnn* m);
int lmx_gnn_info(const lmx_gnn* m, lmx_gnn_info_t* info_host);
int lmx_gnn_score(lmx_gnn* m, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* node_mc, float* stats,
                  float* graph_pred, float* node_pred, float* attn_weights, lmx_stream_t stream);
int lmx_gnn_score_host(lmx_gnn* m, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* node_mc_host,
                       float* stats_host, float* graph_pred_host, float* node_pred_host, float* attn_weights_host);

/* ==== The weight tables of the TCN, the gait transformer, the graph transformer and GraphGPS (csrc/weights_table.h) =====================
 * Which tensors a configuration calls for, under which names, with which shapes, and which pointer of lmx_<model>_weights_t each one
 * fills: stated once per model in the library (lmx_<model>_tensor_rows, csrc/host_<model>.cpp), read by the image readers, by the
 * handles and, through these four, by lmx/kernels.py. */
#define LMX_MAX_TENSOR_ROWS 256   /* above the largest table any configuration in the lists can ask for (gfm: 14 + 17 * 8 + 26 = 176) */
typedef struct lmx_tensor_row {
  char    name[48];     /* NUL padded; the image directory's name width */
  int32_t rank;         /* 1 .. 4 */
  int32_t shape[4];     /* unused dimensions 0 */
  int32_t reserved;     /* 0 */
  int64_t pointer_at;   /* byte offset, inside the model's lmx_<model>_weights_t, of the const float* this tensor fills */
} lmx_tensor_row_t;
/* The tensors the configuration in *config_host calls for (its integers only; its pointers are not read), in the order of the
 * weight image and of pack_tensors.  The configuration is checked against the model's list first: LMX_EINVAL, the message opened
 * by `who` and naming the field, exactly as lmx_h_<model>_forward refuses it.  rows_host may be NULL with cap 0 to check and count
 * only; cap below the count is LMX_EINVAL naming cap and the count.  Host arithmetic, no GPU. */
int lmx_h_tcn_tensors(const char* who, const lmx_tcn_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host);
int lmx_h_xfm_tensors(const char* who, const lmx_xfm_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host);
int lmx_h_gfm_tensors(const char* who, const lmx_gfm_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host);
int lmx_h_gnn_tensors(const char* who, const lmx_gnn_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host);

/* ==== Vector store: cosine top-k over a gallery of unit rows in HBM (csrc/vstore.hip, csrc/host_vstore.cpp, csrc/vstore_model.hip) =======
 * The one piece of arithmetic dinov3-pipeline (search_similar) and tracking-service (reid/matcher.py) go to Qdrant for.
 *
 * lmx_k_cosine_topk: gallery f32 unit rows [N][D] with a row stride of ldg elements (a store with spare capacity is a view), queries f32
 * unit rows [Q][D], dense.  Query q sees the slots [0, limits[q]) (clamped to [0, N]), or [0, N) when limits is NULL: a backlog of B new
 * rows is searched in ONE launch with the results of B search-then-append steps by giving query j the limit old_count + j.  For every
 * query: the k best visible rows in descending score, scores compared as float values, exact ties to the LOWER slot first; ranks past
 * the number of visible rows get slot -1 and score 0.  The order of (score, slot) pairs is total and a score is the PINNED DOT PRODUCT
 * below, so a result is a function of the inputs alone: it depends on no launch geometry, on no other query of the batch and on no
 * other row of the gallery, and there are no atomics.  A NaN score never ranks.
 *
 * THE PINNED DOT PRODUCT of a gallery row g and a query q, both of D elements:
 *   256 partials p[0 .. 255], each +0 at the start;
 *   partial j takes the elements j, j + 256, j + 512, ... in ascending order: p[j] = fmaf(g[i], q[i], p[j]); elements past D contribute
 *   nothing (partials past D stay +0);
 *   the partials are combined by halving: for w = 128, 64, ..., 1: p[j] = p[j] + p[j + w] for every j < w, each a single f32 add;
 *   the score is p[0].
 * (On the device: one wave per row, one 16-byte load per lane per 256 elements, lane l holds the partials 4 l .. 4 l + 3; the steps
 * w >= 4 are xor-butterflies across lanes, the last two are inside the lane.)  At most ceil(D / 256) + 8 roundings lie on the longest
 * path, each relative to at most sum |g[i] q[i]| <= 1: |score - exact| <= (ceil(D / 256) + 8) * 2^-24 for unit rows.
 *
 * Limits, refused with LMX_EINVAL and a message before anything is read, written or launched: D % 4 == 0 and 4 <= D <= 4096; 1 <= k <=
 * 32; 0 <= N <= 2^31 - 1; 0 <= Q <= 65535; ldg >= D and ldg % 4 == 0; gallery and queries 16-byte aligned.  Row offsets are 64-bit.
 * `workspace`: lmx_h_cosine_topk_workspace(N, Q, k) bytes, 8-byte aligned; it needs no clearing.  The call only enqueues on `stream`
 * (two kernels).  lmx_h_cosine_topk_geometry: the scan's rows per workgroup pass, its query tile at dimension D (8 up to D = 1024, 4 up
 * to 2048, 2 above) and its workgroups per CU, for tests that must reach every branch; none of them can show in a result.
 * lmx_h_cosine_topk is the same arithmetic in plain C++ on HOST pointers (no alignment asked); the device is held to it bit for bit.
 *
 * lmx_k_unit_rows / lmx_h_unit_rows: raw rows [n][D] (dense; dtype LMX_VSTORE_F32 or LMX_VSTORE_F64) -> f32 unit rows with a row
 * stride of ldo elements.  The sum of squares ss is taken in double in the same 256-partial order with fma; element i becomes
 * (float)((double)x[i] / (sqrt(ss) + 1e-8)) — the epsilon and its place are those of reid/matcher.py and csrc/graph.h.  A zero row
 * gives zeros.  Same limits on D. */
#define LMX_VSTORE_F32 1
#define LMX_VSTORE_F64 2
int64_t lmx_h_cosine_topk_workspace(int64_t N, int Q, int k);
int lmx_h_cosine_topk_geometry(int D, int* rows_host, int* tile_host, int* wg_per_cu_host);
int lmx_k_cosine_topk(const float* gallery /* [N][ldg] */, int64_t N, int D, int64_t ldg, const float* queries /* [Q][D] */, int Q,
                      const int32_t* limits /* NULL or [Q] */, int k, float* scores /* [Q][k] */, int32_t* slots /* [Q][k] */, void* workspace,
                      lmx_stream_t stream);
int lmx_h_cosine_topk(const float* gallery_host, int64_t N, int D, int64_t ldg, const float* queries_host, int Q, const int32_t* limits_host,
                      int k, float* scores_host, int32_t* slots_host);
int lmx_k_unit_rows(const void* raw /* [n][D] */, int dtype, int64_t n, int D, float* out /* [n][ldo] */, int64_t ldo, lmx_stream_t stream);
int lmx_h_unit_rows(const void* raw_host, int dtype, int64_t n, int D, float* out_host, int64_t ldo);

/* lmx_vstore: a growing gallery of unit rows in HBM behind a handle.  It maps nothing but SLOTS (row numbers 0 .. count - 1); ids and
 * payloads belong to the caller.  lmx_vstore_open takes the current device; every later call must be made with that device current
 * and a stream of that device (LMX_EINVAL otherwise, nothing launched).  lmx_vstore_put_host: one raw row from HOST memory, normalised
 * by lmx_h_unit_rows; slot == count appends, a lower slot replaces in place, any other slot is refused.  lmx_vstore_append: n raw rows
 * already on the DEVICE, normalised by lmx_k_unit_rows (the same bits).  The gallery grows by doubling; put_host, append and get_host
 * are SYNCHRONOUS (they return with the row in place, and wait for the device's earlier work first).  lmx_vstore_get_host: the stored
 * unit row; lmx_vstore_read_host: n of them from slot `first`; lmx_vstore_restore_host appends n rows that ARE unit rows as they stand,
 * byte for byte (what read_host returned: a saved store comes back with the bits it had).  lmx_vstore_gallery: the rows as lmx_k_cosine_topk takes them; the pointer holds until the next put_host or append.
 * lmx_vstore_search: raw queries [Q][dim] on the DEVICE are normalised and searched over the stored rows with lmx_k_cosine_topk; it
 * enqueues on `stream`, except that the first search at a larger Q x k grows the handle's scratch synchronously.  limits as for
 * lmx_k_cosine_topk (DEVICE memory, or NULL).  lmx_vstore_search_host takes the queries and limits from, and returns scores and slots
 * in, HOST memory, on the handle's own stream, and synchronises (examples/vstore_search.c). */
typedef struct lmx_vstore lmx_vstore;
int lmx_vstore_open(int dim, int64_t capacity, lmx_vstore** out_host);
void lmx_vstore_close(lmx_vstore* m);
int64_t lmx_vstore_count(const lmx_vstore* m);
int lmx_vstore_gallery(const lmx_vstore* m, const float** gallery, int64_t* ldg_host);
int lmx_vstore_put_host(lmx_vstore* m, int64_t slot, const void* raw_host, int dtype);
int lmx_vstore_append(lmx_vstore* m, const void* raw_rows, int dtype, int64_t n);
int lmx_vstore_get_host(lmx_vstore* m, int64_t slot, float* out_host);
int lmx_vstore_read_host(lmx_vstore* m, int64_t first, int64_t n, float* out_host);
int lmx_vstore_restore_host(lmx_vstore* m, const float* unit_rows_host, int64_t n);
int lmx_vstore_search(lmx_vstore* m, const void* raw_queries, int dtype, int Q, const int32_t* limits, int k, float* scores, int32_t* slots,
                      lmx_stream_t stream);
int lmx_vstore_search_host(lmx_vstore* m, const void* raw_queries_host, int dtype, int Q, const int32_t* limits_host, int k, float* scores_host,
                           int32_t* slots_host);

#ifdef __cplusplus
}
#endif
#endif
