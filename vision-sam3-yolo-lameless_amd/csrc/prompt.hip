// prompt.hip — the prompt paths of SamPredictor.predict beyond the box: click points, a mask input fed back as the dense
// prompt, all four masks of the decoder, and the un-thresholded postprocess (segment_anything PromptEncoder / MaskDecoder /
// Sam.postprocess_masks; TF:models/sam/modeling_sam.py:596-698, :432-543).
//
// Compiled with -ffp-contract=off (csrc/Makefile EXACT) like sam.hip and exact.hip: the box tokens of prompt_points, the
// slices of hyper_mask_multi[_f32] and the threshold of mask_logits are bit-identical to lmx_k_prompt_box, lmx_k_hyper_mask[_f32]
// and lmx_k_mask_post because each thread runs the same sequence of f32 operations as the kernel it generalises.
#include "common.h"

namespace {

inline int grid_for(int64_t total, int block = 256) {
  int64_t g = (total + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

// thread = (frame, token, j): the sin / cos pair j of one sparse token.  Tokens are [points..., box corners] with a box and
// [points..., pad] without one; label -1 (and the pad) is not_a_point_embed alone, 0 / 1 add point_embed[0 / 1] to the PE.
__global__ __launch_bounds__(256) void prompt_points_kernel(const float* __restrict__ points, const int32_t* __restrict__ labels, int Np,
                                                            const float* __restrict__ boxes, int64_t ldb, float* __restrict__ sparse,
                                                            int n, double sx, double sy, float S, const float* __restrict__ gauss,
                                                            const float* __restrict__ pembed, const float* __restrict__ nap,
                                                            const float* __restrict__ corner, int F) {
  const int Ns = Np + (boxes ? 2 : 1);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * Ns * F) return;
  const int j = (int)(i % F);
  const int64_t bt = i / F;
  const int t = (int)(bt % Ns), b = (int)(bt / Ns);
  float* o = sparse + bt * 2 * F;
  const float* add;
  float px, py;
  if (t < Np) {
    const int l = labels[(int64_t)b * Np + t];
    if (l == -1) {
      o[j] = nap[j];
      o[F + j] = nap[F + j];
      return;
    }
    if (l != 0 && l != 1) {  // not a label segment_anything knows: poison the token (the host checks labels before the launch)
      o[j] = __builtin_nanf("");
      o[F + j] = __builtin_nanf("");
      return;
    }
    const float* p = points + ((int64_t)b * Np + t) * 2;
    // apply_coords in double, then the f32 tensor; + 0.5 (pixel centre) as _embed_points
    px = (float)((double)p[0] * sx) + 0.5f;
    py = (float)((double)p[1] * sy) + 0.5f;
    add = pembed + l * 2 * F;
  } else if (boxes) {
    const int k = t - Np;
    const float* bx = boxes + (int64_t)b * ldb + 2 * k;
    px = (float)((double)bx[0] * sx) + 0.5f;
    py = (float)((double)bx[1] * sy) + 0.5f;
    add = corner + k * 2 * F;
  } else {
    o[j] = nap[j];
    o[F + j] = nap[F + j];
    return;
  }
  const float cx = 2.f * (px / S) - 1.f, cy = 2.f * (py / S) - 1.f;
  const float ang = 6.283185307179586f * (cx * gauss[j] + cy * gauss[F + j]);
  o[j] = sinf(ang) + add[j];
  o[F + j] = cosf(ang) + add[F + j];
}

// SamMaskEmbedding + the dense add: workgroup = MPIX output pixels of the GxG grid.  Each pixel reads the 4x4 patch of the
// mask under it; conv1 (k2 s2, 1 -> 4) per 2x2 sub-pixel, LayerNorm2d, GELU; conv2 (k2 s2, 4 -> 16), LayerNorm2d, GELU build
// the 16-vector in LDS; then thread k produces channel k of conv3 (1x1, 16 -> 256) for every pixel of the group and stores
// emb + dense (one 1 KB row per pixel, coalesced).  Plain f32, every sum in the order written.
constexpr int MPIX = 16;
constexpr int ME_W1 = 0, ME_B1 = 16, ME_G1 = 20, ME_BE1 = 24, ME_W2 = 28, ME_B2 = 284, ME_G2 = 300, ME_BE2 = 316, ME_W3 = 332,
              ME_B3 = 332 + 256 * 16, ME_COUNT = ME_B3 + 256;
static_assert(ME_COUNT == LMX_MASK_EMBED_PARAMS, "lmx.h parameter layout");

__device__ __forceinline__ float gelu_erf(float v) { return act_exact(v, LMX_ACT_GELU); }

template <int EMB_DT>
__global__ __launch_bounds__(256) void mask_embed_kernel(const float* __restrict__ mask, const void* __restrict__ emb, int64_t lde,
                                                         const float* __restrict__ prm, float* __restrict__ keys, int64_t ldk, int n,
                                                         int G) {
  __shared__ float ms[MPIX][16];     // the 4x4 mask patch of each pixel, row-major
  __shared__ float a1[MPIX][4][4];   // [pixel][sub-pixel dy*2+dx][channel] after LayerNorm2d + GELU
  __shared__ float h2[MPIX][16];     // conv2 output
  __shared__ float a2[MPIX][16];     // after LayerNorm2d + GELU
  const float eps = 1e-6f;
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)n * G * G;
  const int64_t pix0 = (int64_t)blockIdx.x * MPIX;
  const int S = 4 * G;
  {
    const int p = tid >> 4, e = tid & 15;
    const int64_t g = pix0 + p;
    float v = 0.f;
    if (g < total) {
      const int X = (int)(g % G);
      const int64_t r = g / G;
      const int Y = (int)(r % G), b = (int)(r / G);
      v = mask[((int64_t)b * S + 4 * Y + (e >> 2)) * S + 4 * X + (e & 3)];
    }
    ms[p][e] = v;
  }
  __syncthreads();
  if (tid < MPIX * 4) {
    const int p = tid >> 2, s = tid & 3;
    const int dy = s >> 1, dx = s & 1;
    float h[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float acc = prm[ME_B1 + c];
#pragma unroll
      for (int ey = 0; ey < 2; ++ey)
#pragma unroll
        for (int ex = 0; ex < 2; ++ex) acc = acc + prm[ME_W1 + c * 4 + ey * 2 + ex] * ms[p][(2 * dy + ey) * 4 + 2 * dx + ex];
      h[c] = acc;
    }
    const float mean = (((h[0] + h[1]) + h[2]) + h[3]) * 0.25f;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) var = var + (h[c] - mean) * (h[c] - mean);
    const float rstd = 1.0f / sqrtf(var * 0.25f + eps);
#pragma unroll
    for (int c = 0; c < 4; ++c) a1[p][s][c] = gelu_erf((h[c] - mean) * rstd * prm[ME_G1 + c] + prm[ME_BE1 + c]);
  }
  __syncthreads();
  {
    const int p = tid >> 4, o = tid & 15;
    float acc = prm[ME_B2 + o];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = acc + prm[ME_W2 + (o * 4 + c) * 4 + s] * a1[p][s][c];
    h2[p][o] = acc;
  }
  __syncthreads();
  {
    const int p = tid >> 4, o = tid & 15;
    float mean = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) mean = mean + h2[p][c];
    mean = mean * 0.0625f;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) var = var + (h2[p][c] - mean) * (h2[p][c] - mean);
    const float rstd = 1.0f / sqrtf(var * 0.0625f + eps);
    a2[p][o] = gelu_erf((h2[p][o] - mean) * rstd * prm[ME_G2 + o] + prm[ME_BE2 + o]);
  }
  __syncthreads();
  const int k = tid;
  float w3[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) w3[c] = prm[ME_W3 + k * 16 + c];
  const float b3 = prm[ME_B3 + k];
  for (int p = 0; p < MPIX; ++p) {
    const int64_t g = pix0 + p;
    if (g >= total) break;
    float acc = b3;
#pragma unroll
    for (int c = 0; c < 16; ++c) acc = acc + w3[c] * a2[p][c];
    float e;
    if (EMB_DT == LMX_F32)
      e = reinterpret_cast<const float*>(emb)[g * lde + k];
    else
      e = (float)reinterpret_cast<const half_t*>(emb)[g * lde + k];
    keys[g * ldk + k] = e + acc;
  }
}

// lmx_k_hyper_mask for M masks at once: the thread loads its sub-pixel's `up` vector once and keeps M accumulators, each fed
// the same fmaf sequence as hyper_mask_kernel (slice m == lmx_k_hyper_mask with hyper[:, m], bit for bit).
template <int M>
__global__ __launch_bounds__(256) void hyper_mask_multi_kernel(const half_t* __restrict__ up, const float* __restrict__ hyper,
                                                               float* __restrict__ logits, int n, int G, int C) {
  const int64_t total = (int64_t)n * G * G * 16;
  const int S = 4 * G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q2 = (int)(i & 3), q1 = (int)((i >> 2) & 3);
    const int64_t cell = i >> 4;
    const int x = (int)(cell % G);
    const int64_t r = cell / G;
    const int y = (int)(r % G);
    const int b = (int)(r / G);
    const half_t* u = up + i * C;
    const float* hy = hyper + (int64_t)b * M * C;
    float acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0.f;
    for (int c = 0; c < C; c += 8) {
      const half8_t v = *reinterpret_cast<const half8_t*>(u + c);
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = fmaf((float)v[e], hy[m * C + c + e], acc[m]);
    }
    const int Y = 4 * y + 2 * (q1 >> 1) + (q2 >> 1), X = 4 * x + 2 * (q1 & 1) + (q2 & 1);
#pragma unroll
    for (int m = 0; m < M; ++m) logits[(((int64_t)b * M + m) * S + Y) * S + X] = acc[m];
  }
}

// lmx_k_hyper_mask_f32 for M masks at once (same per-mask sequence: acc += act(v) * hy, no contraction).
template <int M>
__global__ __launch_bounds__(256) void hyper_mask_multi_f32_kernel(const float* __restrict__ up, const float* __restrict__ hyper,
                                                                   float* __restrict__ logits, int n, int G, int C, int act) {
  const int64_t total = (int64_t)n * G * G * 16;
  const int S = 4 * G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q2 = (int)(i & 3), q1 = (int)((i >> 2) & 3);
    const int64_t cell = i >> 4;
    const int x = (int)(cell % G);
    const int64_t r = cell / G;
    const int y = (int)(r % G);
    const int b = (int)(r / G);
    const float* u = up + i * C;
    const float* hy = hyper + (int64_t)b * M * C;
    float acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0.f;
    for (int c = 0; c < C; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(u + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = act_exact(v[e], act);
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] += a * hy[m * C + c + e];
      }
    }
    const int Y = 4 * y + 2 * (q1 >> 1) + (q2 >> 1), X = 4 * x + 2 * (q1 & 1) + (q2 & 1);
#pragma unroll
    for (int m = 0; m < M; ++m) logits[(((int64_t)b * M + m) * S + Y) * S + X] = acc[m];
  }
}

// Sam.postprocess_masks without the threshold, in one pass: each output pixel takes its four taps of the cropped TxT
// intermediate through sample_mid (the value mask_mid_kernel stores) and blends them as mask_post_kernel does, so
// (out > 0) is mask_post's mask bit for bit.  Thread = 4 consecutive pixels of one row.
__global__ __launch_bounds__(256) void mask_logits_kernel(const float* __restrict__ logits, int L, int T, int nh, int nw, int h, int w,
                                                          float* __restrict__ out) {
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * L * L;
  const float sLT = (float)L / (float)T;
  const float sy = (float)nh / (float)h, sx = (float)nw / (float)w;
  const int wq = (w + 3) / 4;
  const int total = h * wq;  // < 2^31 (checked by the launcher)
  float* ob = out + (int64_t)b * h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / wq, xq = (i - y * wq) * 4;
    int Y0, Y1;
    float ly;
    bil_idx(sy, y, nh, Y0, Y1, ly);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = xq + e;
      if (x >= w) break;
      int X0, X1;
      float lx;
      bil_idx(sx, x, nw, X0, X1, lx);
      const float a00 = sample_mid(lg, L, T, sLT, Y0, X0), a01 = sample_mid(lg, L, T, sLT, Y0, X1);
      const float a10 = sample_mid(lg, L, T, sLT, Y1, X0), a11 = sample_mid(lg, L, T, sLT, Y1, X1);
      const float t0 = (1.f - lx) * a00 + lx * a01;
      const float t1 = (1.f - lx) * a10 + lx * a11;
      r[e] = (1.f - ly) * t0 + ly * t1;
    }
    if ((w & 3) == 0) {
      *reinterpret_cast<f32x4*>(ob + (int64_t)y * w + xq) = r;
    } else {
      for (int e = 0; e < 4 && xq + e < w; ++e) ob[(int64_t)y * w + xq + e] = r[e];
    }
  }
}

}  // namespace

extern "C" int lmx_k_prompt_points(const float* points, const int32_t* labels, int Np, const float* boxes, int64_t ldb, float* sparse,
                                   int n, double sx, double sy, float S, const float* gauss, const float* point_embed,
                                   const float* not_a_point, const float* corner, int F, lmx_stream_t stream) {
  LMX_REQUIRE(sparse && gauss && point_embed && not_a_point && corner, "lmx_k_prompt_points: null pointer");
  LMX_REQUIRE(n > 0 && F > 0 && Np >= 0 && S > 0.f, "lmx_k_prompt_points: n=%d Np=%d F=%d", n, Np, F);
  LMX_REQUIRE(Np > 0 || boxes, "lmx_k_prompt_points: no prompt (no points and no box)");
  LMX_REQUIRE(Np == 0 || (points && labels), "lmx_k_prompt_points: points / labels missing");
  LMX_REQUIRE(!boxes || ldb >= 4, "lmx_k_prompt_points: box stride %lld", (long long)ldb);
  const int64_t items = (int64_t)n * (Np + (boxes ? 2 : 1)) * F;
  LMX_REQUIRE(items < (1ll << 31) - 256, "lmx_k_prompt_points: too many tokens");
  hipLaunchKernelGGL(prompt_points_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), points,
                     labels, Np, boxes, ldb, sparse, n, sx, sy, S, gauss, point_embed, not_a_point, corner, F);
  return lmx_launch_check("prompt_points_kernel");
}

extern "C" int lmx_k_mask_embed(const float* mask_input, const void* emb, int emb_dtype, int64_t lde, const float* params, float* keys,
                                int64_t ldk, int n, int G, lmx_stream_t stream) {
  LMX_REQUIRE(mask_input && emb && params && keys, "lmx_k_mask_embed: null pointer");
  LMX_REQUIRE(n > 0 && G > 0 && lde >= 256 && ldk >= 256, "lmx_k_mask_embed: n=%d G=%d lde=%lld ldk=%lld", n, G, (long long)lde,
              (long long)ldk);
  const int64_t pix = (int64_t)n * G * G;
  LMX_REQUIRE((pix + MPIX - 1) / MPIX < (1ll << 31), "lmx_k_mask_embed: grid too large");
  const dim3 grid((unsigned)((pix + MPIX - 1) / MPIX));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (emb_dtype == LMX_F32)
    hipLaunchKernelGGL(mask_embed_kernel<LMX_F32>, grid, dim3(256), 0, st, mask_input, emb, lde, params, keys, ldk, n, G);
  else if (emb_dtype == LMX_F16)
    hipLaunchKernelGGL(mask_embed_kernel<LMX_F16>, grid, dim3(256), 0, st, mask_input, emb, lde, params, keys, ldk, n, G);
  else
    LMX_REQUIRE(false, "lmx_k_mask_embed: embedding dtype %d", emb_dtype);
  return lmx_launch_check("mask_embed_kernel");
}

extern "C" int lmx_k_hyper_mask_multi(const void* up, const float* hyper, float* logits, int n, int M, int G, int C, lmx_stream_t stream) {
  LMX_REQUIRE(up && hyper && logits, "lmx_k_hyper_mask_multi: null pointer");
  LMX_REQUIRE(n > 0 && G > 0 && C > 0 && C % 8 == 0 && C <= 64 && aligned16(up), "lmx_k_hyper_mask_multi: shape");
  LMX_REQUIRE(M >= 1 && M <= 4, "lmx_k_hyper_mask_multi: M=%d masks (1..4)", M);
  const dim3 grid(grid_for((int64_t)n * G * G * 16));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const half_t* u = reinterpret_cast<const half_t*>(up);
  if (M == 1) hipLaunchKernelGGL(hyper_mask_multi_kernel<1>, grid, dim3(256), 0, st, u, hyper, logits, n, G, C);
  if (M == 2) hipLaunchKernelGGL(hyper_mask_multi_kernel<2>, grid, dim3(256), 0, st, u, hyper, logits, n, G, C);
  if (M == 3) hipLaunchKernelGGL(hyper_mask_multi_kernel<3>, grid, dim3(256), 0, st, u, hyper, logits, n, G, C);
  if (M == 4) hipLaunchKernelGGL(hyper_mask_multi_kernel<4>, grid, dim3(256), 0, st, u, hyper, logits, n, G, C);
  return lmx_launch_check("hyper_mask_multi_kernel");
}

extern "C" int lmx_k_hyper_mask_multi_f32(const float* up, const float* hyper, float* logits, int n, int M, int G, int C, int act,
                                          lmx_stream_t stream) {
  LMX_REQUIRE(up && hyper && logits, "lmx_k_hyper_mask_multi_f32: null pointer");
  LMX_REQUIRE(n > 0 && G > 0 && C > 0 && C % 4 == 0 && aligned16(up), "lmx_k_hyper_mask_multi_f32: shape");
  LMX_REQUIRE(M >= 1 && M <= 4, "lmx_k_hyper_mask_multi_f32: M=%d masks (1..4)", M);
  LMX_REQUIRE(act == LMX_ACT_NONE || act == LMX_ACT_GELU, "lmx_k_hyper_mask_multi_f32: activation %d", act);
  const dim3 grid(grid_for((int64_t)n * G * G * 16));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M == 1) hipLaunchKernelGGL(hyper_mask_multi_f32_kernel<1>, grid, dim3(256), 0, st, up, hyper, logits, n, G, C, act);
  if (M == 2) hipLaunchKernelGGL(hyper_mask_multi_f32_kernel<2>, grid, dim3(256), 0, st, up, hyper, logits, n, G, C, act);
  if (M == 3) hipLaunchKernelGGL(hyper_mask_multi_f32_kernel<3>, grid, dim3(256), 0, st, up, hyper, logits, n, G, C, act);
  if (M == 4) hipLaunchKernelGGL(hyper_mask_multi_f32_kernel<4>, grid, dim3(256), 0, st, up, hyper, logits, n, G, C, act);
  return lmx_launch_check("hyper_mask_multi_f32_kernel");
}

extern "C" int lmx_k_mask_logits(const float* logits, int n, int L, int T, int nh, int nw, int h, int w, float* out, lmx_stream_t stream) {
  LMX_REQUIRE(logits && out, "lmx_k_mask_logits: null pointer");
  LMX_REQUIRE(n > 0 && L > 0 && T >= L && nh > 0 && nw > 0 && nh <= T && nw <= T && h > 0 && w > 0 &&
                  (int64_t)h * ((w + 3) / 4) < 0x7fffffffll - 96 * 256 && n <= 65535, "lmx_k_mask_logits: geometry");
  LMX_REQUIRE(aligned16(out), "lmx_k_mask_logits: out alignment");
  int gx = (int)(((int64_t)h * ((w + 3) / 4) + 255) / 256);
  if (gx > 96) gx = 96;
  hipLaunchKernelGGL(mask_logits_kernel, dim3(gx, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), logits, L, T, nh, nw, h, w, out);
  return lmx_launch_check("mask_logits_kernel");
}
