// graph_tile.h — the device helpers that the two graph kernels (gfm.hip, gnn.hip) share: the workgroup's shape, the row stride of the LDS
// tiles, the wave-level fence, the keep decision of a dropout site, LayerNorm on a wave's 16 rows and the "one block of a sum, four
// column tiles at a time" wrapper around the model's own mma.  What differs stays in the kernels: the two mma bodies (gfm chains its
// MFMAs, gnn restarts each and joins through TwoSum) and the two attentions.  DEVICE code in an anonymous namespace: every
// name is the including kernel file's own.
#pragma once
#include "common.h"
#include "gait.h"

namespace {

constexpr int NW = 8;             // waves of a workgroup
constexpr int NTH = NW * 64;
constexpr int LD = 132;           // floats per row of an LDS tile: rows 16-byte aligned, 16 rows of a float4 column in 16 different slots
constexpr int LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ void wave_fence() {
  // orders this wave's LDS stores before its later LDS loads of other lanes' words (the hardware keeps a wave's DS operations in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NC>
__device__ __forceinline__ void zero(f32x4 (&acc)[NC]) {
#pragma unroll
  for (int ni = 0; ni < NC; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// racc[0 .. ncols) += one block of a sum over blocks (a head's share of out_proj, an FFN chunk's share of fc2): the column tiles
// n0 .. n0 + ncols - 1 (ncols <= 8) of W with NT column tiles, four at a time, each with chains of its own that start at zero, which
// keeps the registers of a second set of eight accumulators free.  MMA is the model's mma over four column tiles.
template <auto MMA>
__device__ __forceinline__ void mma_cols(f32x4 (&racc)[8], const float* src, int ld, const float* __restrict__ W, int q0, int nq, int NT, int n0,
                                         int ncols, int m, int lane) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int nn = ncols - 4 * half < 4 ? ncols - 4 * half : 4;
    if (nn > 0) {
      f32x4 block[4];
      zero<4>(block);
      MMA(block, src, ld, W, q0, nq, NT, n0 + 4 * half, nn, m, lane);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) racc[4 * half + ni] += block[ni];
    }
  }
}

struct Keep {
  bool on;
  uint64_t seed, stream0, thr;
  float scale;
  __device__ __forceinline__ float operator()(float v, int site, uint64_t u) const {
    if (!on) return v;
    return lmx_gait_keep(seed, stream0 + (uint64_t)site, u, thr) ? v * scale : 0.f;
  }
};

// dst = LN(src) on the 16 rows of tile m (dst may be src): one row per 16-lane group, two passes.  The node rows are R0 .. R0 + N - 1
// (gfm keeps the virtual node in row 0: R0 = 1).  site >= 0: the node rows are dropped at that site with u = (t - R0) * D + c.  `out`
// (global, may be null) receives the node rows as [N][D].
template <int R0>
__device__ __forceinline__ void layer_norm(const float* src, float* dst, const float* __restrict__ gam, const float* __restrict__ bet, int D, int N,
                                           int m, int lane, const Keep& keep, int site, float* out) {
  const int r = lane & 15, g = lane >> 4;
  float gg[8], bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = r + 16 * j;
    gg[j] = c < D ? gam[c] : 0.f;
    bb[j] = c < D ? bet[c] : 0.f;
  }
  const float inv = (float)D;
  for (int rr = 0; rr < 4; ++rr) {
    const int t = m * 16 + 4 * rr + g;
    float v[8], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = r + 16 * j < D ? src[t * LD + r + 16 * j] : 0.f;
      sum += v[j];
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum / inv;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (r + 16 * j < D) ss += (v[j] - mean) * (v[j] - mean);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);
    const float rstd = 1.0f / sqrtf(ss / inv + 1e-5f);
    const bool node = t >= R0 && t < N + R0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = r + 16 * j;
      if (c < D) {
        float y = (v[j] - mean) * rstd * gg[j] + bb[j];
        if (site >= 0 && node) y = keep(y, site, (uint64_t)((t - R0) * D + c));
        dst[t * LD + c] = y;
        if (out && node) out[(size_t)(t - R0) * D + c] = y;
      }
    }
  }
}

}  // namespace
