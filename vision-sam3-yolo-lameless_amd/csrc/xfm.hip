// xfm.hip — the whole gait transformer in one launch (include/lmx.h "The gait transformer").
// One workgroup per (clip, sample): NW = 8 waves up to 128 steps, 4 waves beyond.  Three tiles live in LDS (TP = T rounded up to 16):
// the residual stream h [TP][68], the LayerNorm output a [TP][68] and a work tile U [TP][LDU], LDU = max(3 dh, 64) + 4, which holds
// q_i | k_i | v_i of the CURRENT head and then 64 columns of the FFN's hidden layer at a time.  Every matrix product runs on the exact f32-input MFMA v_mfma_f32_16x16x4_f32
// with the operand order of tcn.hip: wave w owns the 16-row tiles w, w + NW, ... (MPW of them, a template parameter), reads ONE float4
// of A per 16 inputs from LDS and one float4 of B per column tile straight from the packed weights in L2, one step ahead of the MFMAs.
// Rows are wave-private everywhere except K and V of a head, which every wave reads.
//   attention, per head and 16 query rows: the TP / 16 score accumulators stay in registers; row maximum and sum go over the 16 lanes
//   that share a row (__shfl_xor 1, 2, 4, 8); the keep bits are applied; each 16 x 16 block of P passes through a private LDS patch of the
//   wave to reach the A-operand layout for P.V; the head's output overwrites q_i's columns and out_proj accumulates over the heads in
//   registers.
//   FFN: 64 hidden columns at a time through U, fc2 accumulates over the chunks in registers.
// Rows t >= T: h starts as zeros there and stays finite, they are masked as keys (their score is -inf, so P is exactly 0 where V holds
// them), never pooled, and never leave the LDS.
#include "gait_launch.h"
#include "xfm.h"

namespace {

constexpr int LD = 68;            // floats per row of h and a
constexpr int PLD = 20;           // floats per row of a wave's 16 x 16 patch: 16-byte aligned rows, the four row groups in different banks
constexpr int PATCH = 16 * PLD;
constexpr int LDS_LIMIT = 160 * 1024;

struct XfmArgs {
  lmx_xfm_weights_t w;
  const float* x;
  const uint8_t* mask;
  const uint64_t* seeds;
  float *pred, *saliency, *trunk;
  int T, S, MT, LDU;
  uint64_t thr;
  float scale, qs;
};

// h | a | U | one patch per wave | one saliency strip per wave | key mask | pooled | one pool partial per wave | classifier's hidden row
__host__ __device__ constexpr int lds_floats(int NW, int TP, int LDU) {
  return 2 * TP * LD + TP * LDU + NW * PATCH + NW * TP + TP + 64 + NW * 64 + 64;
}

__device__ __forceinline__ void wave_fence() {
  // orders this wave's LDS stores before its later LDS loads of other lanes' words (the hardware keeps a wave's DS operations in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MPW>
__device__ __forceinline__ void zero(f32x4 (&acc)[MPW][4]) {
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[mi][ni] += rows of tile (wave + NW mi) of src[.][0 .. 16 nq) x the groups q0 .. q0 + nq - 1 and column tiles n0 .. n0 + nn - 1 of the
// packed linear layer W with NT column tiles.  The B operand of the NEXT group is loaded while the MFMAs of this one run.
template <int NW, int MPW>
__device__ __forceinline__ void mma(f32x4 (&acc)[MPW][4], const float* src, int ld, const float* __restrict__ W, int q0, int nq, int NT, int n0,
                                    int nn, int MT, int wave, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const f32x4* wp = reinterpret_cast<const f32x4*>(W) + ((size_t)q0 * NT + n0) * 64 + lane;
  const f32x4* const wlast = wp + (size_t)(nq - 1) * NT * 64;
  f32x4 b[4], bn[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) b[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < nq; ++q) {
    if (wp != wlast) wp += NT * 64;  // the last step loads its own operand again
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bn[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + NW * mi;
      if (m < MT) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + (m * 16 + r) * ld + 16 * q + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            if (ni < nn) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[ni][e], acc[mi][ni], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) b[ni] = bn[ni];
  }
}

// a = LN(h) on the wave's own rows: one row per 16-lane group, two passes; `out` (global, may be null) receives the rows t < T
template <int NW, int MPW>
__device__ __forceinline__ void layer_norm(const float* h, float* a, const float* __restrict__ gam, const float* __restrict__ bet, int D, int MT,
                                           int T, int wave, int lane, float* out) {
  const int r = lane & 15, g = lane >> 4;
  float gg[4], bb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = r + 16 * j;
    gg[j] = c < D ? gam[c] : 0.f;
    bb[j] = c < D ? bet[c] : 0.f;
  }
  const float inv = (float)D;
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    const int m = wave + NW * mi;
    if (m < MT) {
      for (int rr = 0; rr < 4; ++rr) {
        const int t = m * 16 + 4 * rr + g;
        float v[4], sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = r + 16 * j < D ? h[t * LD + r + 16 * j] : 0.f;
          sum += v[j];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
        const float mean = sum / inv;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (r + 16 * j < D) ss += (v[j] - mean) * (v[j] - mean);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);
        const float rstd = 1.0f / sqrtf(ss / inv + 1e-5f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = r + 16 * j;
          if (c < D) {
            const float y = (v[j] - mean) * rstd * gg[j] + bb[j];
            a[t * LD + c] = y;
            if (out && t < T) out[(size_t)t * D + c] = y;
          }
        }
      }
    }
  }
}

template <int NW, int MPW>
__global__ __launch_bounds__(NW * 64) void xfm_forward_kernel(const XfmArgs a) {
  constexpr int KT = NW * MPW < 10 ? NW * MPW : 10;  // key tiles an instantiation can hold in registers
  constexpr int NTH = NW * 64;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = a.T, MT = a.MT, TP = MT * 16, LDU = a.LDU;
  float* hb = lds;
  float* ab = hb + TP * LD;
  float* ub = ab + TP * LD;
  float* patch = ub + TP * LDU;
  float* salw = patch + NW * PATCH;
  int* mkl = reinterpret_cast<int*>(salw + NW * TP);
  float* pooled = salw + (NW + 1) * TP;
  float* part = pooled + 64;
  float* hid = part + NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Smax = a.S > 0 ? a.S : 1, clip = blockIdx.x / Smax, sample = blockIdx.x % Smax;
  const int F = a.w.input_dim, D = a.w.d_model, H = a.w.n_heads, dh = D / H, L = a.w.n_layers, FF = a.w.ff, NTD = D >> 4;
  const bool drop = a.S > 0;
  const uint64_t seed = drop ? a.seeds[clip] : 0, stream0 = (uint64_t)sample * (uint64_t)(4 * L + 2);
  float* mypatch = patch + wave * PATCH;
  float* mysal = salw + wave * TP;
  const float ninf = -__builtin_huge_valf();

  // masked keys (rows >= T count as masked), the saliency partial sums, and the series into tile a: zeros beyond T and beyond input_dim
  for (int u = tid; u < TP; u += NTH) {
    mkl[u] = (u >= T || (a.mask && a.mask[(size_t)clip * T + u])) ? 1 : 0;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) salw[wv * TP + u] = 0.f;
  }
  const float* x = a.x + (size_t)clip * T * F;
  for (int i = tid; i < TP * 64; i += NTH) {
    const int t = i >> 6, c = i & 63;
    ab[t * LD + c] = (t < T && c < F) ? x[t * F + c] : 0.f;
  }
  __syncthreads();

  f32x4 acc[MPW][4], racc[MPW][4];
  // h = drop_0( x W_in^T + b_in + pe[t] )
  zero<MPW>(acc);
  mma<NW, MPW>(acc, ab, LD, a.w.in_w, 0, (F + 15) >> 4, NTD, 0, NTD, MT, wave, lane);
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    const int m = wave + NW * mi;
    if (m < MT) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float bias = a.w.in_b[c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float v = 0.f;
            if (t < T) {
              v = acc[mi][ni][e] + bias + a.w.pe[t * D + c];
              if (drop) v = lmx_gait_keep(seed, stream0, (uint64_t)(t * D + c), a.thr) ? v * a.scale : 0.f;
            }
            hb[t * LD + c] = v;
          }
        }
    }
  }
  __syncthreads();

  for (int l = 0; l < L; ++l) {
    layer_norm<NW, MPW>(hb, ab, a.w.ln1_g[l], a.w.ln1_b[l], D, MT, T, wave, lane, nullptr);
    __syncthreads();
    const bool sal_here = a.saliency != nullptr && l == L - 1;
    const uint64_t site_p = stream0 + 1 + 4 * l;
    zero<MPW>(racc);  // out_proj, accumulated over the heads
    for (int hd = 0; hd < H; ++hd) {
      // q_i | k_i | v_i of this head into U (q scaled), 4 column tiles at a time
      const float* wq = a.w.qkv_w[l] + (size_t)hd * (NTD * 3 * (dh >> 4) * 256);
      const float* bq = a.w.qkv_b[l] + hd * 3 * dh;
      const int NTQ = 3 * (dh >> 4);
      for (int n0 = 0; n0 < NTQ; n0 += 4) {
        const int nn = NTQ - n0 < 4 ? NTQ - n0 : 4;
        zero<MPW>(acc);
        mma<NW, MPW>(acc, ab, LD, wq, 0, NTD, NTQ, n0, nn, MT, wave, lane);
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi) {
          const int m = wave + NW * mi;
          if (m < MT) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              if (ni < nn) {
                const int c = (n0 + ni) * 16 + r;
                const float bias = bq[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  float v = acc[mi][ni][e] + bias;
                  if (c < dh) v *= a.qs;
                  ub[(m * 16 + 4 * g + e) * LDU + c] = v;
                }
              }
          }
        }
      }
      __syncthreads();  // K and V of every row are there

#pragma unroll
      for (int mi = 0; mi < MPW; ++mi) {
        const int m = wave + NW * mi;
        if (m < MT) {
          // scores of the wave's 16 query rows against every key tile: s[kt][e] is row m * 16 + 4 g + e, key kt * 16 + r
          f32x4 s[KT];
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int q = 0; q < (dh >> 4); ++q) {
            const f32x4 qa = *reinterpret_cast<const f32x4*>(ub + (m * 16 + r) * LDU + 16 * q + 4 * g);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
              if (kt < MT) {
                const f32x4 kb = *reinterpret_cast<const f32x4*>(ub + (kt * 16 + r) * LDU + dh + 16 * q + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kb[e], s[kt], 0, 0, 0);
              }
          }
          float mx[4] = {ninf, ninf, ninf, ninf}, sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            if (kt < MT) {
              const bool masked = mkl[kt * 16 + r] != 0;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (masked) s[kt][e] = ninf;
                mx[e] = fmaxf(mx[e], s[kt][e]);
              }
            }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mx[e] = fmaxf(mx[e], __shfl_xor(mx[e], o, 64));
          }
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            if (kt < MT) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                s[kt][e] = expf(s[kt][e] - mx[e]);  // every key masked: -inf - -inf = NaN, as torch
                sum[e] += s[kt][e];
              }
            }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) sum[e] += __shfl_xor(sum[e], o, 64);
          }
          // P = drop( p / sum ), its column sums for the saliency, then P.V through the patch
          f32x4 ov[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            if (kt < MT) {
              const int key = kt * 16 + r;
              float col = 0.f;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int t = m * 16 + 4 * g + e;
                float pv = s[kt][e] / sum[e];
                if (drop && t < T && key < T)
                  pv = lmx_gait_keep(seed, site_p, ((uint64_t)(hd * T + t)) * (uint64_t)T + (uint64_t)key, a.thr) ? pv * a.scale : 0.f;
                if (t < T) col += pv;
                s[kt][e] = pv;
              }
              if (sal_here) {
                col += __shfl_xor(col, 16, 64);
                col += __shfl_xor(col, 32, 64);
                if (g == 0) mysal[key] += col;
              }
              wave_fence();  // the reads of the previous block are done
#pragma unroll
              for (int e = 0; e < 4; ++e) mypatch[(4 * g + e) * PLD + r] = s[kt][e];
              wave_fence();
              const f32x4 pa = *reinterpret_cast<const f32x4*>(mypatch + r * PLD + 4 * g);  // P[row r][keys 4 g .. 4 g + 3]
#pragma unroll
              for (int ct = 0; ct < 2; ++ct)
                if (ct < (dh >> 4)) {
#pragma unroll
                  for (int e = 0; e < 4; ++e)
                    ov[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], ub[(kt * 16 + 4 * g + e) * LDU + 2 * dh + ct * 16 + r], ov[ct], 0, 0, 0);
                }
            }
          // the head's output over q_i's columns of the wave's own rows: no other wave reads them
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
            if (ct < (dh >> 4)) {
#pragma unroll
              for (int e = 0; e < 4; ++e) ub[(m * 16 + 4 * g + e) * LDU + ct * 16 + r] = ov[ct][e];
            }
        }
      }
      __syncthreads();  // every wave has read K and V of this head
      mma<NW, MPW>(racc, ub, LDU, a.w.out_w[l], hd * (dh >> 4), dh >> 4, NTD, 0, NTD, MT, wave, lane);
      __syncthreads();  // ... and its own rows of the output, before the next head's q | k | v land in U
    }
    // h += drop_{2+4l}( o Wo^T + bo )
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + NW * mi;
      if (m < MT) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < NTD) {
            const int c = ni * 16 + r;
            const float bias = a.w.out_b[l][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              float v = racc[mi][ni][e] + bias;
              if (drop && t < T) v = lmx_gait_keep(seed, stream0 + 2 + 4 * l, (uint64_t)(t * D + c), a.thr) ? v * a.scale : 0.f;
              hb[t * LD + c] += v;
            }
          }
      }
    }
    __syncthreads();
    layer_norm<NW, MPW>(hb, ab, a.w.ln2_g[l], a.w.ln2_b[l], D, MT, T, wave, lane, nullptr);
    __syncthreads();
    // the FFN, 64 hidden columns at a time through U; fc2 accumulates over the chunks
    zero<MPW>(racc);
    const int NTF = FF >> 4;
    for (int n0 = 0; n0 < NTF; n0 += 4) {
      const int nn = NTF - n0 < 4 ? NTF - n0 : 4;
      zero<MPW>(acc);
      mma<NW, MPW>(acc, ab, LD, a.w.ff1_w[l], 0, NTD, NTF, n0, nn, MT, wave, lane);
#pragma unroll
      for (int mi = 0; mi < MPW; ++mi) {
        const int m = wave + NW * mi;
        if (m < MT) {
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            if (ni < nn) {
              const int j = (n0 + ni) * 16 + r;
              const float bias = a.w.ff1_b[l][j];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int t = m * 16 + 4 * g + e;
                float v = acc[mi][ni][e] + bias;
                v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
                if (drop && t < T) v = lmx_gait_keep(seed, stream0 + 3 + 4 * l, (uint64_t)(t * FF + j), a.thr) ? v * a.scale : 0.f;
                ub[t * LDU + ni * 16 + r] = v;
              }
            }
        }
      }
      __syncthreads();
      mma<NW, MPW>(racc, ub, LDU, a.w.ff2_w[l], n0, nn, NTD, 0, NTD, MT, wave, lane);
      __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + NW * mi;
      if (m < MT) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < NTD) {
            const int c = ni * 16 + r;
            const float bias = a.w.ff2_b[l][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              float v = racc[mi][ni][e] + bias;
              if (drop && t < T) v = lmx_gait_keep(seed, stream0 + 4 + 4 * l, (uint64_t)(t * D + c), a.thr) ? v * a.scale : 0.f;
              hb[t * LD + c] += v;
            }
          }
      }
    }
    __syncthreads();
  }

  // trunk = LN(h; gf, bf) into tile a
  layer_norm<NW, MPW>(hb, ab, a.w.lnf_g, a.w.lnf_b, D, MT, T, wave, lane, a.trunk ? a.trunk + (size_t)blockIdx.x * T * D : nullptr);
  // The classifier.  Thread j < head fetches row j of fc1 and its fc2 weight BEFORE the pool, so their latency hides under it.
  const int HD = a.w.head;
  f32x4 w1[16];
  float b1 = 0.f, w2 = 0.f;
  if (tid < HD) {
    const f32x4* wr = reinterpret_cast<const f32x4*>(a.w.fc1_w + tid * D);
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) w1[c4] = c4 < (D >> 2) ? wr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    b1 = a.w.fc1_b[tid];
    w2 = a.w.fc2_w[tid];
  }
  __syncthreads();
  if (a.saliency) {
    // the waves' column sums joined in a fixed order, then the mean over the heads
    for (int u = tid; u < T; u += NTH) {
      float s = salw[u];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv) s += salw[wv * TP + u];
      a.saliency[(size_t)clip * T + u] = s / (float)H;
    }
  }
  // the sum over the unmasked steps: one partial sum per wave and channel (t = p, p + NW, ...), joined in a fixed order
  int count = 0;
  {
    const int c = tid & 63, p = tid >> 6;
    float s = 0.f;
    for (int t = p; t < T; t += NW)
      if (!mkl[t]) s += ab[t * LD + (c < D ? c : 0)];
    part[p * 64 + c] = s;
    for (int t = 0; t < T; ++t) count += mkl[t] ? 0 : 1;
  }
  __syncthreads();
  if (tid < 64) {
    float s = part[tid];
#pragma unroll
    for (int p = 1; p < NW; ++p) s += part[p * 64 + tid];
    pooled[tid] = s / (float)(count > 0 ? count : 1);
  }
  __syncthreads();
  if (tid < HD) {
    float s = b1;
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4)
      if (c4 < (D >> 2)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s += w1[c4][e] * pooled[4 * c4 + e];
      }
    s = fmaxf(s, 0.f);
    if (drop) s = lmx_gait_keep(seed, stream0 + 4 * L + 1, (uint64_t)tid, a.thr) ? s * a.scale : 0.f;
    hid[tid] = w2 * s;  // the product of the second linear; thread 0 adds them in order
  }
  __syncthreads();
  if (tid == 0) {
    float z = a.w.fc2_b[0];
    for (int j = 0; j < HD; ++j) z += hid[j];
    // no unmasked step: every softmax of the clip is NaN and torch's pooling keeps it; fmaxf would not, so it is said here
    a.pred[blockIdx.x] = count ? 1.0f / (1.0f + expf(-z)) : __builtin_nanf("");
  }
}

template <int NW, int MPW>
int launch(const XfmArgs& a, unsigned grid, int lds_bytes, int dev, hipStream_t st) {
  // the limit is raised once per (kernel, device): to what the largest T and the widest head of this instantiation need, or the LDS
  constexpr int MTMAX = NW * MPW < 10 ? NW * MPW : 10;
  constexpr int WANT = lds_floats(NW, MTMAX * 16, 100) * (int)sizeof(float);
  const auto kernel = &xfm_forward_kernel<NW, MPW>;
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(kernel), WANT < LDS_LIMIT ? WANT : LDS_LIMIT, dev));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(NW * 64), lds_bytes, st, a);
  return lmx_launch_check("xfm_forward_kernel");
}

}  // namespace

extern "C" int64_t lmx_xfm_workspace_bytes(int n) { return lmx_gait_workspace_bytes(n); }

extern "C" int lmx_k_xfm_forward(const lmx_xfm_weights_t* w, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S,
                                 double p, float* pred, float* stats, float* saliency, float* trunk, void* workspace, lmx_stream_t stream) {
  LMX_TRY(lmx_xfm_check_config("lmx_k_xfm_forward", w, true));
  LMX_TRY(lmx_xfm_check_call("lmx_k_xfm_forward", w, n, T, S, p, saliency != nullptr));
  if (n == 0) return LMX_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned grid = 0;
  int dev = -1;
  LMX_TRY(lmx_gait_launch_prologue("lmx_k_xfm_forward", n, S, x, pred, stats, {trunk, saliency}, seeds_host, workspace, st, &grid, &dev));
  XfmArgs a;
  a.w = *w;
  a.x = x;
  a.mask = mask;
  a.seeds = static_cast<const uint64_t*>(workspace);
  a.pred = pred;
  a.saliency = saliency;
  a.trunk = trunk;
  a.T = T;
  a.S = S;
  a.MT = (T + 15) / 16;
  const int dh = lmx_xfm_head_dim(*w);
  a.LDU = (3 * dh > 64 ? 3 * dh : 64) + 4;
  a.thr = S > 0 ? lmx_gait_threshold(p) : 0;
  a.scale = S > 0 ? lmx_gait_keep_scale(p) : 1.0f;
  a.qs = lmx_xfm_q_scale(dh);
  // Up to 128 steps: 8 waves with one row tile each, two waves per SIMD; on the shipped shape they take 0.73 of the time of 4 waves with
  // two tiles each.  Beyond: 4 waves with three tiles each, because 8 waves with two spill 548 bytes per lane within
  // their 256 registers, and at T = 160 with a head_dim of 32 their patches and strips no longer fit the LDS.
  const int nw = a.MT <= 8 ? 8 : 4;
  const int lds_bytes = lds_floats(nw, a.MT * 16, a.LDU) * (int)sizeof(float);
  LMX_REQUIRE(lds_bytes <= LDS_LIMIT, "lmx_k_xfm_forward: two tiles of %d x %d f32, one of %d x %d and the rest need %d bytes of LDS, a workgroup has %d",
              a.MT * 16, LD, a.MT * 16, a.LDU, lds_bytes, LDS_LIMIT);
  if (nw == 8)
    LMX_TRY((launch<8, 1>(a, grid, lds_bytes, dev, st)));
  else
    LMX_TRY((launch<4, 3>(a, grid, lds_bytes, dev, st)));
  return lmx_gait_stats_launch(pred, stats, n, S, st);
}
