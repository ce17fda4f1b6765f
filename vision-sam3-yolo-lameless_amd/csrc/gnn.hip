// gnn.hip — the live network of GraphGPS in one launch (include/lmx.h "GraphGPS").  One workgroup of NW = 8 waves per
// (graph, sample).  Three tiles of TP = N rounded up to 16 rows x 132 floats live in LDS: the residual stream h, the tile a (a
// LayerNorm's output, then Ax + the aggregated messages) and the work tile U (a wave's 16-edge tiles, then q_i | k_i | v_i of the current
// head, then 64 columns of the FFN's hidden layer at a time).  Node i sits in row i; wave w owns the 16-row tile w of all three (waves
// beyond the graph's tiles only keep the barriers).  Every product over node rows or edge rows runs on the exact f32-input MFMA
// v_mfma_f32_16x16x4_f32 in the operand order of gfm.hip, with which it shares the helpers of graph_tile.h, except that in a product
// with weights no MFMA accumulates into its third operand: `mma` says why (the scores and P.V of the attention still chain).
// Message passing: Bx | Dx | Ex of every node go to the workgroup's slice of the workspace (they are gathered by src and dst of any
// edge and do not fit beside the three tiles); wave w then walks the edges INTO its own 16 nodes in CSR order, 16 at a time: the edge
// features of the tile (layer 0: recomputed from the 3 attributes; later: read from the slice and batch-normalised), Ce, the gate and the
// messages as one tile in U, and ONE RUNNING SUM PER COLUMN that is flushed into the destination's row of a when the destination
// changes.  A destination belongs to one wave and its edges are added in edge order: no atomics, the same bytes on every run.  The
// edge update of the first layers writes ea once to the slice, by CSR position; its batch statistics are a pass of their own.
// Rows beyond N: h stays zero there, they are masked as keys, never enter a batch statistic, are never pooled and never leave the LDS.
// Every index read from the graph (src, dst, csr_ptr, csr_edge) is clamped into the graph before it is used as an address.
#include "gait_launch.h"
#include "gnn.h"
#include "graph_tile.h"

namespace {

constexpr int PCOL = 100;         // a wave's 16 x 16 patch of attention probabilities: columns 100 .. 115 of its own rows of U (q | k | v end at 96)
constexpr int ICOL = 128;         // dst, src and the edge of an edge tile's row, as integers in columns 128 .. 130 of U
constexpr int KT = (LMX_GNN_MAX_NODES + 15) / 16;  // key tiles held in registers
constexpr int TPMAX = KT * 16;
// partial sums | node mean, rstd | edge mean, rstd | pool scores, weights | mean and weighted pool | classifier hidden 1, 2
constexpr int TAIL = NTH + 4 * LMX_GNN_MAX_D + 2 * TPMAX + 2 * LMX_GNN_MAX_D + LMX_GNN_MAX_D + LMX_GNN_MAX_D / 2;

struct GnnArgs {
  lmx_gnn_weights_t w;
  const int32_t *node_off, *edge_off;  // on the device, in the workspace
  const float *x, *lap, *rw, *attr;
  const int32_t *src, *dst, *csr_ptr, *csr_edge, *deg;
  const uint64_t* seeds;
  float* slices;
  long long slice_floats;
  float *node_mc, *graph_pred, *node_pred, *attw, *trunk;
  int S, TP, max_n;
  uint64_t thr;
  float scale, cs;
};

__host__ __device__ constexpr int lds_floats(int TP) { return 3 * TP * LD + TAIL; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// acc[ni] += rows of tile m of src[.][0 .. 16 nq) x the groups q0 .. q0 + nq - 1 and column tiles n0 .. n0 + nn - 1 (nn <= 4) of the
// packed linear layer W with NT column tiles; the B operand of the NEXT group is loaded while the MFMAs of this one run.
// An MFMA chain is one running f32 sum whose rounding error grows with its length, and BatchNorm over the few rows of a small graph
// multiplies the error of the products in front of it by up to 1 / (2 sqrt(eps)) = 158.  So every MFMA starts from zero (four inputs
// per output), and its result joins the sum through the error-free transformation of Knuth's TwoSum: `low` collects what each addition
// rounded away and is added at the end.  The sum over the MFMAs then carries one rounding, not one per MFMA.
__device__ __forceinline__ void mma(f32x4 (&acc)[4], const float* src, int ld, const float* __restrict__ W, int q0, int nq, int NT, int n0, int nn,
                                    int m, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const f32x4* wp = reinterpret_cast<const f32x4*>(W) + ((size_t)q0 * NT + n0) * 64 + lane;
  const f32x4* const wlast = wp + (size_t)(nq - 1) * NT * 64;
  f32x4 b[4], bn[4], low[4];
  zero<4>(low);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) b[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < nq; ++q) {
    if (wp != wlast) wp += NT * 64;  // the last step loads its own operand again
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bn[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (m * 16 + r) * ld + 16 * q + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        if (ni < nn) {
          const f32x4 part = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[ni][e], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          const f32x4 sum = acc[ni] + part, back = sum - acc[ni];
          low[ni] += (acc[ni] - (sum - back)) + (part - back);
          acc[ni] = sum;
        }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) b[ni] = bn[ni];
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] += low[ni];
}

// racc = concat_i( drop_site( softmax(s) )_i v_i ) Wo^T over the rows of `src` [.][LD], the bias of out_proj left to the caller; the keys
// are rows 0 .. N - 1
__device__ __forceinline__ void attention(f32x4 (&racc)[8], const float* src, float* ub, const float* __restrict__ qkv_w, const float* __restrict__ qkv_b,
                                          const float* __restrict__ out_w, int N, int MT, int m, bool act, int lane, int D, int H, int dh, float cs,
                                          const Keep& keep, int site) {
  const int r = lane & 15, g = lane >> 4, NTD = D >> 4, NQ = dh >> 4, NTQ = 3 * NQ;
  const float ninf = -__builtin_huge_valf();
  float* mypatch = ub + (m * 16) * LD + PCOL;
  zero<8>(racc);
  for (int hd = 0; hd < H; ++hd) {
    // q_i | k_i | v_i of this head into U, 4 column tiles at a time
    const float* wq = qkv_w + (size_t)hd * (NTD * NTQ * 256);
    const float* bq = qkv_b + hd * 3 * dh;
    if (act)
      for (int n0 = 0; n0 < NTQ; n0 += 4) {
        const int nn = NTQ - n0 < 4 ? NTQ - n0 : 4;
        f32x4 acc[4];
        zero<4>(acc);
        mma(acc, src, LD, wq, 0, NTD, NTQ, n0, nn, m, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < nn) {
            const int c = (n0 + ni) * 16 + r;
            const float b = bq[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) ub[(m * 16 + 4 * g + e) * LD + c] = acc[ni][e] + b;
          }
      }
    __syncthreads();  // K and V of every row are there

    if (act) {
      // scores of the wave's 16 query rows against every key tile: s[kt][e] is row m * 16 + 4 g + e, key kt * 16 + r
      f32x4 s[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < NQ; ++q) {
        const f32x4 qa = *reinterpret_cast<const f32x4*>(ub + (m * 16 + r) * LD + 16 * q + 4 * g);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
          if (kt < MT) {
            const f32x4 kb = *reinterpret_cast<const f32x4*>(ub + (kt * 16 + r) * LD + dh + 16 * q + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kb[e], s[kt], 0, 0, 0);
          }
      }
      float mx[4] = {ninf, ninf, ninf, ninf}, sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        if (kt < MT) {
          const bool valid = kt * 16 + r < N;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[kt][e] = valid ? s[kt][e] * cs : ninf;
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
            s[kt][e] = expf(s[kt][e] - mx[e]);  // N >= 1: every row has a valid key, so mx is finite
            sum[e] += s[kt][e];
          }
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum[e] += __shfl_xor(sum[e], o, 64);
      }
      // P = drop( p / sum ), then P.V through the patch
      f32x4 ov[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        if (kt < MT) {
          const int key = kt * 16 + r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float pv = s[kt][e] / sum[e];
            if (keep.on && key < N && t < N) pv = keep(pv, site, ((uint64_t)(hd * N + t)) * (uint64_t)N + (uint64_t)key);
            s[kt][e] = pv;
          }
          wave_fence();  // the reads of the previous block are done
#pragma unroll
          for (int e = 0; e < 4; ++e) mypatch[(4 * g + e) * LD + r] = s[kt][e];
          wave_fence();
          const f32x4 pa = *reinterpret_cast<const f32x4*>(mypatch + r * LD + 4 * g);  // P[row r][keys 4 g .. 4 g + 3]
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
            if (ct < NQ) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                ov[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], ub[(kt * 16 + 4 * g + e) * LD + 2 * dh + ct * 16 + r], ov[ct], 0, 0, 0);
            }
        }
      // the head's output over q_i's columns of the wave's own rows: no other wave reads them
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        if (ct < NQ) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ub[(m * 16 + 4 * g + e) * LD + ct * 16 + r] = ov[ct][e];
        }
    }
    __syncthreads();  // every wave has read K and V of this head
    if (act) mma_cols<mma>(racc, ub, LD, out_w, hd * NQ, NQ, NTD, 0, NTD, m, lane);  // the head's share of out_proj as a block of its own
    __syncthreads();  // ... and its own rows of the output, before the next head's q | k | v land in U
  }
}

// mean and 1 / sqrt(biased variance + eps) per channel over the R rows of src (row stride ld floats; LDS or global), two passes, the rows
// dealt to NTH / D groups of threads whose partial sums are added in group order.  Every thread calls.
__device__ __forceinline__ void batch_stats(const float* src, size_t ld, int R, int D, float* red, float* mean, float* rstd, int tid) {
  const int G = NTH / D, c = tid % D, grp = tid / D;
  for (int pass = 0; pass < 2; ++pass) {
    float s = 0.f;
    if (grp < G) {
      const float mu = pass ? mean[c] : 0.f;
      for (int t = grp; t < R; t += G) {
        const float v = src[(size_t)t * ld + c] - mu;
        s += pass ? v * v : v;
      }
    }
    red[tid] = s;
    __syncthreads();
    if (tid < D) {
      float tot = 0.f;
      for (int k = 0; k < G; ++k) tot += red[k * D + tid];
      if (pass)
        rstd[tid] = 1.0f / sqrtf(tot / (float)R + 1e-5f);
      else
        mean[tid] = tot / (float)R;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NTH) void gnn_forward_kernel(const GnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int TPL = a.TP;
  float* hb = lds;
  float* ab = hb + TPL * LD;
  float* ub = ab + TPL * LD;
  float* red = ub + TPL * LD;
  float* nmean = red + NTH;
  float* nrstd = nmean + LMX_GNN_MAX_D;
  float* emean = nrstd + LMX_GNN_MAX_D;
  float* erstd = emean + LMX_GNN_MAX_D;
  float* sc = erstd + LMX_GNN_MAX_D;
  float* ew = sc + TPMAX;
  float* comb = ew + TPMAX;
  float* k1 = comb + 2 * LMX_GNN_MAX_D;
  float* k2 = k1 + LMX_GNN_MAX_D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Smax = a.S > 0 ? a.S : 1, gi = blockIdx.x / Smax, sample = blockIdx.x % Smax;
  const int n0 = a.node_off[gi], N = a.node_off[gi + 1] - n0, e0 = a.edge_off[gi], NE = a.edge_off[gi + 1] - e0, MT = (N + 15) >> 4, m = wave;
  const bool act = wave < MT;
  const int F = a.w.input_dim, D = a.w.d_model, H = a.w.n_heads, dh = D / H, L = a.w.n_layers, FF = a.w.ff, P = a.w.pe_dim, NTD = D >> 4;
  const int DI = D - 2 * P, D2 = D >> 1, D3 = 3 * D, R0 = m * 16;
  const int32_t *ptr = a.csr_ptr + n0 + gi, *cse = a.csr_edge + e0, *esrc = a.src + e0, *edst = a.dst + e0, *deg = a.deg + n0;
  const float* attr = a.attr + (size_t)e0 * 3;
  float* bde = a.slices + (size_t)blockIdx.x * (size_t)a.slice_floats;  // Bx | Dx | Ex [N][3D]
  float* ews = bde + (size_t)a.max_n * D3;                                // ea [E][D] by CSR position
  const bool train = a.S > 0;
  Keep keep;
  keep.on = train;
  keep.seed = train ? a.seeds[gi] : 0;
  keep.stream0 = (uint64_t)sample * (uint64_t)lmx_gnn_n_sites(L);
  keep.thr = a.thr;
  keep.scale = a.scale;

  // h = 0 and the node features into tile a: zeros beyond N and beyond input_dim
  for (int i = tid; i < MT * 16 * LD; i += NTH) hb[i] = 0.f;
  const float* x = a.x + (size_t)n0 * F;
  for (int i = tid; i < MT * 16 * 64; i += NTH) {
    const int t = i >> 6, c = i & 63;
    ab[t * LD + c] = (t < N && c < F) ? x[t * F + c] : 0.f;
  }
  __syncthreads();
  f32x4 racc[8];
  if (act) {
    const int NTI = DI >> 4;
    zero<8>(racc);
    mma_cols<mma>(racc, ab, LD, a.w.in_w, 0, (F + 15) >> 4, NTI, 0, NTI, m, lane);
#pragma unroll
    for (int ni = 0; ni < 8; ++ni)
      if (ni < NTI) {
        const int c = ni * 16 + r;
        const float b = a.w.in_b[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = R0 + 4 * g + e;
          hb[t * LD + c] = t < N ? racc[ni][e] + b : 0.f;
        }
      }
  }
  __syncthreads();
  // the two encodings: their hidden layers (8 and 16 inputs, one thread per output) into U and a ...
  for (int i = tid; i < N * 2 * P; i += NTH) {
    const int t = i / (2 * P), j = i % (2 * P);
    float s1 = a.w.lap1_b[j], s2 = a.w.rw1_b[j];
    const float* lp = a.lap + (size_t)(n0 + t) * LMX_GNN_LAP_K;
    const float* rp = a.rw + (size_t)(n0 + t) * LMX_GNN_RW_K;
    for (int c = 0; c < LMX_GNN_LAP_K; ++c) s1 += a.w.lap1_w[j * LMX_GNN_LAP_K + c] * lp[c];
    for (int c = 0; c < LMX_GNN_RW_K; ++c) s2 += a.w.rw1_w[j * LMX_GNN_RW_K + c] * rp[c];
    ub[t * LD + j] = fmaxf(s1, 0.f);
    ab[t * LD + j] = fmaxf(s2, 0.f);
  }
  __syncthreads();
  // ... and their output layers with the LayerNorm over P channels, one thread per (node, encoding), into h's last 2 P columns
  for (int i = tid; i < 2 * N; i += NTH) {
    const int t = i >> 1, which = i & 1;
    const float* hid = (which ? ab : ub) + t * LD;
    const float* w2 = which ? a.w.rw2_w : a.w.lap2_w;
    const float* b2 = which ? a.w.rw2_b : a.w.lap2_b;
    const float* gm = which ? a.w.rw_g : a.w.lap_g;
    const float* bt = which ? a.w.rw_beta : a.w.lap_beta;
    float* o = hb + t * LD + DI + which * P;
    float sum = 0.f, ss = 0.f;
    for (int c = 0; c < P; ++c) {
      float s = b2[c];
      for (int j = 0; j < 2 * P; ++j) s += w2[c * 2 * P + j] * hid[j];
      o[c] = s;
      sum += s;
    }
    const float mean = sum / (float)P;
    for (int c = 0; c < P; ++c) ss += (o[c] - mean) * (o[c] - mean);
    const float rstd = 1.0f / sqrtf(ss / (float)P + 1e-5f);
    for (int c = 0; c < P; ++c) o[c] = (o[c] - mean) * rstd * gm[c] + bt[c];
  }
  __syncthreads();

  for (int l = 0; l < L; ++l) {
    // ---- message passing --------------------------------------------------------------------------------------------------------------
    if (act) {
      layer_norm<0>(hb, ab, a.w.ln1_g[l], a.w.ln1_b[l], D, N, m, lane, keep, -1, nullptr);
      wave_fence();
      // Bx | Dx | Ex of the wave's rows to the slice, then Ax over the rows of a that the products have read
      for (int nc = NTD; nc < 4 * NTD; nc += 4) {
        const int nn = 4 * NTD - nc < 4 ? 4 * NTD - nc : 4;
        f32x4 acc[4];
        zero<4>(acc);
        mma(acc, ab, LD, a.w.abde_w[l], 0, NTD, 4 * NTD, nc, nn, m, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < nn) {
            const int c = (nc + ni) * 16 + r;
            const float b = a.w.abde_b[l][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = R0 + 4 * g + e;
              if (t < N) bde[(size_t)t * D3 + (c - D)] = acc[ni][e] + b;
            }
          }
      }
      zero<8>(racc);
      mma_cols<mma>(racc, ab, LD, a.w.abde_w[l], 0, NTD, 4 * NTD, 0, NTD, m, lane);
      wave_fence();
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.abde_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) ab[(R0 + 4 * g + e) * LD + c] = racc[ni][e] + b;
        }
    }
    if (l > 0) {
      // how this layer normalises the edge features the layer before wrote: their batch statistics, or the running ones
      if (train) {
        batch_stats(ews, (size_t)D, NE, D, red, emean, erstd, tid);
      } else if (tid < D) {
        emean[tid] = a.w.bne_mean[l - 1][tid];
        erstd[tid] = 1.0f / sqrtf(a.w.bne_var[l - 1][tid] + 1e-5f);
      }
    }
    __syncthreads();  // Bx | Dx | Ex of every node are in the slice
    if (act) {
      const int last = R0 + 16 < N ? R0 + 16 : N;
      const int pb = clampi(ptr[R0], 0, NE), pe = clampi(ptr[last], pb, NE);
      int cur = -1;
      float run0 = 0.f, run1 = 0.f;
      for (int p0 = pb; p0 < pe; p0 += 16) {
        if (lane < 16) {
          const int p = p0 + lane;
          int e = -1, d = -1, s = -1;
          if (p < pe) {
            e = clampi(cse[p], 0, NE - 1);
            d = clampi(edst[e], 0, N - 1);
            s = clampi(esrc[e], 0, N - 1);
          }
          int* ir = reinterpret_cast<int*>(ub + (R0 + lane) * LD + ICOL);
          ir[0] = d, ir[1] = s, ir[2] = e;
        }
        wave_fence();
        // the edge features of the tile into U
        if (l == 0) {
          for (int i = lane; i < 16 * D2; i += 64) {
            const int j = i / D2, c = i % D2, e = reinterpret_cast<const int*>(ub + (R0 + j) * LD + ICOL)[2];
            float v = 0.f;
            if (e >= 0) {
              const float* at = attr + (size_t)e * 3;
              v = fmaxf(((a.w.ee1_b[c] + a.w.ee1_w[c * 3] * at[0]) + a.w.ee1_w[c * 3 + 1] * at[1]) + a.w.ee1_w[c * 3 + 2] * at[2], 0.f);
            }
            ub[(R0 + j) * LD + c] = v;
          }
          wave_fence();
          zero<8>(racc);
          mma_cols<mma>(racc, ub, LD, a.w.ee2_w, 0, D2 >> 4, NTD, 0, NTD, m, lane);
          wave_fence();
#pragma unroll
          for (int ni = 0; ni < 8; ++ni)
            if (ni < NTD) {
              const int c = ni * 16 + r;
              const float b = a.w.ee2_b[c];
#pragma unroll
              for (int e = 0; e < 4; ++e) ub[(R0 + 4 * g + e) * LD + c] = racc[ni][e] + b;
            }
          wave_fence();
          layer_norm<0>(ub, ub, a.w.ee_g, a.w.ee_beta, D, 0, m, lane, keep, -1, nullptr);
        } else {
          for (int i = lane; i < 16 * D; i += 64) {
            const int j = i / D, c = i % D, p = p0 + j;
            ub[(R0 + j) * LD + c] =
                p < pe ? (ews[(size_t)p * D + c] - emean[c]) * erstd[c] * a.w.bne_g[l - 1][c] + a.w.bne_b[l - 1][c] : 0.f;
          }
        }
        wave_fence();
        zero<8>(racc);
        mma_cols<mma>(racc, ub, LD, a.w.c_w[l], 0, NTD, NTD, 0, NTD, m, lane);  // Ce
        wave_fence();
        // the gate and the messages of the tile
#pragma unroll
        for (int ni = 0; ni < 8; ++ni)
          if (ni < NTD) {
            const int c = ni * 16 + r;
            const float cb = a.w.c_b[l][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int j = 4 * g + e;
              const int* ir = reinterpret_cast<const int*>(ub + (R0 + j) * LD + ICOL);
              const int d = ir[0], s = ir[1];
              const float ce = racc[ni][e] + cb;
              racc[ni][e] = ce;
              float msg = 0.f;
              if (d >= 0) {
                const float dv = bde[(size_t)d * D3 + D + c], ev = bde[(size_t)s * D3 + 2 * D + c], bv = bde[(size_t)s * D3 + c];
                msg = 1.0f / (1.0f + expf(-((ce + dv) + ev))) * bv;
              }
              ub[(R0 + j) * LD + c] = msg;
            }
          }
        wave_fence();
        // one running sum per column over the tile's rows, flushed into the destination's row when the destination changes
        for (int j = 0; j < 16; ++j) {
          const int d = reinterpret_cast<const int*>(ub + (R0 + j) * LD + ICOL)[0];
          if (d < 0) break;
          if (d != cur) {
            if (cur >= 0) {
              const float dg = (float)(deg[cur] > 1 ? deg[cur] : 1);
              if (lane < D) ab[cur * LD + lane] += run0 / dg;
              if (lane + 64 < D) ab[cur * LD + lane + 64] += run1 / dg;
            }
            cur = d, run0 = 0.f, run1 = 0.f;
          }
          if (lane < D) run0 += ub[(R0 + j) * LD + lane];
          if (lane + 64 < D) run1 += ub[(R0 + j) * LD + lane + 64];
        }
        if (l < L - 1) {
          // the edge update: [Dx[dst] | Ex[src] | Ce] as three blocks of D inputs through U, then relu, then the second layer
          f32x4 uacc[8];
          zero<8>(uacc);
          for (int part = 0; part < 3; ++part) {
            wave_fence();
            if (part < 2) {
              for (int i = lane; i < 16 * D; i += 64) {
                const int j = i / D, c = i % D;
                const int* ir = reinterpret_cast<const int*>(ub + (R0 + j) * LD + ICOL);
                ub[(R0 + j) * LD + c] = ir[0] >= 0 ? (part == 0 ? bde[(size_t)ir[0] * D3 + D + c] : bde[(size_t)ir[1] * D3 + 2 * D + c]) : 0.f;
              }
            } else {
#pragma unroll
              for (int ni = 0; ni < 8; ++ni)
                if (ni < NTD) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) ub[(R0 + 4 * g + e) * LD + ni * 16 + r] = racc[ni][e];
                }
            }
            wave_fence();
            mma_cols<mma>(uacc, ub, LD, a.w.eu1_w[l], part * NTD, NTD, NTD, 0, NTD, m, lane);
          }
          wave_fence();
#pragma unroll
          for (int ni = 0; ni < 8; ++ni)
            if (ni < NTD) {
              const int c = ni * 16 + r;
              const float b = a.w.eu1_b[l][c];
#pragma unroll
              for (int e = 0; e < 4; ++e) ub[(R0 + 4 * g + e) * LD + c] = fmaxf(uacc[ni][e] + b, 0.f);
            }
          wave_fence();
          zero<8>(racc);
          mma_cols<mma>(racc, ub, LD, a.w.eu2_w[l], 0, NTD, NTD, 0, NTD, m, lane);
#pragma unroll
          for (int ni = 0; ni < 8; ++ni)
            if (ni < NTD) {
              const int c = ni * 16 + r;
              const float b = a.w.eu2_b[l][c];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int p = p0 + 4 * g + e;
                if (p < pe) ews[(size_t)p * D + c] = racc[ni][e] + b;
              }
            }
        }
        wave_fence();
      }
      if (cur >= 0) {
        const float dg = (float)(deg[cur] > 1 ? deg[cur] : 1);
        if (lane < D) ab[cur * LD + lane] += run0 / dg;
        if (lane + 64 < D) ab[cur * LD + lane + 64] += run1 / dg;
      }
    }
    __syncthreads();  // Ax + agg of every node is in a; ea of every edge is in the slice
    if (train) {
      batch_stats(ab, (size_t)LD, N, D, red, nmean, nrstd, tid);
    } else {
      if (tid < D) {
        nmean[tid] = a.w.bnn_mean[l][tid];
        nrstd[tid] = 1.0f / sqrtf(a.w.bnn_var[l][tid] + 1e-5f);
      }
      __syncthreads();
    }
    if (act) {
      // h += drop( relu( BN(Ax + agg) ) ), then norm2 into a
      for (int i = lane; i < 16 * D; i += 64) {
        const int t = R0 + i / D, c = i % D;
        if (t < N) {
          const float v = fmaxf((ab[t * LD + c] - nmean[c]) * nrstd[c] * a.w.bnn_g[l][c] + a.w.bnn_b[l][c], 0.f);
          hb[t * LD + c] += keep(v, 5 * l, (uint64_t)(t * D + c));
        }
      }
      wave_fence();
      layer_norm<0>(hb, ab, a.w.ln2_g[l], a.w.ln2_b[l], D, N, m, lane, keep, -1, nullptr);
    }
    __syncthreads();
    // ---- global attention -------------------------------------------------------------------------------------------------------------
    attention(racc, ab, ub, a.w.qkv_w[l], a.w.qkv_b[l], a.w.out_w[l], N, MT, m, act, lane, D, H, dh, a.cs, keep, 5 * l + 1);
    if (act) {
      // g = LN( a + drop( o Wo^T + bo ) ) through the wave's rows of U; h += g - a
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.out_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = R0 + 4 * g + e;
            float v = racc[ni][e] + b;
            if (t < N) v = keep(v, 5 * l + 2, (uint64_t)(t * D + c));
            ub[t * LD + c] = ab[t * LD + c] + v;
          }
        }
      wave_fence();
      layer_norm<0>(ub, ub, a.w.lna_g[l], a.w.lna_b[l], D, N, m, lane, keep, -1, nullptr);
      wave_fence();
      for (int i = lane; i < 16 * D; i += 64) {
        const int t = R0 + i / D, c = i % D;
        if (t < N) hb[t * LD + c] += ub[t * LD + c] - ab[t * LD + c];
      }
      wave_fence();
      layer_norm<0>(hb, ab, a.w.ln3_g[l], a.w.ln3_b[l], D, N, m, lane, keep, -1, nullptr);
      wave_fence();
      // ---- the FFN, 64 hidden columns at a time through U; fc2 accumulates over the chunks ---------------------------------------------
      zero<8>(racc);
      const int NTF = FF >> 4;
      for (int n0f = 0; n0f < NTF; n0f += 4) {
        const int nn = NTF - n0f < 4 ? NTF - n0f : 4;
        f32x4 acc[4];
        zero<4>(acc);
        mma(acc, ab, LD, a.w.ff1_w[l], 0, NTD, NTF, n0f, nn, m, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < nn) {
            const int j = (n0f + ni) * 16 + r;
            const float b = a.w.ff1_b[l][j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = R0 + 4 * g + e;
              float v = acc[ni][e] + b;
              v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
              if (t < N) v = keep(v, 5 * l + 3, (uint64_t)(t * FF + j));
              ub[t * LD + ni * 16 + r] = v;
            }
          }
        wave_fence();  // the chunk is read by the wave that wrote it
        mma_cols<mma>(racc, ub, LD, a.w.ff2_w[l], n0f, nn, NTD, 0, NTD, m, lane);
        wave_fence();
      }
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.ff2_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = R0 + 4 * g + e;
            if (t < N) hb[t * LD + c] += keep(racc[ni][e] + b, 5 * l + 4, (uint64_t)(t * D + c));
          }
        }
      wave_fence();
    }
    __syncthreads();  // every wave is done with the slice before the next layer overwrites it
  }

  // ---- the heads on t = LN(h; final_norm) in tile a --------------------------------------------------------------------------------------
  if (act) {
    layer_norm<0>(hb, ab, a.w.lnf_g, a.w.lnf_b, D, N, m, lane, keep, -1, a.trunk ? a.trunk + ((size_t)n0 * Smax + (size_t)sample * N) * D : nullptr);
    wave_fence();
    const int NTP = D2 >> 4;
    for (int which = train ? 1 : 0; which < 2; ++which) {  // 0: the attention pool's scores (eval mode), 1: the node head
      const float* w1 = which ? a.w.nh1_w : a.w.na1_w;
      const float* b1 = which ? a.w.nh1_b : a.w.na1_b;
      const float* w2 = which ? a.w.nh2_w : a.w.na2_w;
      const float b2 = which ? a.w.nh2_b[0] : a.w.na2_b[0];
      f32x4 acc[4];
      zero<4>(acc);
      mma(acc, ab, LD, w1, 0, NTD, NTP, 0, NTP, m, lane);
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        if (ni < NTP) {
          const int c = ni * 16 + r;
          const float b = b1[c], wv = w2[c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = R0 + 4 * g + e;
            const float v = acc[ni][e] + b;
            part[e] += wv * (which ? (t < N ? keep(fmaxf(v, 0.f), 5 * L, (uint64_t)(t * D2 + c)) : 0.f) : tanhf(v));
          }
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) part[e] += __shfl_xor(part[e], o, 64);
        const int t = R0 + 4 * g + e;
        if (r == 0 && t < N) {
          if (!which) {
            sc[t] = part[e] + b2;
          } else {
            const float y = 1.0f / (1.0f + expf(-(part[e] + b2)));
            if (train)
              a.node_mc[(size_t)(n0 + t) * a.S + sample] = y;
            else
              a.node_pred[n0 + t] = y;
          }
        }
      }
    }
  }
  if (train) return;
  __syncthreads();
  if (tid < N) {
    float mx = sc[0];
    for (int t = 1; t < N; ++t) mx = fmaxf(mx, sc[t]);
    ew[tid] = expf(sc[tid] - mx);
  }
  __syncthreads();
  if (tid < N) {
    float esum = 0.f;
    for (int t = 0; t < N; ++t) esum += ew[t];
    const float wgt = ew[tid] / esum;
    sc[tid] = wgt;
    a.attw[n0 + tid] = wgt;
  }
  __syncthreads();
  // mean | sum_i w_i t[i], the sums over the nodes in ascending order
  if (tid < D) {
    float sum = 0.f, pool = 0.f;
    for (int t = 0; t < N; ++t) sum += ab[t * LD + tid];
    for (int t = 0; t < N; ++t) pool += sc[t] * ab[t * LD + tid];
    comb[tid] = sum / (float)N;
    comb[D + tid] = pool;
  }
  __syncthreads();
  if (tid < D) {
    float s = a.w.cl1_b[tid];
    for (int k = 0; k < 2 * D; ++k) s += a.w.cl1_w[(size_t)k * D + tid] * comb[k];
    k1[tid] = fmaxf(s, 0.f);
  }
  __syncthreads();
  if (tid < D2) {
    float s = a.w.cl2_b[tid];
    for (int c = 0; c < D; ++c) s += a.w.cl2_w[(size_t)c * D2 + tid] * k1[c];
    k2[tid] = fmaxf(s, 0.f);
  }
  __syncthreads();
  if (tid == 0) {
    float z = a.w.cl3_b[0];
    for (int j = 0; j < D2; ++j) z += a.w.cl3_w[j] * k2[j];
    a.graph_pred[gi] = 1.0f / (1.0f + expf(-z));
  }
}

// seeds u64 [n] | node_off i32 [n + 1] | edge_off i32 [n + 1] | up to 16 bytes | one slice per workgroup
inline int64_t slices_offset(int n) { return ((int64_t)n * 8 + (int64_t)(n + 1) * 8 + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t lmx_gnn_workspace_bytes(int n, int S, int max_nodes, int max_edges, int d_model, int n_layers) {
  if (n <= 0 || S < 0 || max_nodes <= 0 || max_edges < 0 || d_model <= 0 || n_layers <= 0) return 0;
  return slices_offset(n) + (int64_t)n * (S > 0 ? S : 1) * lmx_gnn_slice_floats(max_nodes, max_edges, d_model, n_layers) * 4;
}

extern "C" int lmx_k_gnn_forward(const lmx_gnn_weights_t* w, const lmx_gnn_graphs_t* gr, const uint64_t* seeds_host, int S, double p, float* node_mc,
                                 float* stats, float* graph_pred, float* node_pred, float* attn_weights, float* trunk, void* workspace,
                                 lmx_stream_t stream) {
  const char* who = "lmx_k_gnn_forward";
  LMX_TRY(lmx_gnn_check_config(who, w, true));
  int64_t nodes = 0;
  int max_n = 0, max_e = 0;
  LMX_TRY(lmx_gnn_check_call(who, w, gr, S, p, node_mc || stats, graph_pred || node_pred || attn_weights, &nodes, &max_n, &max_e));
  const int n = gr->n;
  if (n == 0) return LMX_OK;
  const bool have_edges = gr->edge_off_host[n] > 0;
  LMX_REQUIRE(gr->lap && gr->rw && gr->csr_ptr && gr->deg && (!have_edges || (gr->edge_src && gr->edge_dst && gr->edge_attr && gr->csr_edge)) &&
                  workspace,
              "%s: null pointer", who);
  LMX_REQUIRE(S > 0 ? (node_mc && stats) : (graph_pred && node_pred && attn_weights), "%s: an output of S = %d is null", who, S);
  LMX_REQUIRE((((uintptr_t)gr->lap | (uintptr_t)gr->rw | (uintptr_t)gr->edge_src | (uintptr_t)gr->edge_dst | (uintptr_t)gr->edge_attr |
                (uintptr_t)gr->csr_ptr | (uintptr_t)gr->csr_edge | (uintptr_t)gr->deg | (uintptr_t)node_mc | (uintptr_t)stats | (uintptr_t)graph_pred |
                (uintptr_t)node_pred | (uintptr_t)attn_weights | (uintptr_t)trunk) & 3) == 0 &&
                  ((uintptr_t)workspace & 15) == 0,
              "%s: misaligned pointer", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned grid = 0;
  int dev = -1;
  LMX_TRY(lmx_gait_launch_prologue(who, n, S, gr->x, S > 0 ? node_mc : graph_pred, S > 0 ? stats : node_pred, {trunk}, seeds_host, workspace, st, &grid,
                                   &dev));
  char* ws = static_cast<char*>(workspace);
  LMX_HIP(hipMemcpyAsync(ws + (size_t)n * 8, gr->node_off_host, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
  LMX_HIP(hipMemcpyAsync(ws + (size_t)n * 8 + (size_t)(n + 1) * 4, gr->edge_off_host, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
  GnnArgs a;
  a.w = *w;
  a.seeds = reinterpret_cast<const uint64_t*>(ws);
  a.node_off = reinterpret_cast<const int32_t*>(ws + (size_t)n * 8);
  a.edge_off = a.node_off + (n + 1);
  a.slices = reinterpret_cast<float*>(ws + slices_offset(n));
  a.slice_floats = lmx_gnn_slice_floats(max_n, max_e, w->d_model, w->n_layers);
  a.max_n = max_n;
  a.x = gr->x;
  a.lap = gr->lap;
  a.rw = gr->rw;
  a.attr = gr->edge_attr;
  a.src = gr->edge_src;
  a.dst = gr->edge_dst;
  a.csr_ptr = gr->csr_ptr;
  a.csr_edge = gr->csr_edge;
  a.deg = gr->deg;
  a.node_mc = node_mc;
  a.graph_pred = graph_pred;
  a.node_pred = node_pred;
  a.attw = attn_weights;
  a.trunk = trunk;
  a.S = S;
  a.TP = (max_n + 15) / 16 * 16;
  a.thr = S > 0 ? lmx_gait_threshold(p) : 0;
  a.scale = S > 0 ? lmx_gait_keep_scale(p) : 1.0f;
  a.cs = lmx_gnn_score_scale(lmx_gnn_head_dim(*w));
  const int lds_bytes = lds_floats(a.TP) * (int)sizeof(float);
  constexpr int WANT = lds_floats(TPMAX) * (int)sizeof(float);
  static_assert(WANT <= LDS_LIMIT, "LMX_GNN_MAX_NODES: the tiles do not fit the LDS");
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(&gnn_forward_kernel), WANT, dev));
  hipLaunchKernelGGL(gnn_forward_kernel, dim3(grid), dim3(NTH), lds_bytes, st, a);
  LMX_TRY(lmx_launch_check("gnn_forward_kernel"));
  if (S > 0) return lmx_gait_stats_launch(node_mc, stats, (int)nodes, S, st);
  return LMX_OK;
}
