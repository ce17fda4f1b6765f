// gfm.hip — the whole graph transformer in one launch (include/lmx.h "The graph transformer").
// A small kernel in front fills the attention bias [H][N][N] of every graph ONCE (it depends on no keep bit); then one workgroup of
// NW = 8 waves per (graph, sample) runs the network.  Three tiles live in LDS, TP = N + 1 rounded up to 16 rows: the residual stream
// h [TP][132], the LayerNorm output a [TP][132] and a work tile U [TP][LDU], LDU = max(3 dh, 64) + 4, which holds q_i | k_i | v_i of the
// CURRENT head and then 64 columns of the FFN's hidden layer at a time.  ROW 0 OF EVERY TILE IS THE VIRTUAL NODE'S, node i sits in row
// i + 1: the graph attention masks row 0 as a key and ignores it as a query, the virtual-node attention writes vn_l there and needs no
// shifted copy of h.  Every product over the rows runs on the exact f32-input MFMA v_mfma_f32_16x16x4_f32 with the operand order of
// xfm.hip: wave w owns the 16-row tile w (waves beyond the graph's tiles only keep the barriers), reads ONE float4 of A per 16 inputs
// from LDS and one float4 of B per column tile straight from the packed weights in L2, one step ahead of the MFMAs.  Up to EIGHT column
// tiles of accumulators per row tile (D = 128) stay in registers for out_proj and fc2.  Rows are wave-private everywhere except K and V
// of a head, which every wave reads.  The single-row layers (the virtual node's update, the readout, the graph head) are one thread per
// output over transposed weights, with the host's sequential sums.
// Rows beyond N: h starts as zeros there and stays finite, they are masked as keys (their score is -inf, so P is exactly 0 where V
// holds them), never pooled, and never leave the LDS.
// graph_tile.h has what this kernel shares with gnn.hip: the workgroup's shape, wave_fence, zero, Keep, layer_norm and mma_cols.
#include "gait_launch.h"
#include "gfm.h"
#include "graph_tile.h"

namespace {

constexpr int PLD = 20;           // floats per row of a wave's 16 x 16 patch
constexpr int PATCH = 16 * PLD;
constexpr int KT = (LMX_GFM_MAX_NODES + 1 + 15) / 16;  // key tiles held in registers
constexpr int TAIL = 3 * LMX_GFM_MAX_D + 2 * LMX_GFM_MAX_D + LMX_GFM_MAX_D + LMX_GFM_MAX_D / 2 + LMX_GFM_MAX_D / 4;  // comb | vnv | gr | h1 | h2

struct GfmArgs {
  lmx_gfm_weights_t w;
  const int32_t *node_off, *edge_off;  // on the device, in the workspace
  const float *x, *ts;
  const uint8_t *has_time, *deg_in, *deg_out, *idx;
  const int32_t* win;
  const float* edge_attr;
  const int32_t* target;
  const uint64_t* seeds;
  float* bias;
  float *pred, *node_pred, *attn, *trunk, *vn;
  int S, TP, LDU;
  uint64_t thr;
  float scale, cs;
};

// h | a | U | one patch per wave | pool scores, attention column, pool weights (one per row) | the single-row vectors
__host__ __device__ constexpr int lds_floats(int TP, int LDU) { return TP * (2 * LD + LDU + 3) + NW * PATCH + TAIL; }

// sum of N^2 over the graphs in front of graph g: where its matrices start.  `red`: nth 64-bit words of LDS; every thread calls.
__device__ __forceinline__ long long cells_before(const int32_t* node_off, int g, long long* red, int tid, int nth) {
  long long s = 0;
  for (int i = tid; i < g; i += nth) {
    const long long N = node_off[i + 1] - node_off[i];
    s += N * N;
  }
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    const int lim = g < nth ? g : nth;
    for (int i = 1; i < lim; ++i) s += red[i];
    red[0] = s;
  }
  __syncthreads();
  const long long out = red[0];
  __syncthreads();
  return out;
}

// acc[ni] += rows of tile m of src[.][0 .. 16 nq) x the groups q0 .. q0 + nq - 1 and column tiles n0 .. n0 + nn - 1 (nn <= NC) of the
// packed linear layer W with NT column tiles.  The B operand of the NEXT group is loaded while the MFMAs of this one run.
// An MFMA chain is one running f32 sum, whose rounding error grows with its length.  With four column tiles the groups of even and odd q
// go to two accumulators that are added at the end; the callers with eight keep their chains short themselves (one head, one FFN chunk)
// and add the blocks: the error of sqrt(blocks) shorter chains, as a blocked CPU GEMM has it.
template <int NC>
__device__ __forceinline__ void mma(f32x4 (&acc)[NC], const float* src, int ld, const float* __restrict__ W, int q0, int nq, int NT, int n0, int nn,
                                    int m, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const f32x4* wp = reinterpret_cast<const f32x4*>(W) + ((size_t)q0 * NT + n0) * 64 + lane;
  const f32x4* const wlast = wp + (size_t)(nq - 1) * NT * 64;
  f32x4 b[NC], bn[NC], odd[NC == 4 ? NC : 1];
  if (NC == 4) zero(odd);
#pragma unroll
  for (int ni = 0; ni < NC; ++ni) b[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < nq; ++q) {
    if (wp != wlast) wp += NT * 64;  // the last step loads its own operand again
#pragma unroll
    for (int ni = 0; ni < NC; ++ni) bn[ni] = ni < nn ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (m * 16 + r) * ld + 16 * q + 4 * g);
    if (NC == 4 && (q & 1)) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ni = 0; ni < NC; ++ni)
          if (ni < nn) odd[NC == 4 ? ni : 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[ni][e], odd[NC == 4 ? ni : 0], 0, 0, 0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ni = 0; ni < NC; ++ni)
          if (ni < nn) acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[ni][e], acc[ni], 0, 0, 0);
    }
#pragma unroll
    for (int ni = 0; ni < NC; ++ni) b[ni] = bn[ni];
  }
  if (NC == 4) {
#pragma unroll
    for (int ni = 0; ni < NC; ++ni) acc[ni] += odd[NC == 4 ? ni : 0];
  }
}

// One attention over the rows of `src` [.][LD]: racc = concat_i( drop_site( softmax(s) )_i v_i ) Wo^T, the bias of out_proj left to the
// caller.  VN = false: the graph attention, the keys are rows 1 .. N; tcol (a row, or -1): attw[t] += P_head[t][tcol] per head.
// VN = true: the virtual-node attention, the keys are rows 0 .. N and the bias is 0 in row 0 and column 0.
template <bool VN>
__device__ __forceinline__ void attention(f32x4 (&racc)[8], const float* src, float* ub, float* mypatch, float* attw, const float* __restrict__ qkv_w,
                                          const float* __restrict__ qkv_b, const float* __restrict__ out_w, const float* __restrict__ bias, int N, int MT,
                                          int m, bool act, int lane, int D, int H, int dh, int LDU, float cs, const Keep& keep, int site, int tcol) {
  const int r = lane & 15, g = lane >> 4, NTD = D >> 4, NQ = dh >> 4, NTQ = 3 * NQ;
  const float ninf = -__builtin_huge_valf();
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
        mma<4>(acc, src, LD, wq, 0, NTD, NTQ, n0, nn, m, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < nn) {
            const int c = (n0 + ni) * 16 + r;
            const float b = bq[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) ub[(m * 16 + 4 * g + e) * LDU + c] = acc[ni][e] + b;
          }
      }
    __syncthreads();  // K and V of every row are there

    if (act) {
      // scores of the wave's 16 query rows against every key tile: s[kt][e] is row m * 16 + 4 g + e, key kt * 16 + r
      f32x4 s[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < NQ; ++q) {
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
          const int key = kt * 16 + r;
          const bool node_key = key >= 1 && key <= N, valid = VN ? key <= N : node_key;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float b = 0.f;
            if (node_key && t >= 1 && t <= N) b = bias[((size_t)hd * N + (t - 1)) * N + (key - 1)];
            s[kt][e] = valid ? s[kt][e] * cs + b : ninf;
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
      // P = drop( p / sum ), the target's column, then P.V through the patch
      f32x4 ov[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        if (kt < MT) {
          const int key = kt * 16 + r;
          const bool valid = VN ? key <= N : (key >= 1 && key <= N);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float pv = s[kt][e] / sum[e];
            if (keep.on && valid) {
              if (VN) {
                if (t <= N) pv = keep(pv, site, ((uint64_t)(hd * (N + 1) + t)) * (uint64_t)(N + 1) + (uint64_t)key);
              } else if (t >= 1 && t <= N) {
                pv = keep(pv, site, ((uint64_t)(hd * N + t - 1)) * (uint64_t)N + (uint64_t)(key - 1));
              }
            }
            if (!VN && key == tcol) attw[t] += pv;  // one lane per row, the heads in ascending order
            s[kt][e] = pv;
          }
          wave_fence();  // the reads of the previous block are done
#pragma unroll
          for (int e = 0; e < 4; ++e) mypatch[(4 * g + e) * PLD + r] = s[kt][e];
          wave_fence();
          const f32x4 pa = *reinterpret_cast<const f32x4*>(mypatch + r * PLD + 4 * g);  // P[row r][keys 4 g .. 4 g + 3]
#pragma unroll
          for (int ct = 0; ct < 2; ++ct)
            if (ct < NQ) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                ov[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], ub[(kt * 16 + 4 * g + e) * LDU + 2 * dh + ct * 16 + r], ov[ct], 0, 0, 0);
            }
        }
      // the head's output over q_i's columns of the wave's own rows: no other wave reads them
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        if (ct < NQ) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ub[(m * 16 + 4 * g + e) * LDU + ct * 16 + r] = ov[ct][e];
        }
    }
    __syncthreads();  // every wave has read K and V of this head
    if (act) mma_cols<mma<4>>(racc, ub, LDU, out_w, hd * NQ, NQ, NTD, 0, NTD, m, lane);  // the head's share of out_proj as a block of its own
    __syncthreads();  // ... and its own rows of the output, before the next head's q | k | v land in U
  }
}

// bias[H][N][N] of every graph into the workspace: one thread per (i, j), graph blockIdx.x
__global__ __launch_bounds__(256) void gfm_bias_kernel(const GfmArgs a) {
  __shared__ long long red[256];
  const int gi = blockIdx.x, tid = threadIdx.x;
  const int n0 = a.node_off[gi], N = a.node_off[gi + 1] - n0, e0 = a.edge_off[gi], NE = a.edge_off[gi + 1] - e0;
  if ((int)blockIdx.y * 256 >= N * N) return;  // the whole block
  const long long moff = cells_before(a.node_off, gi, red, tid, 256);
  const int cell = blockIdx.y * 256 + tid;
  if (cell >= N * N) return;
  const int H = a.w.n_heads, NI = a.w.max_spd + 2;
  int id = a.idx[moff + cell];
  id = id < NI ? id : NI - 1;
  const int e = a.win[moff + cell];
  const bool edge = e >= 0 && e < NE;
  float eh[16];
  if (edge) {
    const float* at = a.edge_attr + (size_t)(e0 + e) * 3;
    const float a0 = at[0], a1 = at[1], a2 = at[2];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < 2 * H) eh[j] = fmaxf(((a.w.e1_b[j] + a.w.e1_w[j * 3] * a0) + a.w.e1_w[j * 3 + 1] * a1) + a.w.e1_w[j * 3 + 2] * a2, 0.f);
  }
  float* out = a.bias + (size_t)H * moff + cell;
  for (int hd = 0; hd < H; ++hd) {
    float v = 0.f;
    if (edge) {
      v = a.w.e2_b[hd];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < 2 * H) v += a.w.e2_w[hd * 2 * H + j] * eh[j];
    }
    out[(size_t)hd * N * N] = a.w.spd[id * H + hd] + v;
  }
}

__global__ __launch_bounds__(NTH) void gfm_forward_kernel(const GfmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int TPL = a.TP, LDU = a.LDU;
  float* hb = lds;
  float* ab = hb + TPL * LD;
  float* ub = ab + TPL * LD;
  float* patch = ub + TPL * LDU;
  float* sc = patch + NW * PATCH;
  float* attw = sc + TPL;
  float* ew = attw + TPL;
  float* comb = ew + TPL;
  float* vnv = comb + 3 * LMX_GFM_MAX_D;
  float* gr = vnv + 2 * LMX_GFM_MAX_D;
  float* h1 = gr + LMX_GFM_MAX_D;
  float* h2 = h1 + LMX_GFM_MAX_D / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Smax = a.S > 0 ? a.S : 1, gi = blockIdx.x / Smax, sample = blockIdx.x % Smax;
  const int n0 = a.node_off[gi], N = a.node_off[gi + 1] - n0, MT = (N + 1 + 15) >> 4, m = wave;
  const bool act = wave < MT;
  const int F = a.w.input_dim, D = a.w.d_model, H = a.w.n_heads, dh = D / H, L = a.w.n_layers, FF = a.w.ff, NTD = D >> 4;
  Keep keep;
  keep.on = a.S > 0;
  keep.seed = keep.on ? a.seeds[gi] : 0;
  keep.stream0 = (uint64_t)sample * (uint64_t)(6 * L + 4);
  keep.thr = a.thr;
  keep.scale = a.scale;
  float* mypatch = patch + wave * PATCH;
  const long long moff = cells_before(a.node_off, gi, reinterpret_cast<long long*>(ub), tid, NTH);
  const float* bias = a.bias + (size_t)H * moff;
  int tcol = -1;
  if (a.attn && a.target) {
    const int tg = a.target[gi];
    if (tg >= 0 && tg < N) tcol = tg + 1;
  }

  // h = 0, the attention column, and the node features into tile a: zeros in row 0, beyond N and beyond input_dim
  for (int i = tid; i < MT * 16 * LD; i += NTH) hb[i] = 0.f;
  for (int u = tid; u < TPL; u += NTH) attw[u] = 0.f;
  const float* x = a.x + (size_t)n0 * F;
  for (int i = tid; i < MT * 16 * 64; i += NTH) {
    const int t = i >> 6, c = i & 63;
    ab[t * LD + c] = (t >= 1 && t <= N && c < F) ? x[(t - 1) * F + c] : 0.f;
  }
  __syncthreads();

  f32x4 racc[8];
  // h = drop_0( LN( x W_in^T + b_in ) ) + enc; every step on the wave's own rows
  if (act) {
    zero<8>(racc);
    mma<8>(racc, ab, LD, a.w.in_w, 0, (F + 15) >> 4, NTD, 0, NTD, m, lane);
#pragma unroll
    for (int ni = 0; ni < 8; ++ni)
      if (ni < NTD) {
        const int c = ni * 16 + r;
        const float b = a.w.in_b[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = m * 16 + 4 * g + e;
          hb[t * LD + c] = (t >= 1 && t <= N) ? racc[ni][e] + b : 0.f;
        }
      }
    wave_fence();
    layer_norm<1>(hb, hb, a.w.in_g, a.w.in_beta, D, N, m, lane, keep, 0, nullptr);
    const bool timed = a.has_time != nullptr && a.has_time[gi] != 0;
    if (timed) {
      const float* ts = a.ts + n0;
      float tmin = ts[0];
      for (int t = 1; t < N; ++t) tmin = fminf(tmin, ts[t]);
      for (int i = lane; i < 16 * D; i += 64) {
        const int t = m * 16 + i / D, c = i % D;
        float v = 0.f;
        if (t >= 1 && t <= N) {
          const float days = fminf((ts[t - 1] - tmin) / 86400.0f, 365.0f), arg = days * a.w.div_term[c >> 1];
          v = (c & 1) ? cosf(arg) : sinf(arg);
        }
        ab[t * LD + c] = v;
      }
      wave_fence();
      zero<8>(racc);
      mma<8>(racc, ab, LD, a.w.time_w, 0, NTD, NTD, 0, NTD, m, lane);
    }
    wave_fence();
#pragma unroll
    for (int ni = 0; ni < 8; ++ni)
      if (ni < NTD) {
        const int c = ni * 16 + r;
        const float tb = timed ? a.w.time_b[c] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = m * 16 + 4 * g + e;
          if (t >= 1 && t <= N) {
            int di = a.deg_in[n0 + t - 1], dq = a.deg_out[n0 + t - 1];
            di = di < a.w.max_degree ? di : a.w.max_degree;
            dq = dq < a.w.max_degree ? dq : a.w.max_degree;
            float enc = a.w.deg_in[(size_t)di * D + c] + a.w.deg_out[(size_t)dq * D + c];
            if (timed) enc += racc[ni][e] + tb;
            hb[t * LD + c] += enc;
          }
        }
      }
  }
  __syncthreads();

  for (int l = 0; l < L; ++l) {
    if (act) layer_norm<1>(hb, ab, a.w.ln1_g[l], a.w.ln1_b[l], D, N, m, lane, keep, -1, nullptr);
    __syncthreads();
    attention<false>(racc, ab, ub, mypatch, attw, a.w.qkv_w[l], a.w.qkv_b[l], a.w.out_w[l], bias, N, MT, m, act, lane, D, H, dh, LDU, a.cs, keep,
                     1 + 6 * l, l == L - 1 ? tcol : -1);
    // h += drop_{2+6l}( o Wo^T + bo )
    if (act) {
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.out_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float v = racc[ni][e] + b;
            if (t >= 1 && t <= N) v = keep(v, 2 + 6 * l, (uint64_t)((t - 1) * D + c));
            hb[t * LD + c] += v;
          }
        }
      wave_fence();
      layer_norm<1>(hb, ab, a.w.ln2_g[l], a.w.ln2_b[l], D, N, m, lane, keep, -1, nullptr);
    }
    __syncthreads();
    // the FFN, 64 hidden columns at a time through U; fc2 accumulates over the chunks
    zero<8>(racc);
    const int NTF = FF >> 4;
    for (int n0f = 0; n0f < NTF; n0f += 4) {
      const int nn = NTF - n0f < 4 ? NTF - n0f : 4;
      if (act) {
        f32x4 acc[4];
        zero<4>(acc);
        mma<4>(acc, ab, LD, a.w.ff1_w[l], 0, NTD, NTF, n0f, nn, m, lane);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < nn) {
            const int j = (n0f + ni) * 16 + r;
            const float b = a.w.ff1_b[l][j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              float v = acc[ni][e] + b;
              v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
              if (t >= 1 && t <= N) v = keep(v, 3 + 6 * l, (uint64_t)((t - 1) * FF + j));
              ub[t * LDU + ni * 16 + r] = v;
            }
          }
        wave_fence();  // the chunk is read by the wave that wrote it
        mma_cols<mma<4>>(racc, ub, LDU, a.w.ff2_w[l], n0f, nn, NTD, 0, NTD, m, lane);
        wave_fence();
      }
    }
    if (act) {
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.ff2_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float v = racc[ni][e] + b;
            if (t >= 1 && t <= N) v = keep(v, 4 + 6 * l, (uint64_t)((t - 1) * D + c));
            hb[t * LD + c] += v;
          }
        }
      // the virtual node of this layer into row 0
      if (wave == 0)
        for (int c = lane; c < D; c += 64) hb[c] = a.w.vn[l][c];
    }
    __syncthreads();
    attention<true>(racc, hb, ub, mypatch, attw, a.w.vqkv_w[l], a.w.vqkv_b[l], a.w.vout_w[l], bias, N, MT, m, act, lane, D, H, dh, LDU, a.cs, keep,
                    5 + 6 * l, -1);
    // rows 0 .. N of drop_{6+6l}( o Wo^T + bo ) replace [vn ; h]
    if (act) {
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
        if (ni < NTD) {
          const int c = ni * 16 + r;
          const float b = a.w.vout_b[l][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = m * 16 + 4 * g + e;
            float v = racc[ni][e] + b;
            if (t <= N) v = keep(v, 6 + 6 * l, (uint64_t)(t * D + c));
            hb[t * LD + c] = v;
          }
        }
    }
    __syncthreads();
  }

  // the target's column: the heads were added in order, by the lane that owns the row
  if (a.attn)
    for (int u = tid; u < N; u += NTH) a.attn[n0 + u] = tcol >= 0 ? attw[u + 1] / (float)H : 0.f;
  // vn = LN( gelu( y[0] U1^T + c1 ) U2^T + c2 ) of the last layer, one thread per output; trunk = LN(h; gf, bf) into tile a
  for (int j = tid; j < 2 * D; j += NTH) {
    float s = a.w.vu1_b[j];
    for (int c = 0; c < D; ++c) s += a.w.vu1_w[(size_t)c * 2 * D + j] * hb[c];
    vnv[j] = 0.5f * s * (1.0f + erff(s * 0.70710678118654752440f));
  }
  if (act)
    layer_norm<1>(hb, ab, a.w.lnf_g, a.w.lnf_b, D, N, m, lane, keep, -1, a.trunk ? a.trunk + ((size_t)n0 * Smax + (size_t)sample * N) * D : nullptr);
  __syncthreads();
  if (tid < D) {
    float s = a.w.vu2_b[tid];
    for (int j = 0; j < 2 * D; ++j) s += a.w.vu2_w[(size_t)j * D + tid] * vnv[j];
    gr[tid] = s;
  }
  // the attention pool's scores and the node head on the wave's own rows of trunk
  if (act) {
    const int NTP = lmx_gfm_pool_dim(D) >> 4;
    for (int which = 0; which < (a.node_pred ? 2 : 1); ++which) {
      const float* w1 = which ? a.w.nh1_w : a.w.pool1_w;
      const float* b1 = which ? a.w.nh1_b : a.w.pool1_b;
      const float* w2 = which ? a.w.nh2_w : a.w.pool2_w;
      const float b2 = which ? a.w.nh2_b[0] : a.w.pool2_b[0];
      f32x4 acc[4];
      zero<4>(acc);
      mma<4>(acc, ab, LD, w1, 0, NTD, NTP, 0, NTP, m, lane);
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        if (ni < NTP) {
          const int c = ni * 16 + r;
          const float b = b1[c], wv = w2[c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = acc[ni][e] + b;
            part[e] += wv * (which ? fmaxf(v, 0.f) : tanhf(v));
          }
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) part[e] += __shfl_xor(part[e], o, 64);
        const int t = m * 16 + 4 * g + e;
        if (r == 0) {
          if (!which)
            sc[t] = part[e] + b2;
          else if (t >= 1 && t <= N)
            a.node_pred[n0 + t - 1] = 1.0f / (1.0f + expf(-(part[e] + b2)));
        }
      }
    }
  }
  __syncthreads();
  if (tid < D) {
    float sum = 0.f, ss = 0.f;
    for (int c = 0; c < D; ++c) sum += gr[c];
    const float mean = sum / (float)D;
    for (int c = 0; c < D; ++c) ss += (gr[c] - mean) * (gr[c] - mean);
    const float y = (gr[tid] - mean) * (1.0f / sqrtf(ss / (float)D + 1e-5f)) * a.w.vu_g[tid] + a.w.vu_beta[tid];
    comb[D + tid] = y;
    if (a.vn) a.vn[(size_t)blockIdx.x * D + tid] = y;
  }
  if (tid >= 1 && tid <= N) {
    float mx = sc[1];
    for (int t = 2; t <= N; ++t) mx = fmaxf(mx, sc[t]);
    ew[tid] = expf(sc[tid] - mx);
  }
  __syncthreads();
  // mean | vn | sum_i a_i trunk[i], the sums over the nodes in ascending order
  if (tid < D) {
    float esum = 0.f, sum = 0.f, pool = 0.f;
    for (int t = 1; t <= N; ++t) esum += ew[t];
    for (int t = 1; t <= N; ++t) sum += ab[t * LD + tid];
    for (int t = 1; t <= N; ++t) pool += ew[t] / esum * ab[t * LD + tid];
    comb[tid] = sum / (float)N;
    comb[2 * D + tid] = pool;
  }
  __syncthreads();
  if (tid < D) {
    float s = a.w.comb_b[tid];
    for (int k = 0; k < 3 * D; ++k) s += a.w.comb_w[(size_t)k * D + tid] * comb[k];
    gr[tid] = fmaxf(s, 0.f);
  }
  __syncthreads();
  if (tid < D) {
    float sum = 0.f, ss = 0.f;
    for (int c = 0; c < D; ++c) sum += gr[c];
    const float mean = sum / (float)D;
    for (int c = 0; c < D; ++c) ss += (gr[c] - mean) * (gr[c] - mean);
    vnv[tid] = (gr[tid] - mean) * (1.0f / sqrtf(ss / (float)D + 1e-5f)) * a.w.comb_g[tid] + a.w.comb_beta[tid];
  }
  __syncthreads();
  if (tid < D / 2) {
    float s = a.w.ph1_b[tid];
    for (int c = 0; c < D; ++c) s += a.w.ph1_w[(size_t)c * (D / 2) + tid] * vnv[c];
    h1[tid] = keep(fmaxf(s, 0.f), 6 * L + 1, (uint64_t)tid);
  }
  __syncthreads();
  if (tid < D / 4) {
    float s = a.w.ph2_b[tid];
    for (int c = 0; c < D / 2; ++c) s += a.w.ph2_w[(size_t)c * (D / 4) + tid] * h1[c];
    h2[tid] = keep(fmaxf(s, 0.f), 6 * L + 2, (uint64_t)tid);
  }
  __syncthreads();
  if (tid == 0) {
    float z = a.w.ph3_b[0];
    for (int j = 0; j < D / 4; ++j) z += a.w.ph3_w[j] * h2[j];
    a.pred[blockIdx.x] = 1.0f / (1.0f + expf(-z));
  }
}

// seeds u64 [n] | node_off i32 [n + 1] | edge_off i32 [n + 1] | up to 16 bytes | bias f32 [H][cells]
inline int64_t bias_offset(int n) { return ((int64_t)n * 8 + (int64_t)(n + 1) * 8 + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t lmx_gfm_workspace_bytes(int n, int64_t cells, int n_heads) {
  return n > 0 && cells >= 0 && n_heads > 0 ? bias_offset(n) + cells * n_heads * 4 : 0;
}

extern "C" int lmx_k_gfm_forward(const lmx_gfm_weights_t* w, const lmx_gfm_graphs_t* gr, const uint64_t* seeds_host, int S, double p, float* pred,
                                 float* stats, float* node_pred, float* attn, float* trunk, float* vn, void* workspace, lmx_stream_t stream) {
  const char* who = "lmx_k_gfm_forward";
  LMX_TRY(lmx_gfm_check_config(who, w, true));
  int64_t nodes = 0, cells = 0;
  int max_n = 0;
  LMX_TRY(lmx_gfm_check_call(who, gr, S, p, node_pred != nullptr || attn != nullptr, &nodes, &cells, &max_n));
  const int n = gr->n;
  if (n == 0) return LMX_OK;
  LMX_REQUIRE(gr->deg_in && gr->deg_out && gr->idx && gr->win && (gr->edge_attr || gr->edge_off_host[n] == 0) && workspace, "%s: null pointer", who);
  LMX_REQUIRE(!gr->has_time || gr->timestamps, "%s: has_time without timestamps", who);
  LMX_REQUIRE(!attn || gr->target, "%s: attn_to_target without target", who);
  LMX_REQUIRE((((uintptr_t)gr->timestamps | (uintptr_t)gr->win | (uintptr_t)gr->edge_attr | (uintptr_t)gr->target) & 3) == 0 &&
                  ((uintptr_t)workspace & 15) == 0,
              "%s: misaligned pointer", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned grid = 0;
  int dev = -1;
  LMX_TRY(lmx_gait_launch_prologue(who, n, S, gr->x, pred, stats, {trunk, vn, node_pred, attn}, seeds_host, workspace, st, &grid, &dev));
  char* ws = static_cast<char*>(workspace);
  LMX_HIP(hipMemcpyAsync(ws + (size_t)n * 8, gr->node_off_host, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
  LMX_HIP(hipMemcpyAsync(ws + (size_t)n * 8 + (size_t)(n + 1) * 4, gr->edge_off_host, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
  GfmArgs a;
  a.w = *w;
  a.seeds = reinterpret_cast<const uint64_t*>(ws);
  a.node_off = reinterpret_cast<const int32_t*>(ws + (size_t)n * 8);
  a.edge_off = a.node_off + (n + 1);
  a.bias = reinterpret_cast<float*>(ws + bias_offset(n));
  a.x = gr->x;
  a.ts = gr->timestamps;
  a.has_time = gr->has_time;
  a.deg_in = gr->deg_in;
  a.deg_out = gr->deg_out;
  a.idx = gr->idx;
  a.win = gr->win;
  a.edge_attr = gr->edge_attr;
  a.target = gr->target;
  a.pred = pred;
  a.node_pred = node_pred;
  a.attn = attn;
  a.trunk = trunk;
  a.vn = vn;
  a.S = S;
  a.TP = (max_n + 1 + 15) / 16 * 16;
  const int dh = lmx_gfm_head_dim(*w);
  a.LDU = (3 * dh > 64 ? 3 * dh : 64) + 4;
  a.thr = S > 0 ? lmx_gait_threshold(p) : 0;
  a.scale = S > 0 ? lmx_gait_keep_scale(p) : 1.0f;
  a.cs = lmx_gfm_score_scale(dh);
  const int lds_bytes = lds_floats(a.TP, a.LDU) * (int)sizeof(float);
  constexpr int WANT = lds_floats((LMX_GFM_MAX_NODES + 1 + 15) / 16 * 16, 100) * (int)sizeof(float);
  static_assert(WANT <= LDS_LIMIT, "LMX_GFM_MAX_NODES: the tiles do not fit the LDS");
  LMX_REQUIRE(lds_bytes <= LDS_LIMIT, "%s: two tiles of %d x %d f32, one of %d x %d and the rest need %d bytes of LDS, a workgroup has %d", who, a.TP,
              LD, a.TP, a.LDU, lds_bytes, LDS_LIMIT);
  hipLaunchKernelGGL(gfm_bias_kernel, dim3((unsigned)n, (unsigned)((max_n * max_n + 255) / 256)), dim3(256), 0, st, a);
  LMX_TRY(lmx_launch_check("gfm_bias_kernel"));
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(&gfm_forward_kernel), WANT, dev));
  hipLaunchKernelGGL(gfm_forward_kernel, dim3(grid), dim3(NTH), lds_bytes, st, a);
  LMX_TRY(lmx_launch_check("gfm_forward_kernel"));
  return lmx_gait_stats_launch(pred, stats, n, S, st);
}
