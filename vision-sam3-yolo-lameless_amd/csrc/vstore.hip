// vstore.hip — the vector store's kernels: cosine top-k of unit query rows over a gallery of unit rows in HBM (lmx_k_cosine_topk) and
// raw rows -> f32 unit rows (lmx_k_unit_rows).  The arithmetic is the text at lmx_k_cosine_topk in include/lmx.h and
// csrc/host_vstore.cpp restates it; this file is held to that twin bit for bit (tests/test_gpu_vstore.py).
//
// scan_kernel<T>: one wave per gallery row, LMX_VSTORE_ROWS_PER_WAVE rows in flight per wave, lane l holds partials 4l .. 4l+3 of the
//   pinned dot product for each of the T queries of its tile (the tile's rows wait in LDS).  The T x rows x 4 partials of a lane are
//   reduced across lanes by ONE transposing butterfly (lane_tree: each xor step hands half of the values to the partner, so a step costs
//   half as many cross-lane moves as the one before) in the pinned order 32, 16, .. 1, then the four partials of a row meet.  Every wave
//   keeps its running top-k per query with rank j in lane j; almost every row fails one scalar compare against rank k - 1.  The waves'
//   lists meet in LDS, the workgroup's list goes to the workspace.
// merge_kernel: one workgroup per query merges the workgroups' lists and writes the result.
// No atomics; (score, slot) pairs are totally ordered, so no choice of grid, tile or wave can show in a result.
#include <limits.h>

#include "common.h"
#include "vstore.h"

namespace {

constexpr int WAVES = LMX_VSTORE_WAVES, RPW = LMX_VSTORE_ROWS_PER_WAVE, ROWS = LMX_VSTORE_ROWS;
constexpr int MERGE_WAVES = 16;
constexpr int EMPTY = INT_MAX;  // the slot of a rank nothing has taken yet (its score: -inf); no row has it, N <= 2^31 - 1

// descending score, compared as float values; exact ties to the lower slot
__device__ __forceinline__ bool better(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

__device__ __forceinline__ float lane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// a wave's sorted list, rank j in lane j; (ts, ti) is rank k - 1, the same in every lane.  The candidate is the same in every lane
__device__ __forceinline__ void list_insert(float& ls, int& li, float& ts, int& ti, float cs, int ci, int k, int lane) {
  const float ps = __shfl_up(ls, 1, 64);
  const int pi = __shfl_up(li, 1, 64);
  if (better(cs, ci, ls, li)) {
    const bool here = lane == 0 || !better(cs, ci, ps, pi);
    ls = here ? cs : ps;
    li = here ? ci : pi;
  }
  ts = lane_f(ls, k - 1);
  ti = lane_i(li, k - 1);
}

// `count` candidates at p (LDS or global, any order) into the list
__device__ __forceinline__ void list_merge(float& ls, int& li, float& ts, int& ti, const uint2* p, int count, int k, int lane) {
  for (int b = 0; b < count; b += 256) {
    uint2 c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = b + 64 * u + lane;
      c[u] = e < count ? p[e] : uint2{0u, (unsigned)EMPTY};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float cs = __uint_as_float(c[u].x);
      const int ci = (int)c[u].y;
      unsigned long long m = __ballot(ci != EMPTY && better(cs, ci, ts, ti));
      while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float s = lane_f(cs, j);
        const int i = lane_i(ci, j);
        if (better(s, i, ts, ti)) list_insert(ls, li, ts, ti, s, i, k, lane);
      }
    }
  }
}

// The cross-lane part of the pinned sum for N values per lane at once: step O adds lane l ^ O's value to lane l's, O = 32, 16, .. 1.
// While more than one value is left a step keeps the half of them whose top index bit is the lane's bit O and hands over the other
// half, so value i ends in the lanes whose top bits spell i.  a + b == b + a bit for bit, so whichever lane adds, the sum is the pin's.
template <int N, int O>
struct LaneTree {
  static __device__ __forceinline__ float run(const float* v, int lane) {
    if constexpr (O == 0) {
      return v[0];
    } else if constexpr (N > 1) {
      const bool hi = (lane & O) != 0;
      float nv[N / 2];
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        const float keep = hi ? v[i + N / 2] : v[i];
        const float send = hi ? v[i] : v[i + N / 2];
        nv[i] = keep + __shfl_xor(send, O, 64);
      }
      return LaneTree<N / 2, O / 2>::run(nv, lane);
    } else {
      const float nv[1] = {v[0] + __shfl_xor(v[0], O, 64)};
      return LaneTree<1, O / 2>::run(nv, lane);
    }
  }
};

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

template <int T>
__global__ __launch_bounds__(WAVES * 64) void scan_kernel(const float* __restrict__ gallery, int64_t ldg, int N, int D,
                                                         const float* __restrict__ queries, int Q, const int32_t* __restrict__ limits, int k,
                                                         uint2* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);  // [T][Dp], zero past D
  const int nbf = D / 256, Dp = (D + 255) / 256 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * T;

  for (int e = tid * 4; e < T * Dp; e += WAVES * 64 * 4) {
    const int q = e / Dp, d = e - q * Dp;
    const int qq = q0 + q < Q ? q0 + q : Q - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (d < D) v = *reinterpret_cast<const f32x4*>(queries + (int64_t)qq * D + d);
    *reinterpret_cast<f32x4*>(qs + e) = v;
  }
  int lim[T], nmax = 0;
#pragma unroll
  for (int q = 0; q < T; ++q) {
    int l = 0;
    if (q0 + q < Q) {
      l = limits ? limits[q0 + q] : N;
      l = l < 0 ? 0 : (l > N ? N : l);
    }
    lim[q] = __builtin_amdgcn_readfirstlane(l);
    nmax = lim[q] > nmax ? lim[q] : nmax;
  }
  __syncthreads();

  float ls[T], ts[T];
  int li[T], ti[T];
#pragma unroll
  for (int q = 0; q < T; ++q) ls[q] = ts[q] = -INFINITY, li[q] = ti[q] = EMPTY;

  constexpr int V = RPW * T * 4, SH = 6 - ilog2(V);
  static_assert(V <= 64 && (V & (V - 1)) == 0, "one value per lane at the most, a power of two");
  const bool tail = Dp != D && nbf * 256 + lane * 4 < D;
  for (int64_t base = (int64_t)blockIdx.x * ROWS + wave * RPW; base < nmax; base += (int64_t)gridDim.x * ROWS) {
    const float* gp[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int64_t row = base + r < nmax ? base + r : nmax - 1;  // a row past the end repeats the last one and is not ranked
      gp[r] = gallery + row * ldg + lane * 4;
    }
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int b0 = 0; b0 < nbf; b0 += 4) {
      f32x4 g[4][RPW];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b0 + u < nbf) {
#pragma unroll
          for (int r = 0; r < RPW; ++r) g[u][r] = *reinterpret_cast<const f32x4*>(gp[r] + (b0 + u) * 256);
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b0 + u < nbf) {
#pragma unroll
          for (int q = 0; q < T; ++q) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(qs + q * Dp + (b0 + u) * 256 + lane * 4);
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[(r * T + q) * 4 + c] = fmaf(g[u][r][c], qv[c], acc[(r * T + q) * 4 + c]);
          }
        }
    }
    if (Dp != D) {  // the last, partial block of 256: elements past D contribute nothing
      f32x4 g[RPW];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        g[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (tail) g[r] = *reinterpret_cast<const f32x4*>(gp[r] + nbf * 256);
      }
#pragma unroll
      for (int q = 0; q < T; ++q) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qs + q * Dp + nbf * 256 + lane * 4);
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float f = fmaf(g[r][c], qv[c], acc[(r * T + q) * 4 + c]);
            acc[(r * T + q) * 4 + c] = tail ? f : acc[(r * T + q) * 4 + c];
          }
      }
    }
    // value i = (r * T + q) * 4 + c now sits in the lanes l with l >> SH == i; the four partials of a row meet last: w = 2, then w = 1
    float t = LaneTree<V, 32>::run(acc, lane);
    t = t + __shfl_xor(t, 2 << SH, 64);
    t = t + __shfl_xor(t, 1 << SH, 64);
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int q = 0; q < T; ++q) {
        const float s = lane_f(t, ((r * T + q) * 4) << SH);
        const int64_t row = base + r;
        if (row < lim[q] && better(s, (int)row, ts[q], ti[q])) list_insert(ls[q], li[q], ts[q], ti[q], s, (int)row, k, lane);
      }
  }

  // the waves' lists meet in LDS (the queries are done with): [T][WAVES][k]
  __syncthreads();
  uint2* lists = reinterpret_cast<uint2*>(smem);
#pragma unroll
  for (int q = 0; q < T; ++q)
    if (lane < k) lists[(q * WAVES + wave) * k + lane] = uint2{__float_as_uint(ls[q]), (unsigned)li[q]};
  __syncthreads();
  for (int q = wave; q < T && q0 + q < Q; q += WAVES) {
    float ms = -INFINITY, mts = -INFINITY;
    int mi = EMPTY, mti = EMPTY;
    list_merge(ms, mi, mts, mti, lists + q * WAVES * k, WAVES * k, k, lane);
    if (lane < k) ws[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * k + lane] = uint2{__float_as_uint(ms), (unsigned)mi};
  }
}

// ws: [Q][G][k]; ranks nothing took: slot -1, score 0
__global__ __launch_bounds__(MERGE_WAVES * 64) void merge_kernel(const uint2* __restrict__ ws, int G, int k, float* __restrict__ scores,
                                                                int32_t* __restrict__ slots) {
  __shared__ uint2 lists[MERGE_WAVES * LMX_VSTORE_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = blockIdx.x;
  const int count = G * k, part = ((count + MERGE_WAVES - 1) / MERGE_WAVES + 63) / 64 * 64;
  float ls = -INFINITY, ts = -INFINITY;
  int li = EMPTY, ti = EMPTY;
  const int at = wave * part, n = count - at < part ? count - at : part;
  if (n > 0) list_merge(ls, li, ts, ti, ws + (int64_t)q * count + at, n, k, lane);
  if (lane < k) lists[wave * k + lane] = uint2{__float_as_uint(ls), (unsigned)li};
  __syncthreads();
  if (wave == 0) {
    ls = ts = -INFINITY, li = ti = EMPTY;
    list_merge(ls, li, ts, ti, lists, MERGE_WAVES * k, k, lane);
    if (lane < k) {
      scores[(int64_t)q * k + lane] = li == EMPTY ? 0.f : ls;
      slots[(int64_t)q * k + lane] = li == EMPTY ? -1 : li;
    }
  }
}

// one wave per row: the sum of squares in double in the pinned 256-partial order, then (float)((double)x / (sqrt(ss) + 1e-8))
template <class X>
__global__ __launch_bounds__(256) void unit_rows_kernel(const X* __restrict__ raw, int64_t n, int D, float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const X* x = raw + row * D;
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  for (int d = lane * 4; d < D; d += 256)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double v = (double)x[d + c];
      p[c] = fma(v, v, p[c]);
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] = p[c] + __shfl_xor(p[c], o, 64);
  p[0] = p[0] + p[2];
  p[1] = p[1] + p[3];
  const double den = sqrt(p[0] + p[1]) + 1e-8;
  for (int d = lane * 4; d < D; d += 256)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[row * ldo + d + c] = (float)((double)x[d + c] / den);
}

template <int T>
int launch_scan(const float* gallery, int64_t ldg, int N, int D, const float* queries, int Q, const int32_t* limits, int k, uint2* ws, unsigned G,
                hipStream_t st) {
  const int Dp = (D + 255) / 256 * 256;
  const size_t q_bytes = (size_t)T * Dp * 4, l_bytes = (size_t)T * WAVES * k * 8;
  const dim3 grid(G, (unsigned)((Q + T - 1) / T));
  hipLaunchKernelGGL(scan_kernel<T>, grid, dim3(WAVES * 64), q_bytes > l_bytes ? q_bytes : l_bytes, st, gallery, ldg, N, D, queries, Q, limits, k, ws);
  return lmx_launch_check("vstore scan_kernel");
}

}  // namespace

extern "C" int lmx_k_cosine_topk(const float* gallery, int64_t N, int D, int64_t ldg, const float* queries, int Q, const int32_t* limits, int k,
                                 float* scores, int32_t* slots, void* workspace, lmx_stream_t stream) {
  LMX_TRY(lmx_vstore_check_topk("lmx_k_cosine_topk", gallery, N, D, ldg, queries, Q, k, scores, slots));
  if (Q == 0) return LMX_OK;
  LMX_REQUIRE(N == 0 || workspace != nullptr, "lmx_k_cosine_topk: null workspace (lmx_h_cosine_topk_workspace bytes)");
  hipStream_t st = (hipStream_t)stream;
  int dev = -1;
  LMX_TRY(lmx_stream_device(st, &dev));
  const int cus = lmx_cu_count(dev);
  if (cus < 0) return cus;
  int64_t G = lmx_vstore_lists(N);
  if (G > (int64_t)cus * LMX_VSTORE_WG_PER_CU) G = (int64_t)cus * LMX_VSTORE_WG_PER_CU;
  uint2* ws = reinterpret_cast<uint2*>(workspace);
  if (G > 0) {
    const int tile = lmx_vstore_tile(D), T = Q < tile ? Q : tile;
    if (T <= 1)
      LMX_TRY(launch_scan<1>(gallery, ldg, (int)N, D, queries, Q, limits, k, ws, (unsigned)G, st));
    else if (T <= 2)
      LMX_TRY(launch_scan<2>(gallery, ldg, (int)N, D, queries, Q, limits, k, ws, (unsigned)G, st));
    else if (T <= 4)
      LMX_TRY(launch_scan<4>(gallery, ldg, (int)N, D, queries, Q, limits, k, ws, (unsigned)G, st));
    else
      LMX_TRY(launch_scan<8>(gallery, ldg, (int)N, D, queries, Q, limits, k, ws, (unsigned)G, st));
  }
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)Q), dim3(MERGE_WAVES * 64), 0, st, ws, (int)G, k, scores, slots);
  return lmx_launch_check("vstore merge_kernel");
}

extern "C" int lmx_k_unit_rows(const void* raw, int dtype, int64_t n, int D, float* out, int64_t ldo, lmx_stream_t stream) {
  LMX_TRY(lmx_vstore_check_unit("lmx_k_unit_rows", raw, dtype, n, D, out, ldo));
  if (n == 0) return LMX_OK;
  const dim3 grid((unsigned)((n + 3) / 4));
  if (dtype == LMX_VSTORE_F64)
    hipLaunchKernelGGL(unit_rows_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)raw, n, D, out, ldo);
  else
    hipLaunchKernelGGL(unit_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)raw, n, D, out, ldo);
  return lmx_launch_check("vstore unit_rows_kernel");
}
