// tcn.hip — the whole TCN gait model in one launch (include/lmx.h "The TCN gait model"; DESIGN.md "Gait model").
// One workgroup of 4 waves per (clip, sample).  Two activation tiles live in LDS, [TP][68] f32 each (TP = T rounded up to 16; 64
// channels + 4 floats of padding, so that the 16 rows a wave reads at once fall into 16 different bank groups), and the network walks
// between them: conv1 reads tile A and writes tile B, conv2 reads tile B, the residual reads tile A, and the block's output goes back to
// tile A once every wave has finished reading.  Nothing between the input series and the prediction touches HBM (but `trunk`, for tests).
// Each convolution is a GEMM of M = T, N = Cout, K = taps x Cin over SHIFTED rows of the tile, on the exact f32-input MFMA
// v_mfma_f32_16x16x4_f32: wave w owns the 16-row tiles w, w + 4, ... (MPW of them, the template parameter) and all Cout / 16 column
// tiles.  For one tap and one group of 16 input channels a lane reads ONE float4 of A from LDS (row t - shift, channels 16q + 4g .. +3,
// g = lane >> 4) and one float4 of B per column tile straight from the weights in L2, which lmx.native.write_tcn_image stored in exactly
// that order (gait.h): element e of both is the operand of MFMA e, whose four k are the channels 16q + 4g + e, g = 0 .. 3.
// Rows t >= T of the tiles hold finite values that never reach a row < T (the convolutions are causal) and never leave the LDS.
#include "gait_launch.h"
#include "tcn.h"

namespace {

constexpr int LD = 68;           // floats per tile row
constexpr int TAIL = 64 + 256 + 64;  // pooled | partial sums of the pool | hidden row of the head
constexpr int LDS_LIMIT = 160 * 1024;

struct TcnArgs {
  lmx_tcn_weights_t w;
  const float* x;
  const uint64_t* seeds;
  float *pred, *trunk;
  int T, S, MT;
  uint64_t thr;
  float scale;
};

template <int MPW>
__device__ __forceinline__ void conv_acc(f32x4 (&acc)[MPW][4], const float* src, const float* __restrict__ W, int taps, int d, int Q, int NT,
                                         int MT, int wave, int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the B operand of the NEXT (tap, group) is loaded from L2 while the MFMAs of this one run
  const f32x4* wp = reinterpret_cast<const f32x4*>(W) + lane;
  const f32x4* const wlast = wp + (size_t)(taps * Q - 1) * NT * 64;
  f32x4 b[4], bn[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) b[ni] = ni < NT ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < taps; ++j) {
    const int shift = (taps - 1 - j) * d;
    for (int q = 0; q < Q; ++q) {
      if (wp != wlast) wp += NT * 64;  // the last step loads its own operand again
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) bn[ni] = ni < NT ? wp[ni * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mi = 0; mi < MPW; ++mi) {
        const int m = wave + 4 * mi;
        if (m < MT) {
          const int t = m * 16 + r - shift;
          const f32x4 a = t >= 0 ? *reinterpret_cast<const f32x4*>(src + t * LD + 16 * q + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
          // e outside: consecutive MFMAs go to different accumulators (a dependent one waits 40 cycles, an independent one 32)
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              if (ni < NT) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[ni][e], acc[mi][ni], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) b[ni] = bn[ni];
    }
  }
}

template <int MPW>
__global__ __launch_bounds__(256) void tcn_forward_kernel(const TcnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = a.T, MT = a.MT, TP = MT * 16;
  float* bufA = lds;
  float* bufB = lds + TP * LD;
  float* pooled = lds + 2 * TP * LD;
  float* part = pooled + 64;
  float* hid = part + 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Smax = a.S > 0 ? a.S : 1, clip = blockIdx.x / Smax, sample = blockIdx.x % Smax;
  const int F = a.w.input_dim, nb = a.w.n_blocks;
  const bool drop = a.S > 0;
  const uint64_t seed = drop ? a.seeds[clip] : 0, n_sites = 2 * nb + 1, stream0 = (uint64_t)sample * n_sites;

  // the series into tile A: rows >= T and channels >= input_dim are zeros
  const float* x = a.x + (size_t)clip * T * F;
  for (int i = tid; i < TP * 64; i += 256) {
    const int t = i >> 6, c = i & 63;
    bufA[t * LD + c] = (t < T && c < F) ? x[t * F + c] : 0.f;
  }
  __syncthreads();

  f32x4 acc[MPW][4], res[MPW][4];
  for (int blk = 0; blk < nb; ++blk) {
    const int cin = blk ? a.w.channels[blk - 1] : F, cout = a.w.channels[blk], d = 1 << blk, NT = cout >> 4;
    // conv1: tile A -> bias, ReLU, dropout site 2 blk -> tile B
    conv_acc<MPW>(acc, bufA, a.w.conv_w[blk][0], a.w.k, d, (cin + 15) >> 4, NT, MT, wave, lane);
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + 4 * mi;
      if (m < MT) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < NT) {
            const int c = ni * 16 + r;
            const float bias = a.w.conv_b[blk][0][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              float v = fmaxf(acc[mi][ni][e] + bias, 0.f);
              if (drop && t < T) v = lmx_gait_keep(seed, stream0 + 2 * blk, (uint64_t)(c * T + t), a.thr) ? v * a.scale : 0.f;
              bufB[t * LD + c] = v;
            }
          }
      }
    }
    __syncthreads();
    // conv2: tile B -> bias, ReLU, dropout site 2 blk + 1, in registers
    conv_acc<MPW>(acc, bufB, a.w.conv_w[blk][1], a.w.k, d, cout >> 4, NT, MT, wave, lane);
    const bool has_res = a.w.res_w[blk] != nullptr;
    if (has_res) conv_acc<MPW>(res, bufA, a.w.res_w[blk], 1, 1, (cin + 15) >> 4, NT, MT, wave, lane);
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + 4 * mi;
      if (m < MT) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < NT) {
            const int c = ni * 16 + r;
            const float bias = a.w.conv_b[blk][1][c], rbias = has_res ? a.w.res_b[blk][c] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              float v = fmaxf(acc[mi][ni][e] + bias, 0.f);
              if (drop && t < T) v = lmx_gait_keep(seed, stream0 + 2 * blk + 1, (uint64_t)(c * T + t), a.thr) ? v * a.scale : 0.f;
              const float xr = has_res ? res[mi][ni][e] + rbias : bufA[t * LD + c];
              acc[mi][ni][e] = fmaxf(v + xr, 0.f);
            }
          }
      }
    }
    __syncthreads();  // every wave has read what it needs of tiles A and B
    float* trunk = (a.trunk && blk == nb - 1) ? a.trunk + (size_t)blockIdx.x * T * cout : nullptr;
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const int m = wave + 4 * mi;
      if (m < MT) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          if (ni < NT) {
            const int c = ni * 16 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int t = m * 16 + 4 * g + e;
              bufA[t * LD + c] = acc[mi][ni][e];
              if (trunk && t < T) trunk[(size_t)t * cout + c] = acc[mi][ni][e];
            }
          }
      }
    }
    __syncthreads();
  }

  // The head.  Thread j < head fetches row j of fc1 and its fc2 weight BEFORE the pool, so their latency hides under it.
  const int C = a.w.channels[nb - 1], H = a.w.head;
  f32x4 w1[16];
  float b1 = 0.f, w2 = 0.f;
  if (tid < H) {
    const f32x4* wr = reinterpret_cast<const f32x4*>(a.w.fc1_w + tid * C);
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) w1[c4] = c4 < (C >> 2) ? wr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    b1 = a.w.fc1_b[tid];
    w2 = a.w.fc2_w[tid];
  }
  // mean over the T real steps: four partial sums per channel (t = p, p + 4, ...), joined in a fixed order
  {
    const int c = tid & 63, p = tid >> 6;
    float s = 0.f;
    for (int t = p; t < T; t += 4) s += bufA[t * LD + c];
    part[p * 64 + c] = s;
  }
  __syncthreads();
  if (tid < 64) pooled[tid] = (((part[tid] + part[64 + tid]) + part[128 + tid]) + part[192 + tid]) / (float)T;
  __syncthreads();
  if (tid < H) {
    float s = b1;
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4)
      if (c4 < (C >> 2)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s += w1[c4][e] * pooled[4 * c4 + e];
      }
    s = fmaxf(s, 0.f);
    if (drop) s = lmx_gait_keep(seed, stream0 + 2 * nb, (uint64_t)tid, a.thr) ? s * a.scale : 0.f;
    hid[tid] = w2 * s;  // the product of the second linear; thread 0 adds them in order
  }
  __syncthreads();
  if (tid == 0) {
    float z = a.w.fc2_b[0];
    for (int j = 0; j < H; ++j) z += hid[j];
    a.pred[blockIdx.x] = 1.0f / (1.0f + expf(-z));  // the accurate expf
  }
}

// stats[i] = {mean, unbiased standard deviation} of row i of pred, read in sample order: one thread per clip
__global__ void tcn_stats_kernel(const float* __restrict__ pred, float* __restrict__ stats, int n, int S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (S == 0) {
    stats[2 * i] = pred[i];
    stats[2 * i + 1] = 0.f;
    return;
  }
  const float* row = pred + (size_t)i * S;
  float sum = 0.f, ss = 0.f;
  for (int s = 0; s < S; ++s) sum += row[s];
  const float mean = sum / (float)S;
  for (int s = 0; s < S; ++s) ss += (row[s] - mean) * (row[s] - mean);
  stats[2 * i] = mean;
  stats[2 * i + 1] = sqrtf(ss / (float)(S - 1));
}

template <int MPW>
int launch(const TcnArgs& a, unsigned grid, int lds_bytes, int dev, hipStream_t st) {
  // the limit is raised once per (kernel, device): to what the largest T of this instantiation needs
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(&tcn_forward_kernel<MPW>), (2 * MPW * 64 * LD + TAIL) * (int)sizeof(float), dev));
  hipLaunchKernelGGL(tcn_forward_kernel<MPW>, dim3(grid), dim3(256), lds_bytes, st, a);
  return lmx_launch_check("tcn_forward_kernel");
}

}  // namespace

// gait_launch.h: the stats kernel on `st`; the gait transformer (xfm.hip) writes its stats with it too
int lmx_gait_stats_launch(const float* pred, float* stats, int n, int S, hipStream_t st) {
  hipLaunchKernelGGL(tcn_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pred, stats, n, S);
  return lmx_launch_check("tcn_stats_kernel");
}

extern "C" int64_t lmx_tcn_workspace_bytes(int n) { return lmx_gait_workspace_bytes(n); }

extern "C" int lmx_k_tcn_forward(const lmx_tcn_weights_t* w, const float* x, const uint64_t* seeds_host, int n, int T, int S, double p, float* pred,
                                 float* stats, float* trunk, void* workspace, lmx_stream_t stream) {
  LMX_TRY(lmx_tcn_check_config("lmx_k_tcn_forward", w, true));
  LMX_TRY(lmx_tcn_check_call("lmx_k_tcn_forward", n, T, S, p));
  if (n == 0) return LMX_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned grid = 0;
  int dev = -1;
  LMX_TRY(lmx_gait_launch_prologue("lmx_k_tcn_forward", n, S, x, pred, stats, {trunk}, seeds_host, workspace, st, &grid, &dev));
  TcnArgs a;
  a.w = *w;
  a.x = x;
  a.seeds = static_cast<const uint64_t*>(workspace);
  a.pred = pred;
  a.trunk = trunk;
  a.T = T;
  a.S = S;
  a.MT = (T + 15) / 16;
  a.thr = S > 0 ? lmx_gait_threshold(p) : 0;
  a.scale = S > 0 ? lmx_gait_keep_scale(p) : 1.0f;
  const int lds_bytes = (2 * a.MT * 16 * LD + TAIL) * (int)sizeof(float);
  LMX_REQUIRE(lds_bytes <= LDS_LIMIT, "lmx_k_tcn_forward: two tiles of %d x %d f32 and the head need %d bytes of LDS, a workgroup has %d",
              a.MT * 16, LD, lds_bytes, LDS_LIMIT);
  if (a.MT <= 4)
    LMX_TRY(launch<1>(a, grid, lds_bytes, dev, st));
  else if (a.MT <= 8)
    LMX_TRY(launch<2>(a, grid, lds_bytes, dev, st));
  else
    LMX_TRY(launch<4>(a, grid, lds_bytes, dev, st));
  return lmx_gait_stats_launch(pred, stats, n, S, st);
}
