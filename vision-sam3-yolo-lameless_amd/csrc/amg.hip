// amg.hip — the scoring step of segment_anything's SamAutomaticMaskGenerator._process_batch without the full-resolution
// masks: calculate_stability_score + (masks > thr) + batched_mask_to_box on Sam.postprocess_masks' output, computed straight
// from the LxL low-res logits.  No output pixel is written; each workgroup reduces its counts and box in registers, across
// the wave and through LDS, then issues one atomic per counter (per workgroup, not per pixel).
//
// Compiled with -ffp-contract=off (csrc/Makefile EXACT): the value v at every output pixel is the f32 value
// lmx_k_mask_logits stores there, bit for bit — the same bil_idx / sample_mid sequence, no FMA contraction.
//
// Two kernels, one arithmetic:
//   mask_score_staged_kernel : the output is an upsampling of the cropped TxT intermediate (nh <= h and nw <= w, every
//       frame at least as large as the resized input, 1080p among them).  A workgroup takes tiles of TY x TX output pixels;
//       it evaluates the <= (TY+2) x (TX+2) intermediate values under a tile once (sample_mid, 4 low-res taps each) into LDS,
//       then every pixel blends its four LDS taps.  In lmx_k_mask_logits every pixel evaluates sample_mid 4x (16 taps).
//   mask_score_direct_kernel : any other geometry (a frame smaller than the resized input, where the intermediate has more
//       values than the output): lmx_k_mask_logits' per-pixel evaluation.
#include "common.h"

namespace {

constexpr int TY = 16, TX = 256;           // output tile of the staged kernel (256 threads: one column each, TY rows)
constexpr int MR = TY + 4, MC = TX + 8;    // LDS intermediate tile: <= TY + 2 rows / TX + 2 columns are needed when sy, sx <= 1

struct Acc {
  unsigned hi = 0, lo = 0, area = 0;
  int minx = 0x7fffffff, miny = 0x7fffffff, maxx = -1, maxy = -1;
  __device__ __forceinline__ void add(float v, float t_hi, float t_lo, float t, int x, int y) {
    hi += v > t_hi ? 1u : 0u;
    lo += v > t_lo ? 1u : 0u;
    if (v > t) {
      ++area;
      minx = x < minx ? x : minx;
      maxx = x > maxx ? x : maxx;
      miny = y < miny ? y : miny;
      maxy = y > maxy ? y : maxy;
    }
  }
};

// wave reduction, then across the workgroup's 4 waves through LDS, then ONE atomic per counter for the workgroup
__device__ __forceinline__ void flush(Acc a, long long* __restrict__ o) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    a.hi += __shfl_xor(a.hi, s, 64);
    a.lo += __shfl_xor(a.lo, s, 64);
    a.area += __shfl_xor(a.area, s, 64);
    const int b1 = __shfl_xor(a.minx, s, 64), b2 = __shfl_xor(a.miny, s, 64), b3 = __shfl_xor(a.maxx, s, 64),
              b4 = __shfl_xor(a.maxy, s, 64);
    a.minx = b1 < a.minx ? b1 : a.minx;
    a.miny = b2 < a.miny ? b2 : a.miny;
    a.maxx = b3 > a.maxx ? b3 : a.maxx;
    a.maxy = b4 > a.maxy ? b4 : a.maxy;
  }
  __shared__ unsigned red_c[4][3];
  __shared__ int red_b[4][4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red_c[wv][0] = a.hi;
    red_c[wv][1] = a.lo;
    red_c[wv][2] = a.area;
    red_b[wv][0] = a.minx;
    red_b[wv][1] = a.miny;
    red_b[wv][2] = a.maxx;
    red_b[wv][3] = a.maxy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      a.hi += red_c[k][0];
      a.lo += red_c[k][1];
      a.area += red_c[k][2];
      a.minx = red_b[k][0] < a.minx ? red_b[k][0] : a.minx;
      a.miny = red_b[k][1] < a.miny ? red_b[k][1] : a.miny;
      a.maxx = red_b[k][2] > a.maxx ? red_b[k][2] : a.maxx;
      a.maxy = red_b[k][3] > a.maxy ? red_b[k][3] : a.maxy;
    }
    unsigned long long* u = reinterpret_cast<unsigned long long*>(o);
    if (a.hi) atomicAdd(&u[0], (unsigned long long)a.hi);
    if (a.lo) atomicAdd(&u[1], (unsigned long long)a.lo);
    if (a.area) {
      atomicAdd(&u[2], (unsigned long long)a.area);
      atomicMin(&o[3], (long long)a.minx);
      atomicMin(&o[4], (long long)a.miny);
      atomicMax(&o[5], (long long)a.maxx);
      atomicMax(&o[6], (long long)a.maxy);
    }
  }
}

__global__ __launch_bounds__(256) void mask_score_staged_kernel(const float* __restrict__ logits, const int32_t* __restrict__ idx, int L,
                                                                int T, int nh, int nw, int h, int w, float t_hi, float t_lo, float t,
                                                                long long* __restrict__ out) {
  __shared__ float mid[MR * MC];
  const int b = idx ? idx[blockIdx.y] : (int)blockIdx.y;
  const float* lg = logits + (int64_t)b * L * L;
  const float sLT = (float)L / (float)T;
  const float sy = (float)nh / (float)h, sx = (float)nw / (float)w;
  const int tiles_x = (w + TX - 1) / TX, tiles = tiles_x * ((h + TY - 1) / TY);
  const int tid = threadIdx.x;
  Acc acc;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ya = (tile / tiles_x) * TY, xa = (tile % tiles_x) * TX;
    const int yb = ya + TY < h ? ya + TY : h, xb = xa + TX < w ? xa + TX : w;
    int Ylo, Yhi, Xlo, Xhi, dummy;
    float fd;
    bil_idx(sy, ya, nh, Ylo, dummy, fd);
    bil_idx(sy, yb - 1, nh, dummy, Yhi, fd);
    bil_idx(sx, xa, nw, Xlo, dummy, fd);
    bil_idx(sx, xb - 1, nw, dummy, Xhi, fd);
    const int rows = Yhi - Ylo + 1, cols = Xhi - Xlo + 1;
    // sy, sx <= 1 (checked by the launcher) bound rows / cols by TY + 2 / TX + 2; `fits` keeps any rounding surprise exact
    const bool fits = rows <= MR && cols <= MC;
    if (fits)
      for (int k = tid; k < rows * cols; k += 256) mid[k] = sample_mid(lg, L, T, sLT, Ylo + k / cols, Xlo + k % cols);
    __syncthreads();
    const int x = xa + tid;
    if (x < xb) {
      int X0, X1;
      float lx;
      bil_idx(sx, x, nw, X0, X1, lx);
      for (int y = ya; y < yb; ++y) {
        int Y0, Y1;
        float ly;
        bil_idx(sy, y, nh, Y0, Y1, ly);
        float a00, a01, a10, a11;
        if (fits) {
          a00 = mid[(Y0 - Ylo) * cols + (X0 - Xlo)];
          a01 = mid[(Y0 - Ylo) * cols + (X1 - Xlo)];
          a10 = mid[(Y1 - Ylo) * cols + (X0 - Xlo)];
          a11 = mid[(Y1 - Ylo) * cols + (X1 - Xlo)];
        } else {
          a00 = sample_mid(lg, L, T, sLT, Y0, X0);
          a01 = sample_mid(lg, L, T, sLT, Y0, X1);
          a10 = sample_mid(lg, L, T, sLT, Y1, X0);
          a11 = sample_mid(lg, L, T, sLT, Y1, X1);
        }
        const float t0 = (1.f - lx) * a00 + lx * a01;
        const float t1 = (1.f - lx) * a10 + lx * a11;
        const float v = (1.f - ly) * t0 + ly * t1;
        acc.add(v, t_hi, t_lo, t, x, y);
      }
    }
    __syncthreads();  // the next tile overwrites `mid`
  }
  flush(acc, out + (int64_t)blockIdx.y * 8);
}

__global__ __launch_bounds__(256) void mask_score_direct_kernel(const float* __restrict__ logits, const int32_t* __restrict__ idx, int L,
                                                                int T, int nh, int nw, int h, int w, float t_hi, float t_lo, float t,
                                                                long long* __restrict__ out) {
  const int b = idx ? idx[blockIdx.y] : (int)blockIdx.y;
  const float* lg = logits + (int64_t)b * L * L;
  const float sLT = (float)L / (float)T;
  const float sy = (float)nh / (float)h, sx = (float)nw / (float)w;
  const int total = h * w;  // < 2^31 (checked by the launcher)
  Acc acc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / w, x = i - y * w;
    int Y0, Y1, X0, X1;
    float ly, lx;
    bil_idx(sy, y, nh, Y0, Y1, ly);
    bil_idx(sx, x, nw, X0, X1, lx);
    const float a00 = sample_mid(lg, L, T, sLT, Y0, X0), a01 = sample_mid(lg, L, T, sLT, Y0, X1);
    const float a10 = sample_mid(lg, L, T, sLT, Y1, X0), a11 = sample_mid(lg, L, T, sLT, Y1, X1);
    const float t0 = (1.f - lx) * a00 + lx * a01;
    const float t1 = (1.f - lx) * a10 + lx * a11;
    const float v = (1.f - ly) * t0 + ly * t1;
    acc.add(v, t_hi, t_lo, t, x, y);
  }
  flush(acc, out + (int64_t)blockIdx.y * 8);
}

__global__ void mask_score_init_kernel(long long* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 8) return;
  const int f = i & 7;
  out[i] = (f == 3 || f == 4) ? 0x7fffffffll : ((f == 5 || f == 6) ? -1ll : 0ll);
}

// batched_mask_to_box's convention: an empty mask has the box [0, 0, 0, 0]
__global__ void mask_score_empty_box_kernel(long long* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long* o = out + (int64_t)i * 8;
  if (o[2] == 0) o[3] = o[4] = o[5] = o[6] = 0;
}

}  // namespace

extern "C" int lmx_k_mask_score(const float* logits, int n, int L, int T, int nh, int nw, int h, int w, double thr, double off,
                                const int32_t* idx, int64_t* out, lmx_stream_t stream) {
  LMX_REQUIRE(logits && out, "lmx_k_mask_score: null pointer");
  LMX_REQUIRE(n > 0 && L > 0 && T >= L && nh > 0 && nw > 0 && nh <= T && nw <= T && h > 0 && w > 0 &&
                  (int64_t)h * w < 0x7fffffffll - 256 * 256 && n <= 65535, "lmx_k_mask_score: geometry");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long long* o = reinterpret_cast<long long*>(out);
  // the thresholds as torch compares an f32 tensor with a Python float: the double sum, rounded to f32
  const float t_hi = (float)(thr + off), t_lo = (float)(thr - off), t = (float)thr;
  hipLaunchKernelGGL(mask_score_init_kernel, dim3((n * 8 + 255) / 256), dim3(256), 0, st, o, n);
  if (nh <= h && nw <= w) {
    const int tiles = ((w + TX - 1) / TX) * ((h + TY - 1) / TY);
    const int gx = tiles < 32 ? tiles : 32;
    hipLaunchKernelGGL(mask_score_staged_kernel, dim3(gx, n), dim3(256), 0, st, logits, idx, L, T, nh, nw, h, w, t_hi, t_lo, t, o);
  } else {
    int gx = (int)(((int64_t)h * w + 255) / 256);
    if (gx > 32) gx = 32;
    hipLaunchKernelGGL(mask_score_direct_kernel, dim3(gx, n), dim3(256), 0, st, logits, idx, L, T, nh, nw, h, w, t_hi, t_lo, t, o);
  }
  int rc = lmx_launch_check("mask_score_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mask_score_empty_box_kernel, dim3((n + 255) / 256), dim3(256), 0, st, o, n);
  return lmx_launch_check("mask_score_empty_box_kernel");
}
