// pre.hip — frame preprocessing (K9/K21): Pillow-exact separable u8 resampling and the crop/normalise/patchify
// pass that writes the ViT patch matrix.  HBM-bound byte work: a 1080p BGR frame is 6.2 MB in, the outputs are
// small, so the figure of merit is input bytes / time.  Plus the float path of DINOv3ViTImageProcessor
// (rescale -> float32 antialiased resize -> normalize) as one kernel that writes the same patch matrix.
//
// Pillow reference (not in this tree; Pillow 10+ src/libImaging/Resample.c): ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc with PRECISION_BITS = 22: acc starts at 1<<21, adds u8*coef (int32 wraps never
// reached: |coef| < 2^22*1.x, <= ~30 taps), result = clip8(acc >> 22).
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= PRECISION_BITS;  // arithmetic shift, like the C code's signed >>
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// workgroup = one source row: the row (sw*3 bytes, 5760 for 1080p) is staged into LDS with 16-byte coalesced loads, then
// every thread produces output pixels of that row from LDS.  (One thread per output pixel reading its taps straight from
// global memory issued 3 byte loads per tap on overlapping 12..24-byte windows: 0.4 TB/s.)
constexpr int RESIZE_H_MAX_ROW = 16384;  // bytes of LDS for one source row (sw <= 5461)
__global__ __launch_bounds__(256) void pil_resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           int n, int sh, int sw, int dw,
                                                           const int32_t* __restrict__ bounds,
                                                           const int32_t* __restrict__ kk, int ksize, int swap_rb) {
  __shared__ __attribute__((aligned(16))) uint8_t rowbuf[RESIZE_H_MAX_ROW];
  const int rowb = sw * 3;
  for (int64_t row = blockIdx.x; row < (int64_t)n * sh; row += gridDim.x) {
    const uint8_t* srow = src + row * rowb;
    // rows start at arbitrary byte offsets: align the 16-byte loads on the global address, not on the row
    const int mis = (int)(reinterpret_cast<uintptr_t>(srow) & 15);
    const int head = mis ? 16 - mis : 0;
    for (int i = threadIdx.x; i < head && i < rowb; i += blockDim.x) rowbuf[i] = srow[i];
    const int nvec = (rowb - head) > 0 ? (rowb - head) / 16 : 0;
    for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(srow + head + v * 16);
      // LDS destination head + 16v is 16-byte aligned only when head == 0: store as four dwords when it is not
      uint8_t* d = rowbuf + head + v * 16;
      if ((head & 3) == 0) {
        reinterpret_cast<unsigned*>(d)[0] = x[0];
        reinterpret_cast<unsigned*>(d)[1] = x[1];
        reinterpret_cast<unsigned*>(d)[2] = x[2];
        reinterpret_cast<unsigned*>(d)[3] = x[3];
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) d[e] = (uint8_t)(x[e >> 2] >> (8 * (e & 3)));
      }
    }
    for (int i = head + nvec * 16 + threadIdx.x; i < rowb; i += blockDim.x) rowbuf[i] = srow[i];
    __syncthreads();
    uint8_t* drow = dst + row * dw * 3;
    for (int xo = threadIdx.x; xo < dw; xo += blockDim.x) {
      const int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
      const int32_t* k = kk + (int64_t)xo * ksize;
      const uint8_t* s = rowbuf + xmin * 3;
      int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
      for (int x = 0; x < cnt; ++x) {
        const int c = k[x];
        a0 += (int)s[3 * x + 0] * c;
        a1 += (int)s[3 * x + 1] * c;
        a2 += (int)s[3 * x + 2] * c;
      }
      uint8_t* d = drow + xo * 3;
      if (swap_rb) {
        d[0] = clip8(a2);
        d[1] = clip8(a1);
        d[2] = clip8(a0);
      } else {
        d[0] = clip8(a0);
        d[1] = clip8(a1);
        d[2] = clip8(a2);
      }
    }
    __syncthreads();  // the next row overwrites rowbuf
  }
}

// thread = one output BYTE column element (x*3+c) of one output row: consecutive threads read consecutive bytes.
__global__ __launch_bounds__(256) void pil_resize_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           int n, int sh, int dh, int w,
                                                           const int32_t* __restrict__ bounds,
                                                           const int32_t* __restrict__ kk, int ksize) {
  const int rowb = w * 3;
  const int64_t total = (int64_t)n * dh * rowb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xb = (int)(i % rowb);
    const int64_t r = i / rowb;
    const int yo = (int)(r % dh);
    const int img = (int)(r / dh);
    const int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    const int32_t* k = kk + (int64_t)yo * ksize;
    const uint8_t* s = src + ((int64_t)img * sh + ymin) * rowb + xb;
    int a = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < cnt; ++y) a += (int)s[(int64_t)y * rowb] * k[y];
    dst[i] = clip8(a);
  }
}

// the same pass with FOUR consecutive bytes per thread (row length a multiple of 4 bytes, 4-byte aligned images): one dword load
// per tap row and one dword store instead of four byte loads and four byte stores — identical integer arithmetic per byte
__global__ __launch_bounds__(256) void pil_resize_v4_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int sh,
                                                            int dh, int w, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ kk, int ksize) {
  const int rowb = w * 3, roww = rowb / 4;
  const int64_t total = (int64_t)n * dh * roww;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xw = (int)(i % roww);
    const int64_t r = i / roww;
    const int yo = (int)(r % dh);
    const int img = (int)(r / dh);
    const int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    const int32_t* k = kk + (int64_t)yo * ksize;
    const uint8_t* s = src + ((int64_t)img * sh + ymin) * rowb + xw * 4;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int y = 0; y < cnt; ++y) {
      const unsigned v = *reinterpret_cast<const unsigned*>(s + (int64_t)y * rowb);
      const int c = k[y];
      a0 += (int)(v & 255u) * c;
      a1 += (int)((v >> 8) & 255u) * c;
      a2 += (int)((v >> 16) & 255u) * c;
      a3 += (int)(v >> 24) * c;
    }
    *reinterpret_cast<unsigned*>(dst + r * rowb + xw * 4) =
        (unsigned)clip8(a0) | ((unsigned)clip8(a1) << 8) | ((unsigned)clip8(a2) << 16) | ((unsigned)clip8(a3) << 24);
  }
}

// thread = one cropped pixel; writes its 3 normalised f16 values at the im2col position of its patch.
__global__ __launch_bounds__(256) void patchify_norm_kernel(const uint8_t* __restrict__ img, half_t* __restrict__ out,
                                                            int n, int ih, int iw, int top, int left, int gh, int gw,
                                                            int P, int64_t ldo, const float* __restrict__ lut) {
  const int ch = gh * P, cw = gw * P;
  const int64_t total = (int64_t)n * ch * cw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % cw);
    const int64_t r = i / cw;
    const int y = (int)(r % ch);
    const int b = (int)(r / ch);
    const uint8_t* s = img + (((int64_t)b * ih + top + y) * iw + left + x) * 3;
    const int py = y / P, ky = y - py * P, px = x / P, kx = x - px * P;
    half_t* d = out + (((int64_t)b * gh + py) * gw + px) * ldo + (ky * P + kx) * 3;
    // rescale + normalize depend only on (channel, byte): a 3x256 f32 table built on the host with the
    // processor's own numpy expression (lmx/resample.py) makes this step exact by construction.
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (half_t)lut[c * 256 + s[c]];
  }
}

// ---- DINOv3ViTImageProcessor: rescale -> float32 antialiased resize -> normalize, written as the patch matrix ----------
// torch reference (not in this tree; aten/src/ATen/native/cpu/UpSampleKernel.cpp, the separable antialias path): width is
// resampled first, then height, the intermediate is f32, and each output is src[0]*w[0] followed by one fused multiply-add
// per further tap, in tap order.  The weights come from the host (lmx/resample.py aa_tables, ATen's f32 arithmetic).
//
// workgroup = FR_ROWS output rows x FR_COLS output columns of one frame; thread = one output column.  The source rows the
// band needs are walked ONCE, top to bottom: a row's segment is staged into LDS as f32 (u8 -> float, * rescale: done once
// per source element, 16-byte coalesced loads), every thread resamples its column horizontally from LDS, and the value is
// folded at once into the vertical accumulators of the output rows whose tap range holds this source row — rows arrive in
// increasing order, so every output sees its taps in ATen's order.  No intermediate image exists, in HBM or in LDS; a
// source row is re-read only by the neighbouring band (tap overlap: 2 x support rows per band, L2 hits mostly).
constexpr int FR_ROWS = 8;
constexpr int FR_COLS = 256;
constexpr int FR_MAX_LDS = 65536;  // bytes: (seg_cols * 3 + 4) floats

__global__ __launch_bounds__(FR_COLS) void float_resize_patchify_kernel(
    const uint8_t* __restrict__ src, half_t* __restrict__ out, int sh, int sw, int gh, int gw, int P, int64_t ldo,
    const int32_t* __restrict__ bh, const float* __restrict__ kh, int ksh, const int32_t* __restrict__ bv,
    const float* __restrict__ kv, int ksv, int seg_cols, float rescale, float m0, float m1, float m2, float s0, float s1,
    float s2, int swap_rb) {
  extern __shared__ __attribute__((aligned(16))) float seg[];
  const int tid = threadIdx.x;
  const int dh = gh * P, dw = gw * P;
  const int img = blockIdx.z;
  const int x0 = blockIdx.x * FR_COLS, xo = x0 + tid;
  const int y0 = blockIdx.y * FR_ROWS;
  const bool live = xo < dw;
  // source columns of this tile: bounds are monotone in the output index.  Everything read from the tables is clamped
  // to the frame and to the LDS segment, so a malformed table gives wrong pixels, never an access outside either.
  const int xl = (x0 + FR_COLS < dw ? x0 + FR_COLS : dw) - 1;
  int c_lo = bh[2 * x0];
  c_lo = c_lo < 0 ? 0 : (c_lo > sw ? sw : c_lo);
  int c_hi = bh[2 * xl] + bh[2 * xl + 1];
  c_hi = c_hi > sw ? sw : c_hi;
  if (c_hi > c_lo + seg_cols) c_hi = c_lo + seg_cols;
  if (c_hi < c_lo) c_hi = c_lo;
  int xmin = 0, xcnt = 0;
  if (live) {
    xmin = bh[2 * xo];
    xcnt = bh[2 * xo + 1];
    if (xmin < c_lo) xmin = c_lo;
    if (xcnt > ksh) xcnt = ksh;
    if (xcnt > c_hi - xmin) xcnt = c_hi - xmin;
    if (xcnt < 0) xcnt = 0;
  }
  const float* kx = kh + (int64_t)(live ? xo : 0) * ksh;
  // tap ranges of the band's output rows (uniform over the workgroup)
  int ymin[FR_ROWS], ycnt[FR_ROWS];
  int r_lo = sh, r_hi = 0;
#pragma unroll
  for (int r = 0; r < FR_ROWS; ++r) {
    ymin[r] = 0;
    ycnt[r] = 0;
    if (y0 + r < dh) {
      int a = bv[2 * (y0 + r)], c = bv[2 * (y0 + r) + 1];
      a = a < 0 ? 0 : a;
      c = c > ksv ? ksv : c;
      c = c > sh - a ? sh - a : c;
      c = c < 0 ? 0 : c;
      ymin[r] = a;
      ycnt[r] = c;
      if (c > 0) {
        r_lo = a < r_lo ? a : r_lo;
        r_hi = a + c > r_hi ? a + c : r_hi;
      }
    }
  }
  float acc[FR_ROWS][3];
#pragma unroll
  for (int r = 0; r < FR_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;

  const int nbytes = (c_hi - c_lo) * 3;
  for (int y = r_lo; y < r_hi; ++y) {
    const uint8_t* srow = src + (((int64_t)img * sh + y) * sw + c_lo) * 3;
    // 16-byte loads aligned on the global address; the LDS index is shifted by `pad` so that the vector part of the
    // segment starts on a 16-byte LDS boundary too
    const int mis = (int)(reinterpret_cast<uintptr_t>(srow) & 15);
    int head = mis ? 16 - mis : 0;
    head = head > nbytes ? nbytes : head;
    const int pad = (4 - (head & 3)) & 3;
    float* s = seg + pad;
    if (tid < head) s[tid] = (float)srow[tid] * rescale;
    const int nvec = (nbytes - head) / 16;
    for (int v = tid; v < nvec; v += FR_COLS) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(srow + head + v * 16);
      f32x4* d = reinterpret_cast<f32x4*>(s + head + v * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 f;
        f[0] = (float)(x[q] & 255u) * rescale;
        f[1] = (float)((x[q] >> 8) & 255u) * rescale;
        f[2] = (float)((x[q] >> 16) & 255u) * rescale;
        f[3] = (float)(x[q] >> 24) * rescale;
        d[q] = f;
      }
    }
    for (int i = head + nvec * 16 + tid; i < nbytes; i += FR_COLS) s[i] = (float)srow[i] * rescale;
    __syncthreads();
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
    const float* p = s + (xmin - c_lo) * 3;
    for (int j = 0; j < xcnt; ++j) {
      const float w = kx[j];
      h0 = __builtin_fmaf(p[3 * j + 0], w, h0);
      h1 = __builtin_fmaf(p[3 * j + 1], w, h1);
      h2 = __builtin_fmaf(p[3 * j + 2], w, h2);
    }
#pragma unroll
    for (int r = 0; r < FR_ROWS; ++r) {
      if (y >= ymin[r] && y < ymin[r] + ycnt[r]) {
        const float w = kv[(int64_t)(y0 + r) * ksv + (y - ymin[r])];
        acc[r][0] = __builtin_fmaf(h0, w, acc[r][0]);
        acc[r][1] = __builtin_fmaf(h1, w, acc[r][1]);
        acc[r][2] = __builtin_fmaf(h2, w, acc[r][2]);
      }
    }
    __syncthreads();  // the next row overwrites the segment
  }
  if (!live) return;
  const int px = xo / P, kxp = xo - px * P;
#pragma unroll
  for (int r = 0; r < FR_ROWS; ++r) {
    const int yo = y0 + r;
    if (yo >= dh) break;
    const int py = yo / P, ky = yo - py * P;
    half_t* d = out + (((int64_t)img * gh + py) * gw + px) * ldo + (ky * P + kxp) * 3;
    // torchvision normalize: (x - mean) / std, a true f32 division
    d[0] = (half_t)(((swap_rb ? acc[r][2] : acc[r][0]) - m0) / s0);
    d[1] = (half_t)((acc[r][1] - m1) / s1);
    d[2] = (half_t)(((swap_rb ? acc[r][0] : acc[r][2]) - m2) / s2);
  }
}

inline int grid_for(int64_t total) {
  int64_t g = (total + 255) / 256;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int lmx_k_pil_resize_h(const uint8_t* src, uint8_t* dst, int n, int sh, int sw, int dw, const int32_t* bounds,
                                  const int32_t* kk, int ksize, int swap_rb, lmx_stream_t stream) {
  LMX_REQUIRE(src && dst && bounds && kk, "lmx_k_pil_resize_h: null pointer");
  LMX_REQUIRE(n > 0 && sh > 0 && sw > 0 && dw > 0 && ksize > 0, "lmx_k_pil_resize_h: shape");
  LMX_REQUIRE(sw * 3 <= RESIZE_H_MAX_ROW, "lmx_k_pil_resize_h: source rows wider than %d pixels are not staged", RESIZE_H_MAX_ROW / 3);
  int64_t rows = (int64_t)n * sh;
  hipLaunchKernelGGL(pil_resize_h_kernel, dim3((unsigned)(rows < 256 * 16 ? rows : 256 * 16)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, sw, dw, bounds, kk, ksize, swap_rb);
  return lmx_launch_check("pil_resize_h_kernel");
}

extern "C" int lmx_k_pil_resize_v(const uint8_t* src, uint8_t* dst, int n, int sh, int dh, int w, const int32_t* bounds,
                                  const int32_t* kk, int ksize, lmx_stream_t stream) {
  LMX_REQUIRE(src && dst && bounds && kk, "lmx_k_pil_resize_v: null pointer");
  LMX_REQUIRE(n > 0 && sh > 0 && dh > 0 && w > 0 && ksize > 0, "lmx_k_pil_resize_v: shape");
  if ((w * 3) % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {  // four bytes per thread
    hipLaunchKernelGGL(pil_resize_v4_kernel, dim3(grid_for((int64_t)n * dh * (w * 3 / 4))), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, dh, w, bounds, kk, ksize);
    return lmx_launch_check("pil_resize_v4_kernel");
  }
  hipLaunchKernelGGL(pil_resize_v_kernel, dim3(grid_for((int64_t)n * dh * w * 3)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, dh, w, bounds, kk, ksize);
  return lmx_launch_check("pil_resize_v_kernel");
}

extern "C" int lmx_k_float_resize_patchify(const uint8_t* src, void* out, int n, int sh, int sw, int gh, int gw, int P,
                                           int64_t ldo, const int32_t* bounds_h, const float* kk_h, int ksize_h,
                                           const int32_t* bounds_v, const float* kk_v, int ksize_v, int seg_cols,
                                           float rescale, const float* mean_std, int swap_rb, lmx_stream_t stream) {
  LMX_REQUIRE(src && out && bounds_h && kk_h && bounds_v && kk_v && mean_std, "lmx_k_float_resize_patchify: null pointer");
  LMX_REQUIRE(n > 0 && n <= 65535 && sh > 0 && sw > 0 && gh > 0 && gw > 0 && P > 0 && ksize_h > 0 && ksize_v > 0,
              "lmx_k_float_resize_patchify: shape");
  LMX_REQUIRE(ldo >= (int64_t)P * P * 3, "lmx_k_float_resize_patchify: ldo %lld < P*P*3", (long long)ldo);
  LMX_REQUIRE((int64_t)gh * P <= 65535 * (int64_t)FR_ROWS && (int64_t)gw * P <= (1 << 20), "lmx_k_float_resize_patchify: output size");
  LMX_REQUIRE(seg_cols > 0 && seg_cols <= sw, "lmx_k_float_resize_patchify: seg_cols %d outside 1..%d", seg_cols, sw);
  const int64_t lds = ((int64_t)seg_cols * 3 + 4) * (int64_t)sizeof(float);
  LMX_REQUIRE(lds <= FR_MAX_LDS, "lmx_k_float_resize_patchify: a tile of %d output columns reads %d source columns; more than %d are not staged",
              FR_COLS, seg_cols, (FR_MAX_LDS / 4 - 4) / 3);
  LMX_REQUIRE(mean_std[3] != 0.f && mean_std[4] != 0.f && mean_std[5] != 0.f, "lmx_k_float_resize_patchify: zero std");
  const dim3 grid((unsigned)((gw * P + FR_COLS - 1) / FR_COLS), (unsigned)((gh * P + FR_ROWS - 1) / FR_ROWS), (unsigned)n);
  hipLaunchKernelGGL(float_resize_patchify_kernel, grid, dim3(FR_COLS), (size_t)lds, reinterpret_cast<hipStream_t>(stream), src,
                     reinterpret_cast<half_t*>(out), sh, sw, gh, gw, P, ldo, bounds_h, kk_h, ksize_h, bounds_v, kk_v, ksize_v,
                     seg_cols, rescale, mean_std[0], mean_std[1], mean_std[2], mean_std[3], mean_std[4], mean_std[5], swap_rb);
  return lmx_launch_check("float_resize_patchify_kernel");
}

extern "C" int lmx_k_patchify_norm(const uint8_t* img, void* out, int n, int ih, int iw, int top, int left, int gh,
                                   int gw, int P, int64_t ldo, const float* lut, lmx_stream_t stream) {
  LMX_REQUIRE(img && out && lut, "lmx_k_patchify_norm: null pointer");
  LMX_REQUIRE(n > 0 && gh > 0 && gw > 0 && P > 0 && ldo >= (int64_t)P * P * 3, "lmx_k_patchify_norm: shape");
  LMX_REQUIRE(top >= 0 && left >= 0 && top + gh * P <= ih && left + gw * P <= iw,
              "lmx_k_patchify_norm: crop (%d,%d)+(%d,%d) outside %dx%d", top, left, gh * P, gw * P, ih, iw);
  hipLaunchKernelGGL(patchify_norm_kernel, dim3(grid_for((int64_t)n * gh * P * gw * P)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), img, reinterpret_cast<half_t*>(out), n, ih, iw, top, left, gh,
                     gw, P, ldo, lut);
  return lmx_launch_check("patchify_norm_kernel");
}
