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

// clip8(v >> PRECISION_BITS) of the C code (an arithmetic shift, then the clamp to 0..255), written as the clamp of the
// accumulator followed by a logical shift.  The values are the same; the form is not: from shift-then-clamp of two bytes that
// are packed side by side hipcc selects v_ashr_pk_u8_i32 and ORs the other bytes into its result as if the upper 16 bits were
// zero, and on gfx950 they keep what the register held before (seen as wrong bytes 2 of the 16-byte vertical pass).
__device__ __forceinline__ uint8_t clip8(int v) {
  const int top = (256 << PRECISION_BITS) - 1;
  v = v < 0 ? 0 : (v > top ? top : v);
  return (uint8_t)((unsigned)v >> PRECISION_BITS);
}

// One tap of the 8bpc passes: byte * coefficient.  Pillow's coefficients are round(w * 2^22) with normalised weights |w| < 2, so
// both operands fit 24 signed bits and the 24-bit multiply returns the bits of the 32-bit one at the full VALU rate.
__device__ __forceinline__ int tap(unsigned byte, int coef) { return __mul24((int)byte, coef); }

// workgroup = a group of consecutive source rows (they are contiguous in memory, across frames too): the group's bytes are
// staged into LDS as ONE span with 16-byte coalesced loads, LDS index = global address modulo 16 + offset in the span, so that
// every 16-byte global block lands on a 16-byte LDS slot whatever the rows' alignment.  One barrier pair covers the group.
// thread = one output pixel of RESIZE_H_ROWS staged rows: a coefficient is loaded once for the four rows.  The 12 output bytes
// of four neighbouring pixels leave as three dword stores of three of the four lanes, which take the next lane's bytes by a
// shuffle.  Measured and not kept: the tap's three bytes as one dword read at the pixel's own (unaligned) LDS address, 2.1 x
// slower; four pixels per thread with a 12-byte store each, 110 against 128 us on SAM's 30-frame pass and 951 against 930 us on
// DINO's 150-frame bicubic pass, the same in sum; four coefficient loads issued ahead of their taps, no change.  (One row per
// workgroup pass, three byte stores per pixel and a coefficient load per tap and row took 152 and 1010 us; one thread per output
// pixel reading its taps straight from global memory ran at 0.4 TB/s.)
// Integer adds: any tap order gives Pillow's bits.
constexpr int RESIZE_H_MAX_ROW = 16384;             // longest source row staged, bytes (sw <= 5461)
constexpr int RESIZE_H_LDS = 2 * RESIZE_H_MAX_ROW;  // the staging buffer: 15 bytes of misalignment + the group's rows
constexpr int RESIZE_H_ROWS = 4;

// rows per staging group: what the buffer holds, at most 8 (narrow frames keep enough workgroups), whole thread tasks above 4
inline int resize_h_group(int rowb) {
  int r = (RESIZE_H_LDS - 16) / rowb;
  r = r > 8 ? 8 : r;
  return r >= RESIZE_H_ROWS ? r / RESIZE_H_ROWS * RESIZE_H_ROWS : r;
}

__global__ __launch_bounds__(256) void pil_resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           int n, int sh, int sw, int dw, int group,
                                                           const int32_t* __restrict__ bounds,
                                                           const int32_t* __restrict__ kk, int ksize, int swap_rb) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[RESIZE_H_LDS];
  const int rowb = sw * 3;
  const int64_t rows = (int64_t)n * sh;
  const int dwq = (dw + 3) & ~3;  // whole quads of pixels: a quad lies in one wave (256 and dwq are multiples of 4)
  for (int64_t row0 = (int64_t)blockIdx.x * group; row0 < rows; row0 += (int64_t)gridDim.x * group) {
    const int nr = rows - row0 < group ? (int)(rows - row0) : group;
    const uint8_t* s0 = src + row0 * rowb;
    const int span = nr * rowb;
    const int mis = (int)(reinterpret_cast<uintptr_t>(s0) & 15);
    int head = mis ? 16 - mis : 0;
    head = head > span ? span : head;
    for (int i = threadIdx.x; i < head; i += blockDim.x) buf[mis + i] = s0[i];
    const int nvec = (span - head) / 16;  // mis + head is 0 or 16: aligned on both sides
    for (int v = threadIdx.x; v < nvec; v += blockDim.x)
      *reinterpret_cast<u32x4*>(buf + mis + head + v * 16) = *reinterpret_cast<const u32x4*>(s0 + head + v * 16);
    for (int i = head + nvec * 16 + threadIdx.x; i < span; i += blockDim.x) buf[mis + i] = s0[i];
    __syncthreads();
    const int ntask = dwq * ((nr + RESIZE_H_ROWS - 1) / RESIZE_H_ROWS);
    for (int t0 = 0; t0 < ntask; t0 += blockDim.x) {  // workgroup-uniform: every lane of a wave reaches the shuffle
      const int t = t0 + threadIdx.x;
      const int rg = t / dwq, xq = t - rg * dwq;
      const int r0 = rg * RESIZE_H_ROWS;
      const bool live = t < ntask && xq < dw;
      // lanes past the row's last pixel and rows past the group's last compute on the last valid one and store nothing
      const int xo = xq < dw ? xq : dw - 1;
      int rb[RESIZE_H_ROWS];
#pragma unroll
      for (int r = 0; r < RESIZE_H_ROWS; ++r) rb[r] = mis + (r0 + r < nr ? r0 + r : nr - 1) * rowb;
      const int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
      const int32_t* k = kk + (int64_t)xo * ksize;
      int a[RESIZE_H_ROWS][3];
#pragma unroll
      for (int r = 0; r < RESIZE_H_ROWS; ++r) a[r][0] = a[r][1] = a[r][2] = 1 << (PRECISION_BITS - 1);
      for (int x = 0; x < cnt; ++x) {
        const int c = k[x];
        const int off = (xmin + x) * 3;
#pragma unroll
        for (int r = 0; r < RESIZE_H_ROWS; ++r) {
          const uint8_t* s = buf + rb[r] + off;
          a[r][0] += tap(s[0], c);
          a[r][1] += tap(s[1], c);
          a[r][2] += tap(s[2], c);
        }
      }
      const int j = xq & 3;  // place in the quad; the quad's 12 bytes are dwords 0..2 of lanes j = 0..2
      const bool quad = xq - j + 4 <= dw;
#pragma unroll
      for (int r = 0; r < RESIZE_H_ROWS; ++r) {
        const unsigned b0 = clip8(swap_rb ? a[r][2] : a[r][0]), b1 = clip8(a[r][1]), b2 = clip8(swap_rb ? a[r][0] : a[r][2]);
        const unsigned px = b0 | (b1 << 8) | (b2 << 16);
        const unsigned nx = __shfl_down(px, 1, 64);  // the next pixel's bytes (unused by j = 3)
        if (!live || r0 + r >= nr) continue;
        uint8_t* d = dst + (row0 + r0 + r) * dw * 3 + xq * 3;  // this pixel's bytes; the quad's start with d - 3 * j
        if (quad && ((reinterpret_cast<uintptr_t>(d) - 3 * j) & 3) == 0) {
          if (j < 3) *reinterpret_cast<unsigned*>(d - 3 * j + 4 * j) = (px >> (8 * j)) | (nx << (24 - 8 * j));
        } else {  // the row's last pixels, or an output row that is not dword-aligned
          d[0] = (uint8_t)b0;
          d[1] = (uint8_t)b1;
          d[2] = (uint8_t)b2;
        }
      }
    }
    __syncthreads();  // the next group overwrites buf
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
    for (int y = 0; y < cnt; ++y) a += tap(s[(int64_t)y * rowb], k[y]);
    dst[i] = clip8(a);
  }
}

// the same pass with 4 * DW consecutive bytes per thread: one load of DW dwords per tap row and one store instead of byte loads
// and byte stores, identical integer arithmetic per byte.  DW = 4 (16 bytes) where the row length is a multiple of 16 bytes and
// the images are 16-byte aligned.  DW = 1 for every other row of 4 bytes or more: dword loads and stores at the bytes' own
// addresses, aligned or not (rows of 1365 bytes, DINO's 455 columns, have every alignment), and where the row length is no
// multiple of 4 the row's last piece is moved back to end with the row: the bytes it shares with its neighbour are computed
// twice, to the same values.
template <int DW>
__global__ __launch_bounds__(256) void pil_resize_vw_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int sh,
                                                            int dh, int w, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ kk, int ksize) {
  typedef unsigned vec_t __attribute__((ext_vector_type(DW)));
  const int rowb = w * 3, roww = (rowb + 4 * DW - 1) / (4 * DW);
  const int64_t total = (int64_t)n * dh * roww;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xw = (int)(i % roww);
    const int64_t r = i / roww;
    const int yo = (int)(r % dh);
    const int img = (int)(r / dh);
    const int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    const int32_t* k = kk + (int64_t)yo * ksize;
    const int xb = xw * (4 * DW) + 4 * DW <= rowb ? xw * (4 * DW) : rowb - 4 * DW;
    const uint8_t* s = src + ((int64_t)img * sh + ymin) * rowb + xb;
    int a[4 * DW];
#pragma unroll
    for (int e = 0; e < 4 * DW; ++e) a[e] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < cnt; ++y) {
      vec_t v;
      if (DW == 4)
        v = *reinterpret_cast<const vec_t*>(s + (int64_t)y * rowb);
      else
        __builtin_memcpy(&v, s + (int64_t)y * rowb, sizeof(v));
      const int c = k[y];
#pragma unroll
      for (int q = 0; q < DW; ++q) {
        a[4 * q + 0] += tap(v[q] & 255u, c);
        a[4 * q + 1] += tap((v[q] >> 8) & 255u, c);
        a[4 * q + 2] += tap((v[q] >> 16) & 255u, c);
        a[4 * q + 3] += tap(v[q] >> 24, c);
      }
    }
    vec_t o;
#pragma unroll
    for (int q = 0; q < DW; ++q)
      o[q] = (unsigned)clip8(a[4 * q]) | ((unsigned)clip8(a[4 * q + 1]) << 8) | ((unsigned)clip8(a[4 * q + 2]) << 16) |
             ((unsigned)clip8(a[4 * q + 3]) << 24);
    if (DW == 4)
      *reinterpret_cast<vec_t*>(dst + r * rowb + xb) = o;
    else
      __builtin_memcpy(dst + r * rowb + xb, &o, sizeof(o));
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
  const int group = resize_h_group(sw * 3);
  const int64_t groups = ((int64_t)n * sh + group - 1) / group;
  hipLaunchKernelGGL(pil_resize_h_kernel, dim3((unsigned)(groups < 256 * 16 ? groups : 256 * 16)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, sw, dw, group, bounds, kk, ksize, swap_rb);
  return lmx_launch_check("pil_resize_h_kernel");
}

extern "C" int lmx_k_pil_resize_v(const uint8_t* src, uint8_t* dst, int n, int sh, int dh, int w, const int32_t* bounds,
                                  const int32_t* kk, int ksize, lmx_stream_t stream) {
  LMX_REQUIRE(src && dst && bounds && kk, "lmx_k_pil_resize_v: null pointer");
  LMX_REQUIRE(n > 0 && sh > 0 && dh > 0 && w > 0 && ksize > 0, "lmx_k_pil_resize_v: shape");
  const uintptr_t al = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)(w * 3);
  if ((al & 15) == 0) {  // sixteen bytes per thread
    hipLaunchKernelGGL(pil_resize_vw_kernel<4>, dim3(grid_for((int64_t)n * dh * (w * 3 / 16))), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, dh, w, bounds, kk, ksize);
    return lmx_launch_check("pil_resize_vw_kernel<4>");
  }
  if (w * 3 >= 4) {  // four bytes per thread
    hipLaunchKernelGGL(pil_resize_vw_kernel<1>, dim3(grid_for((int64_t)n * dh * ((w * 3 + 3) / 4))), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, dst, n, sh, dh, w, bounds, kk, ksize);
    return lmx_launch_check("pil_resize_vw_kernel<1>");
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
