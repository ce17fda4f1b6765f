// yuv.hip — frames from a decoder: YUV 4:2:0 (NV12 pitched surfaces, planar I420) -> packed BGR u8, the format every other entry
// point takes.  HBM-bound byte work: 1.5 bytes in and 3 bytes out per pixel, so the figure of merit is 4.5 B/px over time
// (profiles/yuv_ingest.txt).  The arithmetic is include/lmx.h's text at lmx_k_yuv420_to_bgr (limited range, 20-bit fixed point,
// nearest chroma; PARITY UNPINNED against real OpenCV); csrc/host_yuv.cpp restates it in plain C++.
//
// thread = a block of 2 rows x 16 columns, the two luma rows that share one chroma row: 16 + 16 luma bytes, 16 chroma bytes (NV12:
// eight U V pairs; I420: 8 + 8), 48 + 48 output bytes.  Consecutive threads take consecutive blocks of a row pair, so a wave reads
// 1 KiB of each luma row and writes 3 KiB of each output row.  Each of the block's six pieces moves as ONE 16-byte (I420 chroma:
// 8-byte) load, or as three 16-byte stores, where the block is whole and the piece's address is aligned, and byte by byte
// otherwise — decided per piece, so an aligned surface converted into an unaligned buffer still loads wide.  The pixel arithmetic sits
// between the two and is the same code for both.  A frame with w % 16 == 0, aligned planes and pitches has no byte piece.  No LDS, no
// atomics, no workspace; every output byte is stored exactly once.
//
// Behind it, in the same shape (profiles/yuv_egress.txt): the crop window, lmx_k_yuv420_to_bgr_roi — the same pixels for a part of every
// frame, blocks laid on the source's grid — and the way back to an encoder, lmx_k_bgr_to_yuv420 (limited range, 20-bit fixed point,
// chroma from the 2 x 2 sums, a pitched BGR source).  Their texts stand beside them in include/lmx.h.
#include "common.h"
#include "yuv.h"

namespace {

constexpr int BW = 16;  // columns of a thread's block

struct YuvArgs {
  const uint8_t *y, *u, *v;
  int64_t pitch_y, pitch_c, stride_y, stride_c;
  LmxYuvCoef k;
};

// sat8(v >> 20) of the text (an arithmetic shift, then the clamp to 0 .. 255) written as the clamp of v followed by a logical
// shift: the same values, and not the form from which hipcc selects v_ashr_pk_u8_i32 (pre.hip, clip8)
__device__ __forceinline__ unsigned sat8(int v) {
  const int top = (256 << LMX_YUV_SHIFT) - 1;
  v = v < 0 ? 0 : (v > top ? top : v);
  return (unsigned)v >> LMX_YUV_SHIFT;
}

// coefficient * (byte - offset): every coefficient is below 2^23 in magnitude and the other factor within -128 .. 239, so the 24-bit
// multiply returns the bits of the 32-bit one at the full VALU rate (as pre.hip's tap)
__device__ __forceinline__ int mul(int coef, int x) { return __mul24(coef, x); }

__device__ __forceinline__ unsigned byte_of(const u32x4& v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 255u; }

// `cnt` (<= 16) bytes at p into the low bytes of a 16-byte vector: one load where the piece is whole and aligned
__device__ __forceinline__ u32x4 load16(const uint8_t* p, int cnt) {
  if (cnt == BW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const u32x4*>(p);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < BW; ++i)
    if (i < cnt) v[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
  return v;
}
__device__ __forceinline__ u32x2 load8(const uint8_t* p, int cnt) {
  if (cnt == BW / 2 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const u32x2*>(p);
  u32x2 v = {0u, 0u};
#pragma unroll
  for (int i = 0; i < BW / 2; ++i)
    if (i < cnt) v[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
  return v;
}

// the 3 * cnt bytes of one output row of the block: px[i] = B | G << 8 | R << 16 of pixel i
__device__ __forceinline__ void store_row(uint8_t* d, const unsigned (&px)[BW], int cnt) {
  if (cnt == BW && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {  // four pixels are three dwords
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d3 = 4 * q + j, g = d3 / 3 * 4, r = d3 % 3;  // dword d3 of the row: dword r of pixel group g .. g + 3
        o[j] = r == 0 ? (px[g] | (px[g + 1] << 24)) : r == 1 ? ((px[g + 1] >> 8) | (px[g + 2] << 16)) : ((px[g + 2] >> 16) | (px[g + 3] << 8));
      }
      *reinterpret_cast<u32x4*>(d + 16 * q) = o;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < BW; ++i)
    if (i < cnt) {
      d[3 * i + 0] = (uint8_t)(px[i] & 255u);
      d[3 * i + 1] = (uint8_t)((px[i] >> 8) & 255u);
      d[3 * i + 2] = (uint8_t)(px[i] >> 16);
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv420_to_bgr_kernel(YuvArgs a, int n, int h, int w, uint8_t* __restrict__ bgr) {
  const int bx = (w + BW - 1) / BW, hp = h / 2;
  const int64_t total = (int64_t)n * hp * bx;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int xb = (int)(t % bx);
    const int64_t r = t / bx;
    const int yp = (int)(r % hp);
    const int64_t img = r / hp;
    const int x0 = xb * BW;
    const int cnt = w - x0 < BW ? w - x0 : BW;  // even: w is
    const uint8_t* py = a.y + img * a.stride_y + (int64_t)(2 * yp) * a.pitch_y + x0;
    const u32x4 y0 = load16(py, cnt), y1 = load16(py + a.pitch_y, cnt);
    // chroma pair j of the block as U | V << 8
    unsigned uv[BW / 2];
    if (LAYOUT == LMX_YUV_NV12) {
      const u32x4 c = load16(a.u + img * a.stride_c + (int64_t)yp * a.pitch_c + x0, cnt);
#pragma unroll
      for (int j = 0; j < BW / 2; ++j) uv[j] = (c[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    } else {
      const int64_t off = img * a.stride_c + (int64_t)yp * a.pitch_c + x0 / 2;
      const u32x2 cu = load8(a.u + off, cnt / 2), cv = load8(a.v + off, cnt / 2);
#pragma unroll
      for (int j = 0; j < BW / 2; ++j) uv[j] = ((cu[j >> 2] >> (8 * (j & 3))) & 255u) | (((cv[j >> 2] >> (8 * (j & 3))) & 255u) << 8);
    }
    unsigned p0[BW], p1[BW];
    const int half = 1 << (LMX_YUV_SHIFT - 1);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
      const int u = (int)(uv[j] & 255u) - 128, v = (int)(uv[j] >> 8) - 128;
      const int cb = mul(a.k.cub, u) + half, cg = mul(a.k.cug, u) + mul(a.k.cvg, v) + half, cr = mul(a.k.cvr, v) + half;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * j + e;
        const int l0 = (int)byte_of(y0, i) - 16, l1 = (int)byte_of(y1, i) - 16;
        const int yy0 = mul(a.k.cy, l0 < 0 ? 0 : l0), yy1 = mul(a.k.cy, l1 < 0 ? 0 : l1);
        p0[i] = sat8(yy0 + cb) | (sat8(yy0 + cg) << 8) | (sat8(yy0 + cr) << 16);
        p1[i] = sat8(yy1 + cb) | (sat8(yy1 + cg) << 8) | (sat8(yy1 + cr) << 16);
      }
    }
    uint8_t* d = bgr + ((img * h + 2 * yp) * (int64_t)w + x0) * 3;
    store_row(d, p0, cnt);
    store_row(d + (int64_t)w * 3, p1, cnt);
  }
}

// ---- the crop window: lmx_k_yuv420_to_bgr_roi ---------------------------------------------------------------------------------------
// A twin of the kernel above, not a template of it, so that the whole-frame kernel's code is what it was.  The blocks lie on the
// SOURCE's grid — columns xs0 = 16 * k of the frame, row pairs 2k and 2k + 1 — so that the loads of an aligned surface stay whole and
// aligned wherever the window starts; a block's live pixels are columns lo .. hi - 1 (the window's columns inside it) of the rows that
// lie inside the window.  A block on the window's left or right rim may begin or end inside a chroma pair (odd x, odd x + w), one on its
// top or bottom rim has one live row (odd y, odd y + h).  Loads: the whole 16 bytes where the block lies inside the frame and the
// address is aligned (bytes outside the window are loaded and not used: they are the frame's), else the live bytes one by one.
// Stores: three 16-byte stores where all 16 columns are live and the output address is aligned, else the live bytes one by one.

// bytes lo .. hi - 1 of the 16 at p: one load where `whole` (all 16 are the frame's) and p is aligned
__device__ __forceinline__ u32x4 load16_part(const uint8_t* p, int lo, int hi, bool whole) {
  if (whole && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const u32x4*>(p);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < BW; ++i)
    if (i >= lo && i < hi) v[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
  return v;
}
__device__ __forceinline__ u32x2 load8_part(const uint8_t* p, int lo, int hi, bool whole) {
  if (whole && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const u32x2*>(p);
  u32x2 v = {0u, 0u};
#pragma unroll
  for (int i = 0; i < BW / 2; ++i)
    if (i >= lo && i < hi) v[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
  return v;
}

// pixels lo .. hi - 1 of a block's row; d: where pixel 0 of the block would go
__device__ __forceinline__ void store_row_part(uint8_t* d, const unsigned (&px)[BW], int lo, int hi) {
  if (lo == 0 && hi == BW) {
    store_row(d, px, BW);
    return;
  }
#pragma unroll
  for (int i = 0; i < BW; ++i)
    if (i >= lo && i < hi) {
      d[3 * i + 0] = (uint8_t)(px[i] & 255u);
      d[3 * i + 1] = (uint8_t)((px[i] >> 8) & 255u);
      d[3 * i + 2] = (uint8_t)(px[i] >> 16);
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv420_to_bgr_roi_kernel(YuvArgs a, int n, int w, lmx_rect_t roi, uint8_t* __restrict__ bgr) {
  const int xb0 = roi.x / BW, bx = (roi.x + roi.w + BW - 1) / BW - xb0;  // blocks of the source grid the window touches
  const int yp0 = roi.y / 2, hp = (roi.y + roi.h + 1) / 2 - yp0;         // and its row pairs
  const int64_t total = (int64_t)n * hp * bx;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int xb = (int)(t % bx);
    const int64_t r = t / bx;
    const int yp = yp0 + (int)(r % hp);
    const int64_t img = r / hp;
    const int xs0 = (xb0 + xb) * BW;                                                  // the block's first column in the frame
    const int lo = roi.x > xs0 ? roi.x - xs0 : 0;                                     // live columns of the block: lo .. hi - 1
    const int hi = roi.x + roi.w - xs0 < BW ? roi.x + roi.w - xs0 : BW;
    const bool whole = xs0 + BW <= w;                                                 // all 16 columns are the frame's (w is even, so are its bytes)
    const int clo = lo >> 1, chi = (hi + 1) >> 1;                                     // live chroma pairs
    const uint8_t* py = a.y + img * a.stride_y + (int64_t)(2 * yp) * a.pitch_y + xs0;  // both rows are the frame's: its h is even
    const u32x4 y0 = load16_part(py, lo, hi, whole), y1 = load16_part(py + a.pitch_y, lo, hi, whole);
    unsigned uv[BW / 2];
    if (LAYOUT == LMX_YUV_NV12) {
      const u32x4 c = load16_part(a.u + img * a.stride_c + (int64_t)yp * a.pitch_c + xs0, 2 * clo, 2 * chi, whole);
#pragma unroll
      for (int j = 0; j < BW / 2; ++j) uv[j] = (c[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    } else {
      const int64_t off = img * a.stride_c + (int64_t)yp * a.pitch_c + xs0 / 2;
      const u32x2 cu = load8_part(a.u + off, clo, chi, whole), cv = load8_part(a.v + off, clo, chi, whole);
#pragma unroll
      for (int j = 0; j < BW / 2; ++j) uv[j] = ((cu[j >> 2] >> (8 * (j & 3))) & 255u) | (((cv[j >> 2] >> (8 * (j & 3))) & 255u) << 8);
    }
    unsigned p0[BW], p1[BW];
    const int half = 1 << (LMX_YUV_SHIFT - 1);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
      const int u = (int)(uv[j] & 255u) - 128, v = (int)(uv[j] >> 8) - 128;
      const int cb = mul(a.k.cub, u) + half, cg = mul(a.k.cug, u) + mul(a.k.cvg, v) + half, cr = mul(a.k.cvr, v) + half;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * j + e;
        const int l0 = (int)byte_of(y0, i) - 16, l1 = (int)byte_of(y1, i) - 16;
        const int yy0 = mul(a.k.cy, l0 < 0 ? 0 : l0), yy1 = mul(a.k.cy, l1 < 0 ? 0 : l1);
        p0[i] = sat8(yy0 + cb) | (sat8(yy0 + cg) << 8) | (sat8(yy0 + cr) << 16);
        p1[i] = sat8(yy1 + cb) | (sat8(yy1 + cg) << 8) | (sat8(yy1 + cr) << 16);
      }
    }
    // window row of source row 2 * yp is 2 * yp - roi.y (-1 on the top rim: not live), window column of block column 0 is xs0 - roi.x
    const int wy = 2 * yp - roi.y;
    uint8_t* d = bgr + ((img * roi.h + wy) * (int64_t)roi.w + (xs0 - roi.x)) * 3;
    if (wy >= 0) store_row_part(d, p0, lo, hi);
    if (wy + 1 < roi.h) store_row_part(d + (int64_t)roi.w * 3, p1, lo, hi);
  }
}

// ---- frames to an encoder: lmx_k_bgr_to_yuv420 --------------------------------------------------------------------------------------
// thread = the same 2 rows x 16 columns: 48 + 48 BGR bytes in, 16 + 16 luma bytes and 16 chroma bytes (NV12) or 8 + 8 (I420) out.  A
// row's 48 bytes move as three 16-byte loads where the block is whole and the row's address is aligned — each row for itself: the
// source is pitched, a window of a larger frame, and whether `bgr + 3 * x` is aligned is the caller's x.  A whole row off the 16-byte
// grid is that caller's normal case, so it moves dword by dword on the 4-byte grid between its first and last bytes (load_row); a row
// of a partial block moves byte by byte.  The stores: one 16-byte (I420 chroma: 8-byte) store per piece where whole and aligned, else
// the piece's bytes.
struct YuvOutArgs {
  uint8_t *y, *u, *v;
  int64_t pitch_y, pitch_c, stride_y, stride_c;
  LmxYuvOutCoef k;
};

// the text's sat8 on a value that is already shifted
__device__ __forceinline__ unsigned clip8(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// bytes 4 j + s .. 4 j + s + 3 of a little-endian dword stream: its dwords j (lo) and j + 1 (hi), s = 0 .. 4 (s = 4: hi)
__device__ __forceinline__ unsigned funnel(unsigned lo, unsigned hi, unsigned s) { return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * s)); }

// 3 * cnt bytes of a BGR row into 12 dwords
__device__ __forceinline__ void load_row(const uint8_t* p, int cnt, unsigned (&d)[12]) {
  if (cnt == BW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * q + j] = v[j];
    }
    return;
  }
  if (cnt == BW) {
    // a whole row at an address off the 16-byte grid — a window that starts at an x that is no multiple of 16, the normal case: up to
    // three bytes to the next 4-byte boundary, eleven aligned dwords (twelve where the row is 4-byte aligned) and the rest byte by byte,
    // funnelled into the same twelve dwords: 667 -> 174 us on the probe's window against the byte loop.  Every byte read is one of the
    // row's 48.
    const unsigned head = (unsigned)(0 - reinterpret_cast<uintptr_t>(p)) & 3u;
    const unsigned* q = reinterpret_cast<const unsigned*>(p + head);
    unsigned s[13];  // s[0]: the head bytes in its TOP bytes; s[1 ..]: the stream from the boundary on
    s[0] = 0u;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if ((unsigned)i < head) s[0] |= (unsigned)p[i] << (8 * (4 - head + i));
#pragma unroll
    for (int j = 0; j < 11; ++j) s[1 + j] = q[j];
    if (head == 0) {
      s[12] = q[11];
    } else {
      s[12] = 0u;
#pragma unroll
      for (int i = 1; i < 4; ++i)  // row bytes 44 + head .. 47 are stream bytes 44 .. 47 - head
        if ((unsigned)i >= head) s[12] |= (unsigned)p[44 + i] << (8 * (i - head));
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) d[j] = funnel(s[j], s[j + 1], 4 - head);
    return;
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) d[j] = 0u;
#pragma unroll
  for (int i = 0; i < 3 * BW; ++i)
    if (i < 3 * cnt) d[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
}
__device__ __forceinline__ int chan(const unsigned (&d)[12], int i, int c) { return (int)((d[(3 * i + c) >> 2] >> (8 * ((3 * i + c) & 3))) & 255u); }

__device__ __forceinline__ void store16(uint8_t* p, const u32x4& v, int cnt) {
  if (cnt == BW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *reinterpret_cast<u32x4*>(p) = v;
    return;
  }
#pragma unroll
  for (int i = 0; i < BW; ++i)
    if (i < cnt) p[i] = (uint8_t)byte_of(v, i);
}
__device__ __forceinline__ void store8(uint8_t* p, const u32x2& v, int cnt) {
  if (cnt == BW / 2 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    *reinterpret_cast<u32x2*>(p) = v;
    return;
  }
#pragma unroll
  for (int i = 0; i < BW / 2; ++i)
    if (i < cnt) p[i] = (uint8_t)((v[i >> 2] >> (8 * (i & 3))) & 255u);
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void bgr_to_yuv420_kernel(const uint8_t* __restrict__ bgr, int64_t pitch_bgr, int64_t stride_bgr, YuvOutArgs a, int n, int h,
                                                            int w) {
  const int bx = (w + BW - 1) / BW, hp = h / 2;
  const int64_t total = (int64_t)n * hp * bx;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int xb = (int)(t % bx);
    const int64_t r = t / bx;
    const int yp = (int)(r % hp);
    const int64_t img = r / hp;
    const int x0 = xb * BW;
    const int cnt = w - x0 < BW ? w - x0 : BW;  // even: w is
    const uint8_t* src = bgr + img * stride_bgr + (int64_t)(2 * yp) * pitch_bgr + 3 * (int64_t)x0;
    unsigned r0[12], r1[12];
    load_row(src, cnt, r0);
    load_row(src + pitch_bgr, cnt, r1);
    u32x4 l0 = {0u, 0u, 0u, 0u}, l1 = {0u, 0u, 0u, 0u}, cuv = {0u, 0u, 0u, 0u};
    u32x2 cu = {0u, 0u}, cv = {0u, 0u};
    const int half_y = 1 << (LMX_YUV_SHIFT - 1), half_c = 1 << (LMX_YUV_SHIFT + 1);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
      int s[3] = {0, 0, 0};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * j + e;
        const int b0 = chan(r0, i, 0), g0 = chan(r0, i, 1), q0 = chan(r0, i, 2), b1 = chan(r1, i, 0), g1 = chan(r1, i, 1), q1 = chan(r1, i, 2);
        const unsigned ya = clip8(((mul(a.k.yb, b0) + mul(a.k.yg, g0) + mul(a.k.yr, q0) + half_y) >> LMX_YUV_SHIFT) + 16);
        const unsigned yb = clip8(((mul(a.k.yb, b1) + mul(a.k.yg, g1) + mul(a.k.yr, q1) + half_y) >> LMX_YUV_SHIFT) + 16);
        l0[i >> 2] |= ya << (8 * (i & 3));
        l1[i >> 2] |= yb << (8 * (i & 3));
        s[0] += b0 + b1;
        s[1] += g0 + g1;
        s[2] += q0 + q1;
      }
      // the sums are at most 1020 and the coefficients below 2^23: the 24-bit multiply is exact; >> on a negative int is arithmetic
      const unsigned U = clip8(((mul(a.k.ub, s[0]) + mul(a.k.ug, s[1]) + mul(a.k.ur, s[2]) + half_c) >> (LMX_YUV_SHIFT + 2)) + 128);
      const unsigned V = clip8(((mul(a.k.vb, s[0]) + mul(a.k.vg, s[1]) + mul(a.k.vr, s[2]) + half_c) >> (LMX_YUV_SHIFT + 2)) + 128);
      if (LAYOUT == LMX_YUV_NV12) {
        cuv[j >> 1] |= (U | (V << 8)) << (16 * (j & 1));
      } else {
        cu[j >> 2] |= U << (8 * (j & 3));
        cv[j >> 2] |= V << (8 * (j & 3));
      }
    }
    uint8_t* py = a.y + img * a.stride_y + (int64_t)(2 * yp) * a.pitch_y + x0;
    store16(py, l0, cnt);
    store16(py + a.pitch_y, l1, cnt);
    if (LAYOUT == LMX_YUV_NV12) {
      store16(a.u + img * a.stride_c + (int64_t)yp * a.pitch_c + x0, cuv, cnt);
    } else {
      const int64_t off = img * a.stride_c + (int64_t)yp * a.pitch_c + x0 / 2;
      store8(a.u + off, cu, cnt / 2);
      store8(a.v + off, cv, cnt / 2);
    }
  }
}

inline int grid_for(int64_t total) {
  int64_t g = (total + 255) / 256;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int lmx_k_yuv420_to_bgr(const lmx_yuv_frames_t* frames_host, int n, int h, int w, uint8_t* bgr, lmx_stream_t stream) {
  LMX_TRY(lmx_yuv_check("lmx_k_yuv420_to_bgr", frames_host, n, h, w));
  LMX_REQUIRE(n == 0 || bgr != nullptr, "lmx_k_yuv420_to_bgr: null pointer (bgr)");
  if (n == 0) return LMX_OK;
  const lmx_yuv_frames_t& f = *frames_host;
  const YuvArgs a{f.y, f.u, f.v, f.pitch_y, f.pitch_c, f.stride_y, f.stride_c, lmx_yuv_coef(f.matrix)};
  const int64_t total = (int64_t)n * (h / 2) * ((w + BW - 1) / BW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (f.layout == LMX_YUV_NV12) {
    hipLaunchKernelGGL(yuv420_to_bgr_kernel<LMX_YUV_NV12>, dim3(grid_for(total)), dim3(256), 0, st, a, n, h, w, bgr);
    return lmx_launch_check("yuv420_to_bgr_kernel<NV12>");
  }
  hipLaunchKernelGGL(yuv420_to_bgr_kernel<LMX_YUV_I420>, dim3(grid_for(total)), dim3(256), 0, st, a, n, h, w, bgr);
  return lmx_launch_check("yuv420_to_bgr_kernel<I420>");
}

extern "C" int lmx_k_yuv420_to_bgr_roi(const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host, uint8_t* bgr,
                                       lmx_stream_t stream) {
  LMX_TRY(lmx_yuv_check("lmx_k_yuv420_to_bgr_roi", frames_host, n, h, w));
  LMX_TRY(lmx_yuv_check_roi("lmx_k_yuv420_to_bgr_roi", roi_host, h, w));
  LMX_REQUIRE(n == 0 || bgr != nullptr, "lmx_k_yuv420_to_bgr_roi: null pointer (bgr)");
  if (n == 0) return LMX_OK;
  const lmx_yuv_frames_t& f = *frames_host;
  const lmx_rect_t roi = *roi_host;
  const YuvArgs a{f.y, f.u, f.v, f.pitch_y, f.pitch_c, f.stride_y, f.stride_c, lmx_yuv_coef(f.matrix)};
  const int64_t total = (int64_t)n * ((roi.y + roi.h + 1) / 2 - roi.y / 2) * ((roi.x + roi.w + BW - 1) / BW - roi.x / BW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (f.layout == LMX_YUV_NV12) {
    hipLaunchKernelGGL(yuv420_to_bgr_roi_kernel<LMX_YUV_NV12>, dim3(grid_for(total)), dim3(256), 0, st, a, n, w, roi, bgr);
    return lmx_launch_check("yuv420_to_bgr_roi_kernel<NV12>");
  }
  hipLaunchKernelGGL(yuv420_to_bgr_roi_kernel<LMX_YUV_I420>, dim3(grid_for(total)), dim3(256), 0, st, a, n, w, roi, bgr);
  return lmx_launch_check("yuv420_to_bgr_roi_kernel<I420>");
}

extern "C" int lmx_k_bgr_to_yuv420(const uint8_t* bgr, int64_t pitch_bgr, int64_t stride_bgr, int n, int h, int w, const lmx_yuv_out_t* out_host,
                                   lmx_stream_t stream) {
  LMX_TRY(lmx_yuv_check_out("lmx_k_bgr_to_yuv420", bgr, pitch_bgr, out_host, n, h, w));
  if (n == 0) return LMX_OK;
  const lmx_yuv_out_t& o = *out_host;
  const YuvOutArgs a{o.y, o.u, o.v, o.pitch_y, o.pitch_c, o.stride_y, o.stride_c, lmx_yuv_out_coef(o.matrix)};
  const int64_t total = (int64_t)n * (h / 2) * ((w + BW - 1) / BW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (o.layout == LMX_YUV_NV12) {
    hipLaunchKernelGGL(bgr_to_yuv420_kernel<LMX_YUV_NV12>, dim3(grid_for(total)), dim3(256), 0, st, bgr, pitch_bgr, stride_bgr, a, n, h, w);
    return lmx_launch_check("bgr_to_yuv420_kernel<NV12>");
  }
  hipLaunchKernelGGL(bgr_to_yuv420_kernel<LMX_YUV_I420>, dim3(grid_for(total)), dim3(256), 0, st, bgr, pitch_bgr, stride_bgr, a, n, h, w);
  return lmx_launch_check("bgr_to_yuv420_kernel<I420>");
}
