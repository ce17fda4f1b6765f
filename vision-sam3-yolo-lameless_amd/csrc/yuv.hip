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
