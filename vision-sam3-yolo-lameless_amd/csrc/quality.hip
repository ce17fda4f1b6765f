// quality.hip — what clip-curation's compute_blur_score and compute_brightness_score (main.py:276-289) reduce a frame to, for every frame
// of a batch in one pass: out[i] = { Σ g, Σ lap, Σ lap², h * w } of frame i's 8-bit gray image g and its ksize-1 Laplacian under
// BORDER_REFLECT_101.  HBM-bound byte work: 3 bytes read per pixel, 32 bytes written per frame, so the figure of merit is 3 B/px over
// time (profiles/frame_quality.txt).  The arithmetic is include/lmx.h's text at lmx_k_frame_quality (PARITY UNPINNED against real
// OpenCV); csrc/host_quality.cpp restates it in plain C++.
//
// thread = a run of 16 columns of one row, 48 bytes: three 16-byte loads where the run is whole and its address aligned, byte loads
// otherwise, decided per run.  wave = a strip of 64 runs (1024 columns) that walks a band of RB rows downwards with the gray values of
// the row above, the row itself and the row below in registers and the bytes of the row after that in flight, so a source byte is
// fetched once — but for one halo row above and below each band, and for the one-pixel column halo: a lane takes it from its
// neighbours' registers (two shuffles per row); the first lane of a strip, its last lane and the lane that holds the row's end read
// theirs from memory (the border's reflection included).  No LDS, no workspace.  The four waves of a workgroup are independent.
// Gray values sit two to a register in 16-bit halves: the neighbours of a pair are v_alignbit of adjacent registers, the Laplacian
// is packed 16-bit adds (|lap| <= 1020) and the three sums are v_dot2 instructions: a third fewer VALU instructions in the row loop and
// 108 instead of 120 VGPRs than with one value per register — and the same time on frames that come from HBM (252 us against 250 for
// 150 frames of 1080p, profiles/frame_quality_rocprof.txt): what the kernel waits for is its loads, not its arithmetic.
//
// Sums: a thread adds at most RB * 16 = 512 pixels of a band into 32-bit registers — Σ g <= 512 * 255, |Σ lap| <= 512 * 1020 and
// Σ lap² <= 512 * 1 040 400 = 532 684 800 < 2^31 (|lap| <= 4 * 255; an int32 holds 2063 such squares, which is what bounds RB at 128).
// The wave's Σ g and Σ lap stay below 64 * 512 * 1020 < 2^25 and are reduced in 32 bits, Σ lap² in 64; lane 0 adds the three to out[i]
// with 64-bit integer atomics, on words the call itself zeroes on the stream.  Integer sums throughout: the result does not depend on
// the launch geometry, on n or on the order in which the waves arrive.
#include "common.h"
#include "quality.h"

namespace {

constexpr int BW = 16;           // columns of a thread's run
constexpr int SW = 64 * BW;      // columns of a wave's strip
constexpr int RB = 32;           // rows of a band
constexpr int WAVES = 4;         // per workgroup
static_assert(RB * BW <= 2063, "a thread's 32-bit sum of squares");

// the 48 bytes of a run (zero where the run ends early or the lane has none) and, in the lanes that read them, the halo pixels left
// and right of the run as B | G << 8 | R << 16
struct Raw {
  unsigned d[12];
  unsigned hl, hr;
};
// the gray values of a run, p[j] = g[2j] | g[2j + 1] << 16, and of the pixels left and right of it
struct Gray {
  unsigned p[BW / 2];
  unsigned l, r;
};
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s(unsigned v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ u16x2 as_u(unsigned v) { return __builtin_bit_cast(u16x2, v); }
// which of its halo pixels a lane reads from memory, and where (columns of the frame)
struct Halo {
  bool mem_l, mem_r;
  int xl, xr;
};

__device__ __forceinline__ int reflect101(int i, int size) { return i < 0 ? -i : (i >= size ? 2 * size - 2 - i : i); }

__device__ __forceinline__ int gray(unsigned b, unsigned g, unsigned r) {
  return (int)((LMX_GRAY_CB * b + LMX_GRAY_CG * g + LMX_GRAY_CR * r + (1u << (LMX_GRAY_SHIFT - 1))) >> LMX_GRAY_SHIFT);
}

__device__ __forceinline__ unsigned byte_of(const unsigned (&d)[12], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 255u; }

__device__ __forceinline__ unsigned pixel_at(const uint8_t* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

// row: the first byte of a frame's row; the run starts at column x0 and has cnt (0 .. 16) columns
__device__ __forceinline__ Raw load_run(const uint8_t* row, int x0, int cnt, const Halo& hx) {
  Raw r;
#pragma unroll
  for (int j = 0; j < 12; ++j) r.d[j] = 0u;
  r.hl = r.hr = 0u;
  if (cnt > 0) {
    const uint8_t* p = row + 3 * x0;
    if (cnt == BW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const u32x4 v = reinterpret_cast<const u32x4*>(p)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) r.d[4 * q + j] = v[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3 * BW; ++i)
        if (i < 3 * cnt) r.d[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
    if (hx.mem_l) r.hl = pixel_at(row + 3 * hx.xl);
    if (hx.mem_r) r.hr = pixel_at(row + 3 * hx.xr);
  }
  return r;
}

// every lane of the wave calls this together (the shuffles)
__device__ __forceinline__ Gray to_gray(const Raw& r, int cnt, const Halo& hx) {
  Gray o;
#pragma unroll
  for (int j = 0; j < BW / 2; ++j) {
    const int i = 2 * j;
    const unsigned lo = (unsigned)gray(byte_of(r.d, 3 * i), byte_of(r.d, 3 * i + 1), byte_of(r.d, 3 * i + 2));
    const unsigned hi = (unsigned)gray(byte_of(r.d, 3 * i + 3), byte_of(r.d, 3 * i + 4), byte_of(r.d, 3 * i + 5));
    o.p[j] = lo | (hi << 16);
  }
  const unsigned from_l = (unsigned)__shfl_up((int)o.p[BW / 2 - 1], 1, 64) >> 16, from_r = (unsigned)__shfl_down((int)o.p[0], 1, 64) & 0xffffu;
  o.l = hx.mem_l ? (unsigned)gray(r.hl & 255u, (r.hl >> 8) & 255u, r.hl >> 16) : from_l;
  o.r = hx.mem_r ? (unsigned)gray(r.hr & 255u, (r.hr >> 8) & 255u, r.hr >> 16) : from_r;
  if (cnt == 0) o.l = o.r = 0u;  // a lane without columns adds zeros
  return o;
}

// the row c between the rows u and d, two pixels per register in 16-bit halves (|lap| <= 1020).  TAIL: some lane of the wave has
// 0 < cnt < 16 columns: its run ends at the halo, which is put behind its last column, and the columns beyond are masked out
template <bool TAIL>
__device__ __forceinline__ void add_row(const Gray& u, const Gray& c, const Gray& d, int cnt, int& s0, int& s1, unsigned& s2) {
  unsigned cp[BW / 2], m[BW / 2];
#pragma unroll
  for (int j = 0; j < BW / 2; ++j) {
    cp[j] = c.p[j];
    if (TAIL) {
      if (cnt == 2 * j) cp[j] = (cp[j] & 0xffff0000u) | c.r;
      if (cnt == 2 * j + 1) cp[j] = (cp[j] & 0xffffu) | (c.r << 16);
      m[j] = (2 * j < cnt ? 1u : 0u) | (2 * j + 1 < cnt ? 0x10000u : 0u);
    }
  }
  const unsigned ones = 0x10001u;
  int q = (int)s2;
#pragma unroll
  for (int j = 0; j < BW / 2; ++j) {
    const unsigned lw = j == 0 ? (c.l << 16) : cp[j - 1], rw = j == BW / 2 - 1 ? c.r : cp[j + 1];
    const unsigned left = __builtin_amdgcn_alignbit(cp[j], lw, 16), right = __builtin_amdgcn_alignbit(rw, cp[j], 16);
    s16x2 lap = as_s(u.p[j]) + as_s(d.p[j]) + as_s(left) + as_s(right) - as_s(cp[j]) * (short)4;
    if (TAIL) {
      const s16x2 lm = lap * as_s(m[j]);
      s0 = (int)__builtin_amdgcn_udot2(as_u(cp[j]), as_u(m[j]), (unsigned)s0, false);
      s1 = __builtin_amdgcn_sdot2(lm, as_s(ones), s1, false);
      q = __builtin_amdgcn_sdot2(lm, lap, q, false);
    } else {
      s0 = (int)__builtin_amdgcn_udot2(as_u(cp[j]), as_u(ones), (unsigned)s0, false);
      s1 = __builtin_amdgcn_sdot2(lap, as_s(ones), s1, false);
      q = __builtin_amdgcn_sdot2(lap, lap, q, false);
    }
  }
  s2 = (unsigned)q;
}

__global__ __launch_bounds__(64 * WAVES) void frame_quality_kernel(const uint8_t* __restrict__ bgr, int64_t units, int h, int w, int bands, int strips,
                                                                    unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t unit = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); unit < units; unit += (int64_t)gridDim.x * WAVES) {  // wave-uniform
    const int strip = (int)(unit % strips);
    const int64_t rest = unit / strips;
    const int band = (int)(rest % bands);
    const int64_t img = rest / bands;
    const int x0 = strip * SW + lane * BW;
    const int cnt = w - x0 < 0 ? 0 : (w - x0 < BW ? w - x0 : BW);
    const bool last = x0 + cnt >= w;  // the run reaches the row's end
    const Halo hx{cnt > 0 && lane == 0, cnt > 0 && (lane == 63 || last), x0 == 0 ? 1 : x0 - 1, last ? w - 2 : x0 + BW};
    const bool tail = __any(cnt > 0 && cnt < BW);
    const int y0 = band * RB, rows = h - y0 < RB ? h - y0 : RB;
    const uint8_t* frame = bgr + img * ((int64_t)h * w * 3);
    // source rows y0 - 1 .. y0 + rows, reflected at the frame's border, as k = 0 .. rows + 1
    const auto row_at = [&](int k) { return frame + (int64_t)reflect101(y0 - 1 + k, h) * w * 3; };

    Gray up = to_gray(load_run(row_at(0), x0, cnt, hx), cnt, hx);
    Gray mid = to_gray(load_run(row_at(1), x0, cnt, hx), cnt, hx);
    Raw raw = load_run(row_at(2), x0, cnt, hx);
    int s0 = 0, s1 = 0;
    unsigned s2 = 0u;
    for (int k = 2; k <= rows + 1; ++k) {
      Raw next = raw;
      if (k <= rows) next = load_run(row_at(k + 1), x0, cnt, hx);  // in flight while this row is added
      const Gray down = to_gray(raw, cnt, hx);
      if (tail)
        add_row<true>(up, mid, down, cnt, s0, s1, s2);
      else
        add_row<false>(up, mid, down, cnt, s0, s1, s2);
      up = mid;
      mid = down;
      raw = next;
    }

    unsigned long long q = s2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o, 64);
      s1 += __shfl_xor(s1, o, 64);
      q += __shfl_xor(q, o, 64);
    }
    if (lane == 0) {
      unsigned long long* o = out + 4 * img;
      atomicAdd(o + 0, (unsigned long long)(long long)s0);
      atomicAdd(o + 1, (unsigned long long)(long long)s1);  // two's complement: the 64-bit sum of the signed values
      atomicAdd(o + 2, q);
      if (band == 0 && strip == 0) o[3] = (unsigned long long)((int64_t)h * w);  // no other wave touches this word
    }
  }
}

}  // namespace

extern "C" int64_t lmx_frame_quality_workspace_bytes(int n, int h, int w) {
  (void)n, (void)h, (void)w;
  return 0;  // the partial sums meet in `out` itself
}

extern "C" int lmx_k_frame_quality(const uint8_t* bgr, int n, int h, int w, int64_t* out, void* workspace, lmx_stream_t stream) {
  (void)workspace;
  LMX_TRY(lmx_quality_check("lmx_k_frame_quality", bgr, n, h, w, out));
  LMX_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "lmx_k_frame_quality: out must be 8-byte aligned");
  if (n == 0) return LMX_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_HIP(hipMemsetAsync(out, 0, (size_t)n * 32, st));
  const int bands = (h + RB - 1) / RB, strips = (w + SW - 1) / SW;
  const int64_t units = (int64_t)n * bands * strips;
  int64_t grid = (units + WAVES - 1) / WAVES;
  if (grid > (1 << 20)) grid = 1 << 20;
  hipLaunchKernelGGL(frame_quality_kernel, dim3((unsigned)grid), dim3(64 * WAVES), 0, st, bgr, units, h, w, bands, strips,
                     reinterpret_cast<unsigned long long*>(out));
  return lmx_launch_check("frame_quality_kernel");
}
