// yuv.h — what the device kernel (yuv.hip) and its host restatement (host_yuv.cpp) of the YUV 4:2:0 -> BGR conversion share: the two
// coefficient sets and the argument checks; each file writes the pixel arithmetic itself.  The arithmetic is defined by INTEGRATION.md ("Frames from a decoder"):
// limited range, 20-bit fixed point, nearest chroma — the public integer form of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420).  cv2 is not
// installed here: PARITY UNPINNED against real OpenCV (and swscale).  Plain C++, no HIP: host_yuv.cpp is compiled by g++.
#pragma once
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

const int LMX_YUV_SHIFT = 20;

// int(round(c * 2^20)) of the three-decimal constants: 1.164 | 2.018, -0.391, -0.813, 1.596 (BT.601, cv2's) | 2.112, -0.213, -0.533, 1.793 (BT.709)
struct LmxYuvCoef {
  int32_t cy, cub, cug, cvg, cvr;
};
inline LmxYuvCoef lmx_yuv_coef(int matrix) {
  return matrix == LMX_YUV_BT709 ? LmxYuvCoef{1220542, 2214593, -223347, -558891, 1880097} : LmxYuvCoef{1220542, 2116026, -409993, -852492, 1673527};
}

#define LMX_YUV_REQUIRE(cond, ...) \
  do {                             \
    if (!(cond)) {                 \
      lmx_set_error(__VA_ARGS__);  \
      return LMX_EINVAL;           \
    }                              \
  } while (0)

// what is served: 4:2:0 frames of even sizes in one of the two layouts under one of the two matrices (`fn`: the entry point's name)
inline int lmx_yuv_check_format(const char* fn, int layout, int matrix, int n, int h, int w) {
  LMX_YUV_REQUIRE(n >= 0, "%s: n = %d frames", fn, n);
  LMX_YUV_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "%s: 4:2:0 frames have even sizes of 2 or more, not %d x %d", fn, h, w);
  LMX_YUV_REQUIRE(layout == LMX_YUV_NV12 || layout == LMX_YUV_I420, "%s: layout %d is neither LMX_YUV_NV12 (0) nor LMX_YUV_I420 (1)", fn, layout);
  LMX_YUV_REQUIRE(matrix == LMX_YUV_BT601 || matrix == LMX_YUV_BT709, "%s: matrix %d is neither LMX_YUV_BT601 (0) nor LMX_YUV_BT709 (1)", fn, matrix);
  return LMX_OK;
}

// the checks of a descriptor: lmx_k_yuv420_to_bgr, lmx_h_yuv420_to_bgr and lmx_fused_step_yuv
inline int lmx_yuv_check(const char* fn, const lmx_yuv_frames_t* f, int n, int h, int w) {
  LMX_YUV_REQUIRE(f != nullptr, "%s: null descriptor (frames_host)", fn);
  if (const int rc = lmx_yuv_check_format(fn, f->layout, f->matrix, n, h, w)) return rc;
  if (f->layout == LMX_YUV_NV12)
    LMX_YUV_REQUIRE(f->v == nullptr, "%s: NV12 takes the interleaved chroma plane in u; v must be NULL", fn);
  else
    LMX_YUV_REQUIRE(f->v != nullptr, "%s: I420 needs the v plane", fn);
  const int64_t row_c = f->layout == LMX_YUV_NV12 ? w : w / 2;
  LMX_YUV_REQUIRE(f->pitch_y >= w, "%s: pitch_y = %lld is below the luma row of %d bytes", fn, (long long)f->pitch_y, w);
  LMX_YUV_REQUIRE(f->pitch_c >= row_c, "%s: pitch_c = %lld is below the chroma row of %lld bytes", fn, (long long)f->pitch_c, (long long)row_c);
  LMX_YUV_REQUIRE(n == 0 || (f->y != nullptr && f->u != nullptr), "%s: null pointer (%s)", fn, !f->y ? "y" : "u");
  return LMX_OK;
}
