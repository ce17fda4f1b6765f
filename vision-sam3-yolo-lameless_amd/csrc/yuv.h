// yuv.h — what the device kernel (yuv.hip) and its host restatement (host_yuv.cpp) of the YUV 4:2:0 -> BGR conversion share: the two
// coefficient sets and the argument checks; each file writes the pixel arithmetic itself.  The arithmetic is defined by INTEGRATION.md ("Frames from a decoder"):
// limited range, 20-bit fixed point, nearest chroma — the public integer form of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420).  cv2 is not
// installed here: PARITY UNPINNED against real OpenCV (and swscale).  Plain C++, no HIP: host_yuv.cpp is compiled by g++.
// Below them, the same for the crop window (lmx_*_yuv420_to_bgr_roi) and for the way back to an encoder (lmx_*_bgr_to_yuv420): the
// window's checks, the second coefficient table and the checks of the writable descriptor.
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

// ---- the crop window and the way back to an encoder (INTEGRATION.md "Frames to an encoder, and the crop in between") -----------------
// a window of an h x w frame: lmx_k_ / lmx_h_yuv420_to_bgr_roi and lmx_fused_step_yuv_roi
inline int lmx_yuv_check_roi(const char* fn, const lmx_rect_t* r, int h, int w) {
  LMX_YUV_REQUIRE(r != nullptr, "%s: null window (roi_host)", fn);
  LMX_YUV_REQUIRE(r->w >= 1 && r->h >= 1, "%s: roi is empty: w = %d, h = %d", fn, r->w, r->h);
  LMX_YUV_REQUIRE(r->x >= 0 && r->y >= 0 && (int64_t)r->x + r->w <= w && (int64_t)r->y + r->h <= h,
                  "%s: roi (x = %d, y = %d, w = %d, h = %d) is outside the %d x %d frame", fn, r->x, r->y, r->w, r->h, h, w);
  return LMX_OK;
}

// BGR -> YUV 4:2:0, limited range, 20-bit fixed point, chroma from the 2 x 2 sums (22-bit shift): int(round(c * 2^20)) of
// 0.098 0.504 0.257 | 0.439 -0.291 -0.148 | -0.071 -0.368 0.439 (BT.601) and 0.062 0.614 0.183 | 0.439 -0.338 -0.101 | -0.040 -0.399 0.439
// (BT.709).  Both chroma rows sum to 0.
struct LmxYuvOutCoef {
  int32_t yb, yg, yr, ub, ug, ur, vb, vg, vr;
};
inline LmxYuvOutCoef lmx_yuv_out_coef(int matrix) {
  return matrix == LMX_YUV_BT709 ? LmxYuvOutCoef{65012, 643826, 191889, 460325, -354419, -105906, -41943, -418382, 460325}
                                 : LmxYuvOutCoef{102760, 528482, 269484, 460325, -305136, -155189, -74449, -385876, 460325};
}

// the checks of lmx_k_ / lmx_h_bgr_to_yuv420: the pitched BGR source and the writable descriptor
inline int lmx_yuv_check_out(const char* fn, const void* bgr, int64_t pitch_bgr, const lmx_yuv_out_t* o, int n, int h, int w) {
  LMX_YUV_REQUIRE(o != nullptr, "%s: null descriptor (out_host)", fn);
  if (const int rc = lmx_yuv_check_format(fn, o->layout, o->matrix, n, h, w)) return rc;
  LMX_YUV_REQUIRE(pitch_bgr >= 3 * (int64_t)w, "%s: pitch_bgr = %lld is below the BGR row of %lld bytes", fn, (long long)pitch_bgr, 3 * (long long)w);
  if (o->layout == LMX_YUV_NV12)
    LMX_YUV_REQUIRE(o->v == nullptr, "%s: NV12 takes the interleaved chroma plane in u; v must be NULL", fn);
  else
    LMX_YUV_REQUIRE(o->v != nullptr, "%s: I420 needs the v plane", fn);
  const int64_t row_c = o->layout == LMX_YUV_NV12 ? w : w / 2;
  LMX_YUV_REQUIRE(o->pitch_y >= w, "%s: pitch_y = %lld is below the luma row of %d bytes", fn, (long long)o->pitch_y, w);
  LMX_YUV_REQUIRE(o->pitch_c >= row_c, "%s: pitch_c = %lld is below the chroma row of %lld bytes", fn, (long long)o->pitch_c, (long long)row_c);
  LMX_YUV_REQUIRE(n == 0 || (bgr != nullptr && o->y != nullptr && o->u != nullptr), "%s: null pointer (%s)", fn, !bgr ? "bgr" : !o->y ? "y" : "u");
  return LMX_OK;
}
