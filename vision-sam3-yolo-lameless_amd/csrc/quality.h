// quality.h — what the device kernel (quality.hip) and its host restatement (host_quality.cpp) of the per-frame blur / brightness
// sums share: the gray coefficients and the argument checks; each file writes the pixel arithmetic itself.  The arithmetic is the text
// at lmx_k_frame_quality in include/lmx.h (OpenCV 4's 8-bit BGR2GRAY, cv2.Laplacian ksize 1 under BORDER_REFLECT_101, exact int64 sums).
// cv2 is not installed here: PARITY UNPINNED against real OpenCV.  Plain C++, no HIP: host_quality.cpp is compiled by g++.
#pragma once
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

// round(c * 2^15) of 0.114, 0.587, 0.299; g = (CB * B + CG * G + CR * R + 2^14) >> 15.  The three add up to 2^15, so g <= 255
const int LMX_GRAY_CB = 3735, LMX_GRAY_CG = 19235, LMX_GRAY_CR = 9798, LMX_GRAY_SHIFT = 15;
const int LMX_QUALITY_MAX_SIDE = 32768;

#define LMX_QUALITY_REQUIRE(cond, ...) \
  do {                                 \
    if (!(cond)) {                     \
      lmx_set_error(__VA_ARGS__);      \
      return LMX_EINVAL;               \
    }                                  \
  } while (0)

// lmx_k_frame_quality and lmx_h_frame_quality (`fn`: the entry point's name); nothing is read or written before these pass
inline int lmx_quality_check(const char* fn, const void* bgr, int n, int h, int w, const void* out) {
  LMX_QUALITY_REQUIRE(n >= 0, "%s: n = %d frames", fn, n);
  LMX_QUALITY_REQUIRE(h >= 2 && w >= 2, "%s: the reflected border needs sizes of 2 or more, not %d x %d", fn, h, w);
  LMX_QUALITY_REQUIRE(h <= LMX_QUALITY_MAX_SIDE && w <= LMX_QUALITY_MAX_SIDE, "%s: sizes above %d are not served (%d x %d)", fn, LMX_QUALITY_MAX_SIDE, h, w);
  LMX_QUALITY_REQUIRE(n == 0 || (bgr != nullptr && out != nullptr), "%s: null pointer (%s)", fn, !bgr ? "bgr" : "out");
  return LMX_OK;
}
