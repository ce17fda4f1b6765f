// host_quality.cpp — HOST restatement of csrc/quality.hip: per frame the sums { Σ g, Σ lap, Σ lap², h * w } of the 8-bit gray image and its
// ksize-1 Laplacian, one pixel at a time, straight from the text at lmx_k_frame_quality in include/lmx.h (what compute_blur_score and
// compute_brightness_score of clip-curation main.py:276-289 reduce a frame to).  cv2 is not installed here: PARITY UNPINNED against real
// OpenCV.  It makes the formula testable without a GPU (tests/test_frame_quality_host.py).
#include <stdint.h>

#include "quality.h"

namespace {

// BORDER_REFLECT_101: -1 -> 1, size -> size - 2 (size >= 2, one step outside at most)
inline int reflect101(int i, int size) { return i < 0 ? -i : (i >= size ? 2 * size - 2 - i : i); }

inline int32_t gray(const uint8_t* px) {
  return (LMX_GRAY_CB * (int32_t)px[0] + LMX_GRAY_CG * (int32_t)px[1] + LMX_GRAY_CR * (int32_t)px[2] + (1 << (LMX_GRAY_SHIFT - 1))) >> LMX_GRAY_SHIFT;
}

}  // namespace

extern "C" int lmx_h_frame_quality(const uint8_t* bgr_host, int n, int h, int w, int64_t* out_host) {
  if (const int rc = lmx_quality_check("lmx_h_frame_quality", bgr_host, n, h, w, out_host)) return rc;
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* f = bgr_host + i * (int64_t)h * w * 3;
    const auto g = [&](int y, int x) { return gray(f + ((int64_t)reflect101(y, h) * w + reflect101(x, w)) * 3); };
    int64_t s0 = 0, s1 = 0, s2 = 0;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const int32_t c = g(y, x), lap = g(y, x - 1) + g(y, x + 1) + g(y - 1, x) + g(y + 1, x) - 4 * c;
        s0 += c;
        s1 += lap;
        s2 += (int64_t)lap * lap;
      }
    int64_t* o = out_host + 4 * i;
    o[0] = s0, o[1] = s1, o[2] = s2, o[3] = (int64_t)h * w;
  }
  return LMX_OK;
}
