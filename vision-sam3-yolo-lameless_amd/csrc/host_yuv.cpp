// host_yuv.cpp — HOST restatement of csrc/yuv.hip: YUV 4:2:0 (NV12 / I420) -> packed BGR u8, one pixel at a time, straight from the
// text at lmx_k_yuv420_to_bgr in include/lmx.h (limited range, 20-bit fixed point, nearest chroma: the public integer form of
// cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420)).  cv2 is not installed here: PARITY UNPINNED against real OpenCV.  It makes the formula
// testable without a GPU (tests/test_yuv_host.py) and is what a stand-alone check program runs (tests/yuv_check_main.cpp).
#include <stdint.h>

#include "yuv.h"

namespace {

// the shift of the text is an arithmetic one (floor); >> on a negative int is that on every compiler this builds with
inline uint8_t sat8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

}  // namespace

extern "C" int lmx_h_yuv420_to_bgr(const lmx_yuv_frames_t* frames_host, int n, int h, int w, uint8_t* bgr_host) {
  if (const int rc = lmx_yuv_check("lmx_h_yuv420_to_bgr", frames_host, n, h, w)) return rc;
  LMX_YUV_REQUIRE(n == 0 || bgr_host != nullptr, "lmx_h_yuv420_to_bgr: null pointer (bgr_host)");
  const lmx_yuv_frames_t& f = *frames_host;
  const LmxYuvCoef k = lmx_yuv_coef(f.matrix);
  const int32_t half = 1 << (LMX_YUV_SHIFT - 1);
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* yp = f.y + i * f.stride_y;
    const uint8_t* up = f.u + i * f.stride_c;
    const uint8_t* vp = f.layout == LMX_YUV_I420 ? f.v + i * f.stride_c : nullptr;
    uint8_t* out = bgr_host + i * (int64_t)h * w * 3;
    for (int y = 0; y < h; ++y) {
      for (int x = 0; x < w; ++x) {
        const int32_t Y = yp[(int64_t)y * f.pitch_y + x];
        int32_t U, V;
        if (f.layout == LMX_YUV_NV12) {
          const uint8_t* c = up + (int64_t)(y >> 1) * f.pitch_c + 2 * (x >> 1);
          U = c[0];
          V = c[1];
        } else {
          const int64_t off = (int64_t)(y >> 1) * f.pitch_c + (x >> 1);
          U = up[off];
          V = vp[off];
        }
        const int32_t yy = (Y - 16 < 0 ? 0 : Y - 16) * k.cy, u = U - 128, v = V - 128;
        uint8_t* d = out + ((int64_t)y * w + x) * 3;
        d[0] = sat8((yy + k.cub * u + half) >> LMX_YUV_SHIFT);
        d[1] = sat8((yy + k.cug * u + k.cvg * v + half) >> LMX_YUV_SHIFT);
        d[2] = sat8((yy + k.cvr * v + half) >> LMX_YUV_SHIFT);
      }
    }
  }
  return LMX_OK;
}
