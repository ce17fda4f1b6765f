// host_yuv.cpp — HOST restatement of csrc/yuv.hip: YUV 4:2:0 (NV12 / I420) -> packed BGR u8, one pixel at a time, straight from the
// text at lmx_k_yuv420_to_bgr in include/lmx.h (limited range, 20-bit fixed point, nearest chroma: the public integer form of
// cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420)).  cv2 is not installed here: PARITY UNPINNED against real OpenCV.  It makes the formula
// testable without a GPU (tests/test_yuv_host.py) and is what a stand-alone check program runs (tests/yuv_check_main.cpp).
// Behind it the window form (lmx_h_yuv420_to_bgr_roi: the same pixel at (x + i, y + j)) and the way back, lmx_h_bgr_to_yuv420 (limited
// range, 20-bit fixed point, chroma from the 2 x 2 sums), from the texts beside them in include/lmx.h (tests/test_yuv_egress_host.py,
// tests/yuv_egress_check_main.cpp).
#include <stdint.h>

#include "yuv.h"

namespace {

// the shift of the text is an arithmetic one (floor); >> on a negative int is that on every compiler this builds with
inline uint8_t sat8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// pixel (x, y) of frame planes yp / up / vp by the text: one definition for the whole frame and for a window
inline void pixel_bgr(const lmx_yuv_frames_t& f, const LmxYuvCoef& k, const uint8_t* yp, const uint8_t* up, const uint8_t* vp, int x, int y, uint8_t* d) {
  const int32_t half = 1 << (LMX_YUV_SHIFT - 1);
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
  d[0] = sat8((yy + k.cub * u + half) >> LMX_YUV_SHIFT);
  d[1] = sat8((yy + k.cug * u + k.cvg * v + half) >> LMX_YUV_SHIFT);
  d[2] = sat8((yy + k.cvr * v + half) >> LMX_YUV_SHIFT);
}

void window_bgr(const lmx_yuv_frames_t& f, int n, const lmx_rect_t& r, uint8_t* bgr_host) {
  const LmxYuvCoef k = lmx_yuv_coef(f.matrix);
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* yp = f.y + i * f.stride_y;
    const uint8_t* up = f.u + i * f.stride_c;
    const uint8_t* vp = f.layout == LMX_YUV_I420 ? f.v + i * f.stride_c : nullptr;
    uint8_t* out = bgr_host + i * (int64_t)r.h * r.w * 3;
    for (int y = 0; y < r.h; ++y)
      for (int x = 0; x < r.w; ++x) pixel_bgr(f, k, yp, up, vp, r.x + x, r.y + y, out + ((int64_t)y * r.w + x) * 3);
  }
}

}  // namespace

extern "C" int lmx_h_yuv420_to_bgr(const lmx_yuv_frames_t* frames_host, int n, int h, int w, uint8_t* bgr_host) {
  if (const int rc = lmx_yuv_check("lmx_h_yuv420_to_bgr", frames_host, n, h, w)) return rc;
  LMX_YUV_REQUIRE(n == 0 || bgr_host != nullptr, "lmx_h_yuv420_to_bgr: null pointer (bgr_host)");
  window_bgr(*frames_host, n, lmx_rect_t{0, 0, w, h}, bgr_host);
  return LMX_OK;
}

extern "C" int lmx_h_yuv420_to_bgr_roi(const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host, uint8_t* bgr_host) {
  if (const int rc = lmx_yuv_check("lmx_h_yuv420_to_bgr_roi", frames_host, n, h, w)) return rc;
  if (const int rc = lmx_yuv_check_roi("lmx_h_yuv420_to_bgr_roi", roi_host, h, w)) return rc;
  LMX_YUV_REQUIRE(n == 0 || bgr_host != nullptr, "lmx_h_yuv420_to_bgr_roi: null pointer (bgr_host)");
  window_bgr(*frames_host, n, *roi_host, bgr_host);
  return LMX_OK;
}

extern "C" int lmx_h_bgr_to_yuv420(const uint8_t* bgr_host, int64_t pitch_bgr, int64_t stride_bgr, int n, int h, int w, const lmx_yuv_out_t* out_host) {
  if (const int rc = lmx_yuv_check_out("lmx_h_bgr_to_yuv420", bgr_host, pitch_bgr, out_host, n, h, w)) return rc;
  const lmx_yuv_out_t& o = *out_host;
  const LmxYuvOutCoef k = lmx_yuv_out_coef(o.matrix);
  const int32_t half_y = 1 << (LMX_YUV_SHIFT - 1), half_c = 1 << (LMX_YUV_SHIFT + 1);
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* src = bgr_host + i * stride_bgr;
    uint8_t* yp = o.y + i * o.stride_y;
    uint8_t* up = o.u + i * o.stride_c;
    uint8_t* vp = o.layout == LMX_YUV_I420 ? o.v + i * o.stride_c : nullptr;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const uint8_t* p = src + (int64_t)y * pitch_bgr + 3 * (int64_t)x;
        yp[(int64_t)y * o.pitch_y + x] = sat8(((k.yb * p[0] + k.yg * p[1] + k.yr * p[2] + half_y) >> LMX_YUV_SHIFT) + 16);
      }
    for (int j = 0; j < h / 2; ++j)
      for (int c = 0; c < w / 2; ++c) {
        int32_t s[3] = {0, 0, 0};
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx) {
            const uint8_t* p = src + (int64_t)(2 * j + dy) * pitch_bgr + 3 * (int64_t)(2 * c + dx);
            s[0] += p[0];
            s[1] += p[1];
            s[2] += p[2];
          }
        const uint8_t U = sat8(((k.ub * s[0] + k.ug * s[1] + k.ur * s[2] + half_c) >> (LMX_YUV_SHIFT + 2)) + 128);
        const uint8_t V = sat8(((k.vb * s[0] + k.vg * s[1] + k.vr * s[2] + half_c) >> (LMX_YUV_SHIFT + 2)) + 128);
        if (o.layout == LMX_YUV_NV12) {
          uint8_t* d = up + (int64_t)j * o.pitch_c + 2 * c;
          d[0] = U;
          d[1] = V;
        } else {
          up[(int64_t)j * o.pitch_c + c] = U;
          vp[(int64_t)j * o.pitch_c + c] = V;
        }
      }
  }
  return LMX_OK;
}
