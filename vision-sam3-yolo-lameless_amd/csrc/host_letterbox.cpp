// host_letterbox.cpp — HOST-side arithmetic of the YOLO predictor, the C++ twins of lmx/letterbox.py and lmx.kernels.split_k_for
// (which stay the restatements the tests pin; tests/test_native_yolo_host.py holds these to their bits):
//   lmx_h_letterbox_geometry   ultralytics LetterBox + the gain / padding ops.scale_boxes re-derives      = letterbox.geometry
//   lmx_h_letterbox_tables     OpenCV's resizeGeneric_ table build, INTER_LINEAR on 8U, for lmx_k_letterbox = letterbox.resize_tables
//   lmx_h_conv_split_k         the split_k of an exact-plan 3 x 3 convolution                             = kernels.split_k_for
// Built with -ffp-contract=off (csrc/Makefile): Python and numpy round after every operation, and so must this file.
#include <math.h>
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define LB_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

namespace {

const int MAX_SIDE = 1 << 20;
const int COEF_SCALE = 1 << 11;  // INTER_RESIZE_COEF_SCALE

// Python's round() on a float: the nearest integer, halves to even — nearbyint in the default rounding mode
int py_round(double x) { return (int)nearbyint(x); }
// Python's % on ints takes the sign of the divisor
int py_mod(int a, int b) {
  const int r = a % b;
  return r < 0 ? r + b : r;
}
double py_min(double a, double b) { return b < a ? b : a; }

// saturate_cast<short>(float): cvRound (half to even), then saturate
int16_t sat16(float v) {
  const float r = rintf(v);
  return (int16_t)(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
}

// letterbox._axis_table: the coordinate in double, narrowed to float32; the fraction arithmetic in float32
void axis_table(int ssize, int dsize, int32_t* ofs, int16_t* coef) {
  const double inv_scale = (double)dsize / (double)ssize;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f = f - (float)s;
    ofs[d] = s;
    const float c0 = 1.0f - f;
    coef[2 * d] = sat16(c0 * (float)COEF_SCALE);
    coef[2 * d + 1] = sat16(f * (float)COEF_SCALE);
  }
}

}  // namespace

extern "C" int lmx_h_letterbox_geometry(int sh, int sw, int imgsz, int stride, int auto_, lmx_letterbox_geo_t* out) {
  LB_REQUIRE(out != nullptr, "lmx_h_letterbox_geometry: out_host is null");
  LB_REQUIRE(sh > 0 && sw > 0 && sh <= MAX_SIDE && sw <= MAX_SIDE, "lmx_h_letterbox_geometry: frame size %d x %d outside 1 .. 2^20", sh, sw);
  LB_REQUIRE(stride > 0, "lmx_h_letterbox_geometry: stride %d", stride);
  LB_REQUIRE(imgsz >= stride && imgsz <= MAX_SIDE, "lmx_h_letterbox_geometry: imgsz %d outside stride %d .. 2^20", imgsz, stride);
  const int new_h = imgsz, new_w = imgsz;
  const double r = py_min((double)new_h / sh, (double)new_w / sw);
  const int rw = py_round(sw * r), rh = py_round(sh * r);
  LB_REQUIRE(rw > 0 && rh > 0, "lmx_h_letterbox_geometry: a %d x %d frame resizes to %d x %d for imgsz %d", sh, sw, rh, rw, imgsz);
  int dwi = new_w - rw, dhi = new_h - rh;
  if (auto_) {
    dwi = py_mod(dwi, stride);
    dhi = py_mod(dhi, stride);
  }
  const double dw = dwi / 2.0, dh = dhi / 2.0;
  const int top = py_round(dh - 0.1), bottom = py_round(dh + 0.1);
  const int left = py_round(dw - 0.1), right = py_round(dw + 0.1);
  const int oh = rh + top + bottom, ow = rw + left + right;
  LB_REQUIRE(top >= 0 && left >= 0 && bottom >= 0 && right >= 0, "lmx_h_letterbox_geometry: negative padding for a %d x %d frame at imgsz %d", sh,
             sw, imgsz);
  // ops.scale_boxes(img1_shape=(oh, ow), boxes, img0_shape=(sh, sw)): gain and pad re-derived from the shapes
  const double gain = py_min((double)oh / sh, (double)ow / sw);
  const double gx = sw * gain, gy = sh * gain;
  out->sh = sh;
  out->sw = sw;
  out->rh = rh;
  out->rw = rw;
  out->top = top;
  out->left = left;
  out->oh = oh;
  out->ow = ow;
  out->gain = gain;
  out->pad_x = (double)py_round((ow - gx) / 2 - 0.1);
  out->pad_y = (double)py_round((oh - gy) / 2 - 0.1);
  return LMX_OK;
}

extern "C" int lmx_h_letterbox_tables(int sh, int sw, int rh, int rw, int32_t* xofs, int16_t* ialpha, int32_t* yofs, int16_t* ibeta) {
  LB_REQUIRE(sh > 0 && sw > 0 && sh <= MAX_SIDE && sw <= MAX_SIDE, "lmx_h_letterbox_tables: source size %d x %d outside 1 .. 2^20", sh, sw);
  LB_REQUIRE(rh > 0 && rw > 0 && rh <= MAX_SIDE && rw <= MAX_SIDE, "lmx_h_letterbox_tables: destination size %d x %d outside 1 .. 2^20", rh, rw);
  LB_REQUIRE(xofs && ialpha && yofs && ibeta, "lmx_h_letterbox_tables: null output (xofs_host, ialpha_host, yofs_host, ibeta_host are all required)");
  axis_table(sw, rw, xofs, ialpha);
  // x: the table build clamps (sx < 0 -> 0, fx = 0; sx >= sw - 1 -> sw - 1, fx = 0); y offsets stay raw: the kernel clips the row index
  for (int d = 0; d < rw; ++d) {
    if (xofs[d] < 0) {
      xofs[d] = 0;
      ialpha[2 * d] = COEF_SCALE;
      ialpha[2 * d + 1] = 0;
    }
    if (xofs[d] >= sw - 1) {
      xofs[d] = sw - 1;
      ialpha[2 * d] = COEF_SCALE;
      ialpha[2 * d + 1] = 0;
    }
  }
  axis_table(sh, rh, yofs, ibeta);
  return LMX_OK;
}

extern "C" int lmx_h_conv_split_k(int64_t px_per_frame, int N, int K, int cin) {
  LB_REQUIRE(px_per_frame > 0 && N > 0 && K > 0 && cin > 0, "lmx_h_conv_split_k: px_per_frame %lld, N %d, K %d, cin %d must be positive",
             (long long)px_per_frame, N, K, cin);
  if (N < 64 || N % 8 || cin % 32) return 1;
  const int64_t tiles1 = ((px_per_frame + 255) / 256) * ((N + 255) / 256);  // tiles one frame contributes
  const int64_t nk = K / 64;
  int64_t s = 8;
  if (nk / 8 < s) s = nk / 8;
  if (32 / tiles1 < s) s = 32 / tiles1;
  return s >= 2 ? (int)s : 1;
}
