// host_crop.cpp — the crop box of a clip, video-preprocessing main.py:86-110 on the host (include/lmx.h at lmx_h_crop_box;
// lmx/services/preprocessing.py crop_box_of is the same arithmetic in Python, tests/test_preprocessing_host.py holds the two together):
// boxes above 10 % of the frame, np.median per float32 column, int() truncation, the padding, the clamp, and the full frame when
// nothing qualifies.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define CROP_REQUIRE(cond, ...)   \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

extern "C" int lmx_h_crop_box(const float* boxes_host, int k, int h, int w, int pad, int32_t* box_host) {
  CROP_REQUIRE(k >= 0, "lmx_h_crop_box: k = %d boxes", k);
  CROP_REQUIRE(h >= 1 && w >= 1, "lmx_h_crop_box: a frame of %d x %d (h x w)", h, w);
  CROP_REQUIRE(pad >= 0, "lmx_h_crop_box: pad = %d", pad);
  CROP_REQUIRE(box_host != nullptr && (k == 0 || boxes_host != nullptr), "lmx_h_crop_box: null pointer (%s)", !box_host ? "box_host" : "boxes_host");
  const double floor_area = (double)w * (double)h * 0.1;  // width * height * 0.1 of Python floats
  std::vector<float> col[4];
  for (int i = 0; i < k; ++i) {
    const float* b = boxes_host + 4 * (int64_t)i;
    const volatile float bw = b[2] - b[0], bh = b[3] - b[1];
    const volatile float area = bw * bh;  // float32 products and differences, as numpy's scalars
    if ((double)area > floor_area)
      for (int c = 0; c < 4; ++c) col[c].push_back(b[c]);
  }
  if (col[0].empty()) {
    box_host[0] = box_host[1] = 0;
    box_host[2] = w;
    box_host[3] = h;
    return LMX_OK;
  }
  int32_t med[4];
  for (int c = 0; c < 4; ++c) {
    std::sort(col[c].begin(), col[c].end());
    const size_t m = col[c].size();
    const volatile float sum = col[c][(m - 1) / 2] + col[c][m / 2];  // np.median: the mean of the two middle values in float32 (an odd count: a + a)
    const float v = m % 2 ? col[c][m / 2] : sum / 2.0f;
    med[c] = (int32_t)v;  // int(): towards zero
  }
  box_host[0] = std::max(0, med[0] - pad);
  box_host[1] = std::max(0, med[1] - pad);
  box_host[2] = std::min(w, med[2] + pad);
  box_host[3] = std::min(h, med[3] + pad);
  return LMX_OK;
}
