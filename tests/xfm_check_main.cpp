// xfm_check_main.cpp — the host half of the gait transformer (csrc/host_image.cpp, host_xfm_image.cpp, host_xfm.cpp and, for the
// features, host_tcn.cpp) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files
// tests/test_xfm_sanitized.py writes.
//   xfm_check_main check PATH...                 one line per file: "<return code>\t<path>\t<error text>" (the image reader)
//   xfm_check_main score IMAGE POSE T0 S SEED    POSE: T0 x 40 f64 keypoints, T0 x 4 f64 boxes, T0 x i32 keypoint counts, T0 x 20 f64
//                                                keypoint confidences, T0 x f64 detection confidences.  Prints the features' sum, the
//                                                number of masked steps, the predictions, mean and deviation and (S = 0) the saliency
//                                                as hex floats
// The readers report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../vision-sam3-yolo-lameless_amd/csrc/xfm_image.h"

static char g_error[512];  // the size of the library's buffer: a long message is cut at the same place

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, g_error);
  return 1;
}

static int score(const char* image, const char* pose, int T0, int S, uint64_t seed) {
  LmxXfmImage img;
  if (lmx_xfm_image_parse(image, &img)) return fail("image");
  // the data section, 64-byte aligned as a device allocation is
  const size_t bytes = (size_t)(img.file_bytes - img.data_offset), room = (bytes + 63) / 64 * 64;
  char* data = static_cast<char*>(aligned_alloc(64, room));
  FILE* f = fopen(image, "rb");
  if (!data || !f || fseek(f, (long)img.data_offset, SEEK_SET) || fread(data, 1, bytes, f) != bytes) return 2;
  fclose(f);
  lmx_xfm_weights_t w;
  lmx_xfm_bind(img, data, &w);

  std::vector<double> kp((size_t)T0 * 40), bbox((size_t)T0 * 4), conf((size_t)T0 * 20), det((size_t)T0);
  std::vector<int> n_kp((size_t)T0);
  f = fopen(pose, "rb");
  if (!f || fread(kp.data(), 8, kp.size(), f) != kp.size() || fread(bbox.data(), 8, bbox.size(), f) != bbox.size() ||
      fread(n_kp.data(), 4, n_kp.size(), f) != n_kp.size() || fread(conf.data(), 8, conf.size(), f) != conf.size() ||
      fread(det.data(), 8, det.size(), f) != det.size())
    return 2;
  fclose(f);
  const int T = 125, F = LMX_TCN_FEATURES, Smax = S > 0 ? S : 1;
  std::vector<float> x((size_t)T * F), pred((size_t)Smax), trunk((size_t)Smax * T * w.d_model), sal((size_t)T);
  std::vector<uint8_t> mask((size_t)T);
  float stats[2];
  if (lmx_h_tcn_features(kp.data(), n_kp.data(), bbox.data(), T0, T, x.data())) return fail("features");
  if (lmx_h_xfm_mask(conf.data(), n_kp.data(), det.data(), T0, T, mask.data())) return fail("mask");
  double sum = 0;
  for (float v : x) sum += v;
  printf("features %a\n", sum);
  long masked = 0;
  for (uint8_t v : mask) masked += v;
  printf("masked %ld\n", masked);
  if (lmx_h_xfm_forward(&w, x.data(), mask.data(), &seed, 1, T, S, img.p, pred.data(), stats, S == 0 ? sal.data() : nullptr, trunk.data()))
    return fail("forward");
  for (float v : pred) printf("pred %a\n", v);
  printf("stats %a %a\n", stats[0], stats[1]);
  if (S == 0)
    for (float v : sal) printf("saliency %a\n", v);
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && strcmp(argv[1], "check") == 0) {
    for (int i = 2; i < argc; ++i) {
      g_error[0] = 0;
      lmx_xfm_info_t info;
      const int rc = lmx_xfm_image_check_host(argv[i], &info);
      printf("%d\t%s\t%s\n", rc, argv[i], g_error);
    }
    return 0;
  }
  if (argc == 7 && strcmp(argv[1], "score") == 0) return score(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), strtoull(argv[6], nullptr, 10));
  fprintf(stderr, "usage: %s check PATH... | score IMAGE POSE T0 S SEED\n", argv[0]);
  return 2;
}
