// tcn_check_main.cpp — the host half of the TCN gait model (csrc/host_image.cpp, host_tcn_image.cpp, host_tcn.cpp) as a stand-alone
// program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_tcn_sanitized.py writes.
//   tcn_check_main check PATH...                 one line per file: "<return code>\t<path>\t<error text>" (the image reader)
//   tcn_check_main score IMAGE POSE T0 S SEED    POSE: T0 x 40 f64 keypoints, T0 x 4 f64 boxes, T0 x i32 keypoint counts.  Prints the
//                                                features' and the keep bits' sums, then the predictions, mean and deviation as hex floats
// The readers report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../vision-sam3-yolo-lameless_amd/csrc/tcn_image.h"

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
  LmxTcnImage img;
  if (lmx_tcn_image_parse(image, &img)) return fail("image");
  // the data section, 64-byte aligned as a device allocation is
  const size_t bytes = (size_t)(img.file_bytes - img.data_offset), room = (bytes + 63) / 64 * 64;
  char* data = static_cast<char*>(aligned_alloc(64, room));
  FILE* f = fopen(image, "rb");
  if (!data || !f || fseek(f, (long)img.data_offset, SEEK_SET) || fread(data, 1, bytes, f) != bytes) return 2;
  fclose(f);
  lmx_tcn_weights_t w;
  lmx_tcn_bind(img, data, &w);

  std::vector<double> kp((size_t)T0 * 40), bbox((size_t)T0 * 4);
  std::vector<int> n_kp((size_t)T0);
  f = fopen(pose, "rb");
  if (!f || fread(kp.data(), 8, kp.size(), f) != kp.size() || fread(bbox.data(), 8, bbox.size(), f) != bbox.size() ||
      fread(n_kp.data(), 4, n_kp.size(), f) != n_kp.size())
    return 2;
  fclose(f);
  const int T = 125, F = LMX_TCN_FEATURES, Smax = S > 0 ? S : 1;
  std::vector<float> x((size_t)T * F), pred((size_t)Smax), trunk((size_t)Smax * T * w.channels[w.n_blocks - 1]);
  float stats[2];
  if (lmx_h_tcn_features(kp.data(), n_kp.data(), bbox.data(), T0, T, x.data())) return fail("features");
  double sum = 0;
  for (float v : x) sum += v;
  printf("features %a\n", sum);
  const int n_sites = 2 * w.n_blocks + 1;
  for (int site = 0; site < n_sites; ++site) {
    std::vector<uint8_t> keep((size_t)T * 64);
    if (lmx_h_tcn_keep_bits(seed, Smax - 1, site, n_sites, (int64_t)keep.size(), img.p, keep.data())) return fail("keep bits");
    long kept = 0;
    for (uint8_t v : keep) kept += v;
    printf("site %d kept %ld\n", site, kept);
  }
  if (lmx_h_tcn_forward(&w, x.data(), &seed, 1, T, S, img.p, pred.data(), stats, trunk.data())) return fail("forward");
  for (float v : pred) printf("pred %a\n", v);
  printf("stats %a %a\n", stats[0], stats[1]);
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && strcmp(argv[1], "check") == 0) {
    for (int i = 2; i < argc; ++i) {
      g_error[0] = 0;
      lmx_tcn_info_t info;
      const int rc = lmx_tcn_image_check_host(argv[i], &info);
      printf("%d\t%s\t%s\n", rc, argv[i], g_error);
    }
    return 0;
  }
  if (argc == 7 && strcmp(argv[1], "score") == 0) return score(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), strtoull(argv[6], nullptr, 10));
  fprintf(stderr, "usage: %s check PATH... | score IMAGE POSE T0 S SEED\n", argv[0]);
  return 2;
}
