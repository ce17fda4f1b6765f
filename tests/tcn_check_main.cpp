// tcn_check_main.cpp — the host half of the TCN gait model (csrc/host_image.cpp, host_tcn_image.cpp, host_tcn.cpp) as a stand-alone
// program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_tcn_sanitized.py writes.
//   tcn_check_main check PATH...                 one line per file: "<return code>\t<path>\t<error text>" (the image reader)
//   tcn_check_main score IMAGE POSE T0 S SEED    POSE: T0 x 40 f64 keypoints, T0 x 4 f64 boxes, T0 x i32 keypoint counts.  Prints the
//                                                features' and the keep bits' sums, then the predictions, mean and deviation as hex floats
// The readers report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/tcn_image.h"
#include "check_main.h"

static int score(const char* image, const char* pose, int T0, int S, uint64_t seed) {
  LmxTcnImage img;
  if (lmx_tcn_image_parse(image, &img)) return fail("image");
  char* data = load_data(image, img.data_offset, img.file_bytes);
  if (!data) return 2;
  lmx_tcn_weights_t w;
  lmx_tcn_bind(img, data, &w);

  std::vector<double> kp, bbox;
  std::vector<int> n_kp;
  FILE* f = open_pose(pose, T0, kp, bbox, n_kp);
  if (!f) return 2;
  fclose(f);
  const int T = 125, F = LMX_GAIT_FEATURES, Smax = S > 0 ? S : 1;
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

int main(int argc, char** argv) { return gait_main<lmx_tcn_info_t>(argc, argv, lmx_tcn_image_check_host, score); }
