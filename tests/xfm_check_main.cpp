// xfm_check_main.cpp — the host half of the gait transformer (csrc/host_image.cpp, host_xfm_image.cpp, host_xfm.cpp and, for the
// features, host_tcn.cpp) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files
// tests/test_xfm_sanitized.py writes.
//   xfm_check_main check PATH...                 one line per file: "<return code>\t<path>\t<error text>" (the image reader)
//   xfm_check_main score IMAGE POSE T0 S SEED    POSE: T0 x 40 f64 keypoints, T0 x 4 f64 boxes, T0 x i32 keypoint counts, T0 x 20 f64
//                                                keypoint confidences, T0 x f64 detection confidences.  Prints the features' sum, the
//                                                number of masked steps, the predictions, mean and deviation and (S = 0) the saliency
//                                                as hex floats
// The readers report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/xfm_image.h"
#include "check_main.h"

static int score(const char* image, const char* pose, int T0, int S, uint64_t seed) {
  LmxXfmImage img;
  if (lmx_xfm_image_parse(image, &img)) return fail("image");
  char* data = load_data(image, img.data_offset, img.file_bytes);
  if (!data) return 2;
  lmx_xfm_weights_t w;
  lmx_xfm_bind(img, data, &w);

  std::vector<double> kp, bbox, conf((size_t)T0 * 20), det((size_t)T0);
  std::vector<int> n_kp;
  FILE* f = open_pose(pose, T0, kp, bbox, n_kp);
  if (!f || !read_all(f, conf) || !read_all(f, det)) return 2;
  fclose(f);
  const int T = 125, F = LMX_GAIT_FEATURES, Smax = S > 0 ? S : 1;
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

int main(int argc, char** argv) { return gait_main<lmx_xfm_info_t>(argc, argv, lmx_xfm_image_check_host, score); }
