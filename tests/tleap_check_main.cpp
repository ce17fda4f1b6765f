// tleap_check_main.cpp — the host half of the pose series (csrc/host_tleap.cpp over host_tcn.cpp's lmx_h_tcn_features and host_xfm.cpp's
// lmx_h_xfm_mask) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the file
// tests/test_tleap_sanitized.py writes.
//   tleap_check_main INPUT MODE K NDIM F MAX_DET H W N TARGET N_COW
// INPUT: boxes f32 [F][MAX_DET][4], scores f32 [F][MAX_DET], cls i32 [F][MAX_DET], counts i32 [F], kpts f32 [F][MAX_DET][K][NDIM] (MODE 0
// only), clip_first i32 [N + 1], cow classes i32 [N_COW].  Every buffer is a heap block of exactly the length include/lmx.h states.
// Prints per clip its rows, every record, per step the sum of its 44 features (added in doubles, in order) and the mask, then the
// locomotion features of the clip's records under the mode's keypoint names: floats as hex.
#include "../vision-sam3-yolo-lameless_amd/csrc/tleap.h"
#include "check_main.h"

static const char* const kHeuristic[20] = {"left_eye", "right_eye", "nose", "left_ear", "right_ear", "left_front_elbow", "right_front_elbow",
                                           "left_back_elbow", "right_back_elbow", "left_front_knee", "right_front_knee", "left_back_knee",
                                           "right_back_knee", "left_front_paw", "right_front_paw", "left_back_paw", "right_back_paw", "throat",
                                           "withers", "tailbase"};
static const char* const kTrained[20] = {"left_ear_base", "neck", "withers", "mid_back", "right_hind_hip", "right_hind_mid_leg", "right_hind_fetlock",
                                         "left_hind_shoulder", "left_hind_mid_leg", "left_hind_fetlock", "right_front_shoulder", "right_front_mid_leg",
                                         "right_front_lower_leg", "left_front_shoulder", "left_front_mid_leg", "left_front_lower_leg",
                                         "right_front_hoof", "left_front_hoof", "right_hind_hoof", "left_hind_hoof"};

template <class T>
static T* block(FILE* f, size_t count) {  // exactly `count` values from the file, or an empty block for count 0
  T* p = static_cast<T*>(malloc(count ? count * sizeof(T) : 1));
  if (!p || fread(p, sizeof(T), count, f) != count) exit(2);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 12) {
    fprintf(stderr, "usage: %s INPUT MODE K NDIM F MAX_DET H W N TARGET N_COW\n", argv[0]);
    return 2;
  }
  const int mode = atoi(argv[2]), K = atoi(argv[3]), ndim = atoi(argv[4]), F = atoi(argv[5]), md = atoi(argv[6]), h = atoi(argv[7]), w = atoi(argv[8]),
            n = atoi(argv[9]), target = atoi(argv[10]), n_cow = atoi(argv[11]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const size_t D = (size_t)F * md;
  float* boxes = block<float>(f, D * 4);
  float* scores = block<float>(f, D);
  int32_t* cls = block<int32_t>(f, D);
  int32_t* counts = block<int32_t>(f, (size_t)F);
  float* kpts = mode == LMX_TLEAP_TRAINED ? block<float>(f, D * K * ndim) : nullptr;
  int32_t* first = block<int32_t>(f, (size_t)n + 1);
  int32_t* cow = block<int32_t>(f, (size_t)n_cow);
  fclose(f);
  int32_t* rows = static_cast<int32_t*>(malloc(sizeof(int32_t) * n));
  lmx_tleap_record_t* rec = static_cast<lmx_tleap_record_t*>(malloc(sizeof(lmx_tleap_record_t) * D));
  float* series = static_cast<float*>(malloc(sizeof(float) * n * target * LMX_GAIT_FEATURES));
  uint8_t* mask = static_cast<uint8_t*>(malloc((size_t)n * target));
  if (lmx_h_tleap_series(boxes, scores, cls, counts, kpts, K, ndim, F, md, h, w, first, n, target, mode, cow, n_cow, rows, rec, series, mask))
    return fail("series");
  for (int c = 0; c < n; ++c) {
    printf("rows %d %d\n", c, rows[c]);
    const lmx_tleap_record_t* r = rec + (size_t)first[c] * md;
    for (int i = 0; i < rows[c]; ++i) {
      printf("rec %d %d %d %a %a %a %a %a", r[i].frame, r[i].det, r[i].n_kp, r[i].bbox[0], r[i].bbox[1], r[i].bbox[2], r[i].bbox[3], r[i].confidence);
      for (int k = 0; k < LMX_TLEAP_KEYPOINTS; ++k) printf(" %a %a %a", r[i].keypoints[k][0], r[i].keypoints[k][1], r[i].keypoints[k][2]);
      printf("\n");
    }
    for (int s = 0; s < target; ++s) {
      double sum = 0;
      for (int j = 0; j < LMX_GAIT_FEATURES; ++j) sum += series[((size_t)c * target + s) * LMX_GAIT_FEATURES + j];
      printf("step %d %a\n", mask[(size_t)c * target + s], sum);
    }
    lmx_tleap_locomotion_t loco;
    // an exactly-sized copy of the clip's records: a read past rows[c] is a report
    lmx_tleap_record_t* own = static_cast<lmx_tleap_record_t*>(malloc(rows[c] ? sizeof(lmx_tleap_record_t) * rows[c] : 1));
    memcpy(own, r, sizeof(lmx_tleap_record_t) * rows[c]);
    if (lmx_h_tleap_locomotion(own, rows[c], mode == LMX_TLEAP_TRAINED ? kTrained : kHeuristic, &loco)) return fail("locomotion");
    free(own);
    printf("loco %u", loco.present);
    const double* v = &loco.back_arch_mean;
    for (int i = 0; i < 17; ++i) printf(" %a", v[i]);
    printf("\n");
  }
  free(boxes), free(scores), free(cls), free(counts), free(kpts), free(first), free(cow), free(rows), free(rec), free(series), free(mask);
  return 0;
}
