/* tleap_gait.c — from a clip's frames to its two gait scores and its locomotion features in plain C, with no host arithmetic between the
 * detector and the scores: lmx_yolo_detect leaves its outputs in HBM, lmx_k_tleap_series turns them into tleap's pose records, the
 * 125 x 44 series and the key-padding mask where they lie (services/tleap-pipeline/app/main.py:142-313 and :479-486), lmx_tcn_score and
 * lmx_xfm_score read the series and the mask from there, and lmx_h_tleap_locomotion (main.py:338-436) runs on the downloaded records.
 * The buffers live on the device, so this example calls the HIP runtime itself.
 *
 *   cc -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/tleap_gait.c -o tleap_gait \
 *      -Lvision-sam3-yolo-lameless_amd/lmx -llmx -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx
 *   ./tleap_gait yolo.lmx tcn.lmx xfm.lmx frames.raw seed [conf]
 *
 * yolo.lmx    a weight image of lmx.native.write_yolo_image: with a Pose head the model type is `trained`, without one `heuristic`
 *             (the classes whose name contains "cow", and id 19, are cows)
 * tcn.lmx, xfm.lmx   weight images of lmx.native.write_tcn_image / write_xfm_image
 * frames.raw  int32 n, h, w (little-endian), then n * h * w * 3 bytes: the clip's SAMPLED frames, BGR as cv2 delivers them
 * seed        the clip's 64-bit dropout seed in decimal; the services use the first 8 bytes of SHA-256(video_id), little-endian
 * conf        the detector's confidence, 0.3 as tleap-pipeline sets it
 * Prints the rows, the two severity scores with their spreads (hex floats too: they are the bits the Python services write), and the
 * locomotion features that exist.  A trained model's keypoint names match only `withers`, so a trained clip has none: the reference's
 * quirk. */
#include <ctype.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lmx.h"

enum { MAX_DET = 300, STEPS = 125, FEATURES = 44, SAMPLES = 10 };

static const char* const HEURISTIC_NAMES[20] = {"left_eye", "right_eye", "nose", "left_ear", "right_ear", "left_front_elbow", "right_front_elbow",
                                                "left_back_elbow", "right_back_elbow", "left_front_knee", "right_front_knee", "left_back_knee",
                                                "right_back_knee", "left_front_paw", "right_front_paw", "left_back_paw", "right_back_paw", "throat",
                                                "withers", "tailbase"};
static const char* const TRAINED_NAMES[20] = {"left_ear_base", "neck", "withers", "mid_back", "right_hind_hip", "right_hind_mid_leg",
                                              "right_hind_fetlock", "left_hind_shoulder", "left_hind_mid_leg", "left_hind_fetlock",
                                              "right_front_shoulder", "right_front_mid_leg", "right_front_lower_leg", "left_front_shoulder",
                                              "left_front_mid_leg", "left_front_lower_leg", "right_front_hoof", "left_front_hoof", "right_hind_hoof",
                                              "left_hind_hoof"};
static const char* const FEATURE_NAMES[17] = {"back_arch_mean", "back_arch_std", "back_arch_score", "head_bob_magnitude", "head_bob_frequency",
                                              "head_bob_score", "stride_fl_mean", "stride_fl_std", "stride_fr_mean", "stride_fr_std", "stride_rl_mean",
                                              "stride_rl_std", "stride_rr_mean", "stride_rr_std", "front_leg_asymmetry", "rear_leg_asymmetry",
                                              "lameness_score"};

static int fail(const char* what) {
  fprintf(stderr, "tleap_gait: %s: %s\n", what, lmx_last_error());
  return 1;
}

static int hip_fail(const char* what, hipError_t e) {
  fprintf(stderr, "tleap_gait: %s: %s\n", what, hipGetErrorString(e));
  return 1;
}

#define HIP(call)                                     \
  do {                                                \
    const hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hip_fail(#call, e_); \
  } while (0)

static int names_cow(const char* name) {
  char low[64];
  size_t i = 0;
  for (; name && name[i] && i + 1 < sizeof(low); ++i) low[i] = (char)tolower((unsigned char)name[i]);
  low[i] = 0;
  return strstr(low, "cow") != NULL;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s yolo.lmx tcn.lmx xfm.lmx frames.raw seed [conf]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[5], NULL, 10);
  const float conf = argc > 6 ? (float)atof(argv[6]) : 0.3f;
  lmx_yolo_info_t yinfo;
  if (lmx_yolo_image_check_host(argv[1], &yinfo) != LMX_OK) return fail("lmx_yolo_image_check_host");
  const int precision = (yinfo.plans & (1 << LMX_YOLO_EXACT)) ? LMX_YOLO_EXACT : LMX_YOLO_F16;
  const int trained = yinfo.kpt_k > 0;

  FILE* f = fopen(argv[4], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) {
    fprintf(stderr, "tleap_gait: %s: no int32 n, h, w header\n", argv[4]);
    return 1;
  }
  const int n = hdr[0], h = hdr[1], w = hdr[2];
  const size_t bytes = (size_t)n * h * w * 3, dets = (size_t)n * MAX_DET;
  uint8_t* frames_host = (uint8_t*)malloc(bytes);
  if (!frames_host || fread(frames_host, 1, bytes, f) != bytes) {
    fprintf(stderr, "tleap_gait: %s: fewer than %d frames of %d x %d\n", argv[4], n, h, w);
    return 1;
  }
  fclose(f);

  /* 1. the detector: its outputs stay on the device */
  uint8_t* frames;
  float *boxes, *scores, *kpts = NULL;
  int32_t *cls, *src, *counts;
  HIP(hipMalloc((void**)&frames, bytes));
  HIP(hipMalloc((void**)&boxes, dets * 4 * sizeof(float)));
  HIP(hipMalloc((void**)&scores, dets * sizeof(float)));
  HIP(hipMalloc((void**)&cls, dets * sizeof(int32_t)));
  HIP(hipMalloc((void**)&src, dets * sizeof(int32_t)));
  HIP(hipMalloc((void**)&counts, (size_t)n * sizeof(int32_t)));
  if (trained) HIP(hipMalloc((void**)&kpts, dets * (size_t)yinfo.kpt_k * (size_t)yinfo.kpt_ndim * sizeof(float)));
  HIP(hipMemcpy(frames, frames_host, bytes, hipMemcpyHostToDevice));
  lmx_yolo* yolo = NULL;
  if (lmx_yolo_open_host(argv[1], n < 8 ? n : 8, &yolo) != LMX_OK) return fail("lmx_yolo_open_host");
  if (lmx_yolo_detect(yolo, frames, n, h, w, precision, conf, 0.7, MAX_DET, boxes, scores, cls, src, counts, kpts, NULL) != LMX_OK)
    return fail("lmx_yolo_detect");
  int32_t cows[LMX_TLEAP_MAX_COW_CLASSES];
  int n_cow = 0;
  cows[n_cow++] = 19; /* main.py:282 */
  for (int c = 0; c < yinfo.nc && n_cow < LMX_TLEAP_MAX_COW_CLASSES; ++c)
    if (c != 19 && names_cow(lmx_yolo_class_name(yolo, c))) cows[n_cow++] = c;

  /* 2. the pose series, on the same buffers: one clip of n frames */
  const int32_t clip_first[2] = {0, n};
  const int64_t ws_bytes = lmx_tleap_workspace_bytes(n, MAX_DET);
  int32_t* rows;
  lmx_tleap_record_t* records;
  float* series;
  uint8_t* mask;
  void* workspace;
  if (ws_bytes == 0) return fail("lmx_tleap_workspace_bytes");
  HIP(hipMalloc((void**)&rows, sizeof(int32_t)));
  HIP(hipMalloc((void**)&records, dets * sizeof(lmx_tleap_record_t)));
  HIP(hipMalloc((void**)&series, (size_t)STEPS * FEATURES * sizeof(float)));
  HIP(hipMalloc((void**)&mask, STEPS));
  HIP(hipMalloc(&workspace, (size_t)ws_bytes));
  if (lmx_k_tleap_series(boxes, scores, cls, counts, kpts, yinfo.kpt_k, yinfo.kpt_ndim, n, MAX_DET, h, w, clip_first, 1, STEPS,
                         trained ? LMX_TLEAP_TRAINED : LMX_TLEAP_HEURISTIC, trained ? NULL : cows, trained ? 0 : n_cow, rows, records, series, mask,
                         workspace, NULL) != LMX_OK)
    return fail("lmx_k_tleap_series");
  int32_t T0 = 0;
  uint8_t mask_host[STEPS];
  HIP(hipMemcpy(&T0, rows, sizeof(T0), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(mask_host, mask, STEPS, hipMemcpyDeviceToHost));
  int masked = 0;
  for (int t = 0; t < STEPS; ++t) masked += mask_host[t];
  printf("model_type %s\nframes %d\nrows %d\nmasked_steps %d\n", trained ? "trained" : "heuristic", n, T0, masked);

  /* 3. the two gait models, on the series and the mask where they lie */
  float *pred, *stats;
  float stats_host[2];
  HIP(hipMalloc((void**)&pred, SAMPLES * sizeof(float)));
  HIP(hipMalloc((void**)&stats, 2 * sizeof(float)));
  if (T0 > 0) {
    lmx_tcn* tcn = NULL;
    if (lmx_tcn_open_host(argv[2], 1, SAMPLES, &tcn) != LMX_OK) return fail("lmx_tcn_open_host");
    if (lmx_tcn_score(tcn, series, &seed, 1, STEPS, SAMPLES, pred, stats, NULL) != LMX_OK) return fail("lmx_tcn_score");
    HIP(hipMemcpy(stats_host, stats, sizeof(stats_host), hipMemcpyDeviceToHost));
    lmx_tcn_close(tcn);
    printf("tcn severity_score %.9g uncertainty %.9g bits %a %a\n", stats_host[0], stats_host[1], stats_host[0], stats_host[1]);
  }
  if (T0 > 0 && masked < STEPS) { /* every step masked: no defined score, the service refuses the clip */
    lmx_xfm* xfm = NULL;
    if (lmx_xfm_open_host(argv[3], 1, SAMPLES, &xfm) != LMX_OK) return fail("lmx_xfm_open_host");
    if (lmx_xfm_score(xfm, series, mask, &seed, 1, STEPS, SAMPLES, pred, stats, NULL, NULL) != LMX_OK) return fail("lmx_xfm_score");
    HIP(hipMemcpy(stats_host, stats, sizeof(stats_host), hipMemcpyDeviceToHost));
    lmx_xfm_close(xfm);
    printf("transformer severity_score %.9g uncertainty %.9g bits %a %a\n", stats_host[0], stats_host[1], stats_host[0], stats_host[1]);
  }

  /* 4. the locomotion features, from the downloaded records */
  lmx_tleap_record_t* rec_host = (lmx_tleap_record_t*)malloc((T0 > 0 ? (size_t)T0 : 1) * sizeof(lmx_tleap_record_t));
  if (!rec_host) return 1;
  if (T0 > 0) HIP(hipMemcpy(rec_host, records, (size_t)T0 * sizeof(lmx_tleap_record_t), hipMemcpyDeviceToHost));
  lmx_tleap_locomotion_t loco;
  if (lmx_h_tleap_locomotion(rec_host, T0, trained ? TRAINED_NAMES : HEURISTIC_NAMES, &loco) != LMX_OK) return fail("lmx_h_tleap_locomotion");
  const double values[17] = {loco.back_arch_mean, loco.back_arch_std, loco.back_arch_score, loco.head_bob_magnitude, loco.head_bob_frequency,
                             loco.head_bob_score, loco.stride_fl_mean, loco.stride_fl_std, loco.stride_fr_mean, loco.stride_fr_std,
                             loco.stride_rl_mean, loco.stride_rl_std, loco.stride_rr_mean, loco.stride_rr_std, loco.front_leg_asymmetry,
                             loco.rear_leg_asymmetry, loco.lameness_score};
  for (int i = 0; i < 17; ++i)
    if (loco.present >> i & 1u) printf("%s %.17g\n", FEATURE_NAMES[i], values[i]);

  lmx_yolo_close(yolo);
  free(rec_host);
  free(frames_host);
  hipFree(frames), hipFree(boxes), hipFree(scores), hipFree(cls), hipFree(src), hipFree(counts), hipFree(kpts), hipFree(rows), hipFree(records);
  hipFree(series), hipFree(mask), hipFree(workspace), hipFree(pred), hipFree(stats);
  return 0;
}
