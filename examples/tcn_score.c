/* tcn_score.c — a lameness severity score and its MC-dropout uncertainty from a pose series in plain C: no Python, no HIP code of the
 * caller's own.
 *
 *   cc -O2 -Iinclude examples/tcn_score.c -o tcn_score -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./tcn_score model.lmx pose.bin seed [n_samples]
 *
 * model.lmx   a weight image, exported once from Python: lmx.native.write_tcn_image(cfg, folded, "model.lmx") with
 *             cfg, folded = lmx.checkpoints.tcn_from_state_dict(torch.load("tcn_lameness.pt"))
 * pose.bin    int32 T0 (little-endian), then T0 x 20 x 2 float64 keypoints (x, y), T0 x 4 float64 boxes (x0, y0, x1, y1) and
 *             T0 int32 keypoint counts: the `pose_sequences` of a `{id}_tleap.json`
 * seed        the clip's 64-bit dropout seed in decimal; the service uses the first 8 bytes of SHA-256(video_id), little-endian
 * Prints what services/tcn-pipeline/app/main.py:355-364 computes for the clip: 125 steps of 44 features, ten samples by default.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

enum { STEPS = 125, FEATURES = 44 };

static int fail(const char* what) {
  fprintf(stderr, "tcn_score: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.lmx pose.bin seed [n_samples]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[3], NULL, 10);
  const int S = argc > 4 ? atoi(argv[4]) : 10;
  lmx_tcn_info_t info;
  if (lmx_tcn_image_check_host(argv[1], &info) != LMX_OK) return fail("lmx_tcn_image_check_host");
  if (info.input_dim != FEATURES) {
    fprintf(stderr, "tcn_score: the model takes %d features per step, a pose series has %d\n", info.input_dim, FEATURES);
    return 1;
  }

  FILE* f = fopen(argv[2], "rb");
  int32_t T0 = 0;
  if (!f || fread(&T0, sizeof(T0), 1, f) != 1 || T0 <= 0) {
    fprintf(stderr, "tcn_score: %s: no int32 frame count\n", argv[2]);
    return 1;
  }
  double* kp = (double*)malloc((size_t)T0 * 40 * sizeof(double));
  double* bbox = (double*)malloc((size_t)T0 * 4 * sizeof(double));
  int* n_kp = (int*)malloc((size_t)T0 * sizeof(int));
  if (!kp || !bbox || !n_kp || fread(kp, sizeof(double), (size_t)T0 * 40, f) != (size_t)T0 * 40 ||
      fread(bbox, sizeof(double), (size_t)T0 * 4, f) != (size_t)T0 * 4 || fread(n_kp, sizeof(int), (size_t)T0, f) != (size_t)T0) {
    fprintf(stderr, "tcn_score: %s: fewer than %d pose frames\n", argv[2], T0);
    return 1;
  }
  fclose(f);

  static float x[STEPS * FEATURES];
  if (lmx_h_tcn_features(kp, n_kp, bbox, T0, STEPS, x) != LMX_OK) return fail("lmx_h_tcn_features");
  float* pred = (float*)malloc((size_t)(S > 0 ? S : 1) * sizeof(float));
  float stats[2];
  lmx_tcn* model = NULL;
  if (!pred || lmx_tcn_open_host(argv[1], /*max_clips=*/1, /*max_samples=*/S > 2 ? S : 2, &model) != LMX_OK) return fail("lmx_tcn_open_host");
  if (lmx_tcn_score_host(model, x, &seed, 1, STEPS, S, pred, stats) != LMX_OK) {
    lmx_tcn_close(model);
    return fail("lmx_tcn_score_host");
  }
  lmx_tcn_close(model);
  printf("tcn_score: %d pose frames -> %d steps, receptive field %d, %d samples\n", T0, STEPS, info.receptive_field, S);
  printf("severity_score %.9g\nuncertainty %.9g\nprediction %d\n", stats[0], stats[1], stats[0] > 0.5f);
  free(kp);
  free(bbox);
  free(n_kp);
  free(pred);
  return 0;
}
