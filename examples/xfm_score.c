/* xfm_score.c — the gait transformer's severity score, MC-dropout uncertainty and temporal saliency from a pose series in plain C: no
 * Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/xfm_score.c -o xfm_score -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./xfm_score model.lmx pose.bin seed [n_samples]
 *
 * model.lmx   a weight image, exported once from Python: lmx.native.write_xfm_image(cfg, weights, "model.lmx") with
 *             cfg, weights = lmx.checkpoints.xfm_from_state_dict(torch.load("transformer_lameness.pt"))
 * pose.bin    int32 T0 (little-endian), then T0 x 20 x 2 float64 keypoints (x, y), T0 x 4 float64 boxes (x0, y0, x1, y1), T0 int32
 *             keypoint counts, T0 x 20 float64 keypoint confidences and T0 float64 detection confidences: the `pose_sequences` of a
 *             `{id}_tleap.json`
 * seed        the clip's 64-bit dropout seed in decimal; the service uses the first 8 bytes of SHA-256(video_id), little-endian
 * Prints what services/transformer-pipeline/app/main.py:419-441 computes for the clip: 125 steps of 44 features with the confidence
 * mask, ten samples by default, then the saliency of the unmasked eval run (its first 20 values).
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

enum { STEPS = 125, FEATURES = 44, SHOWN = 20 };

static int fail(const char* what) {
  fprintf(stderr, "xfm_score: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.lmx pose.bin seed [n_samples]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[3], NULL, 10);
  const int S = argc > 4 ? atoi(argv[4]) : 10;
  lmx_xfm_info_t info;
  if (lmx_xfm_image_check_host(argv[1], &info) != LMX_OK) return fail("lmx_xfm_image_check_host");
  if (info.input_dim != FEATURES || info.max_len < STEPS) {
    fprintf(stderr, "xfm_score: the model takes %d features and up to %d steps, a pose series has %d and %d\n", info.input_dim, info.max_len,
            FEATURES, STEPS);
    return 1;
  }

  FILE* f = fopen(argv[2], "rb");
  int32_t T0 = 0;
  if (!f || fread(&T0, sizeof(T0), 1, f) != 1 || T0 <= 0) {
    fprintf(stderr, "xfm_score: %s: no int32 frame count\n", argv[2]);
    return 1;
  }
  const size_t n = (size_t)T0;
  double* kp = (double*)malloc(n * 40 * sizeof(double));
  double* bbox = (double*)malloc(n * 4 * sizeof(double));
  int* n_kp = (int*)malloc(n * sizeof(int));
  double* conf = (double*)malloc(n * 20 * sizeof(double));
  double* det = (double*)malloc(n * sizeof(double));
  if (!kp || !bbox || !n_kp || !conf || !det || fread(kp, sizeof(double), n * 40, f) != n * 40 || fread(bbox, sizeof(double), n * 4, f) != n * 4 ||
      fread(n_kp, sizeof(int), n, f) != n || fread(conf, sizeof(double), n * 20, f) != n * 20 || fread(det, sizeof(double), n, f) != n) {
    fprintf(stderr, "xfm_score: %s: fewer than %d pose frames\n", argv[2], T0);
    return 1;
  }
  fclose(f);

  static float x[STEPS * FEATURES], saliency[STEPS];
  static uint8_t mask[STEPS];
  if (lmx_h_tcn_features(kp, n_kp, bbox, T0, STEPS, x) != LMX_OK) return fail("lmx_h_tcn_features");
  if (lmx_h_xfm_mask(conf, n_kp, det, T0, STEPS, mask) != LMX_OK) return fail("lmx_h_xfm_mask");
  int masked = 0;
  for (int t = 0; t < STEPS; ++t) masked += mask[t];
  if (masked == STEPS) {
    fprintf(stderr, "xfm_score: every step is masked (low confidence): no score\n");
    return 1;
  }
  float* pred = (float*)malloc((size_t)(S > 0 ? S : 1) * sizeof(float));
  float stats[2], eval_pred, eval_stats[2];
  lmx_xfm* model = NULL;
  if (!pred || lmx_xfm_open_host(argv[1], /*max_clips=*/1, /*max_samples=*/S > 2 ? S : 2, &model) != LMX_OK) return fail("lmx_xfm_open_host");
  /* the score with the mask, then the saliency in eval mode without it, as the service does */
  if (lmx_xfm_score_host(model, x, mask, &seed, 1, STEPS, S, pred, stats, NULL) != LMX_OK ||
      lmx_xfm_score_host(model, x, NULL, NULL, 1, STEPS, 0, &eval_pred, eval_stats, saliency) != LMX_OK) {
    lmx_xfm_close(model);
    return fail("lmx_xfm_score_host");
  }
  lmx_xfm_close(model);
  printf("xfm_score: %d pose frames -> %d steps, %d masked, %d samples\n", T0, STEPS, masked, S);
  printf("severity_score %.9g\nuncertainty %.9g\nprediction %d\ntemporal_saliency", stats[0], stats[1], stats[0] > 0.5f);
  for (int t = 0; t < SHOWN; ++t) printf(" %.9g", saliency[t]);
  printf("\n");
  free(kp);
  free(bbox);
  free(n_kp);
  free(conf);
  free(det);
  free(pred);
  return 0;
}
