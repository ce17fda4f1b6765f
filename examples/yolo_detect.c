/* yolo_detect.c — YOLOv8 detections from raw frames in plain C: no Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/yolo_detect.c -o yolo_detect -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./yolo_detect model.lmx frames.raw detections.bin [max_batch]
 *
 * model.lmx       a weight image, exported once from Python: lmx.native.write_yolo_image(detector, "model.lmx")
 * frames.raw      int32 n, h, w (little-endian), then n * h * w * 3 bytes: BGR frames as cv2 delivers them
 * detections.bin  receives what `self.yolo_model(frame, verbose=False, conf=0.25)` yields per frame
 *                 (services/yolo-pipeline/app/main.py:76), at most 300 detections each: counts int32 [n], then boxes float32
 *                 [n][300][4] (xyxy in frame pixels), scores float32 [n][300], cls int32 [n][300]; rows past a frame's count are
 *                 zero.  A pose image appends keypoints float32 [n][300][K][ndim] (services/tleap-pipeline/app/main.py:150).
 * The exact plan is used when the image holds it (the detector's default), the f16 plan otherwise.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

#define MAX_DET 300

static int fail(const char* what) {
  fprintf(stderr, "yolo_detect: %s: %s\n", what, lmx_last_error());
  return 1;
}

static int put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.lmx frames.raw detections.bin [max_batch]\n", argv[0]);
    return 2;
  }
  const int max_batch = argc > 4 ? atoi(argv[4]) : 8;
  lmx_yolo_info_t info;
  if (lmx_yolo_image_check_host(argv[1], &info) != LMX_OK) return fail("lmx_yolo_image_check_host");
  const int precision = (info.plans & (1 << LMX_YOLO_EXACT)) ? LMX_YOLO_EXACT : LMX_YOLO_F16;

  FILE* f = fopen(argv[2], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) {
    fprintf(stderr, "yolo_detect: %s: no int32 n, h, w header\n", argv[2]);
    return 1;
  }
  const int n = hdr[0], h = hdr[1], w = hdr[2];
  const size_t bytes = (size_t)n * h * w * 3, rows = (size_t)n * MAX_DET, kp = rows * (size_t)info.kpt_k * (size_t)info.kpt_ndim;
  uint8_t* frames = (uint8_t*)malloc(bytes);
  float* boxes = (float*)malloc(rows * 4 * sizeof(float));
  float* scores = (float*)malloc(rows * sizeof(float));
  int32_t* cls = (int32_t*)malloc(rows * sizeof(int32_t));
  int32_t* src = (int32_t*)malloc(rows * sizeof(int32_t));
  int32_t* counts = (int32_t*)malloc((size_t)n * sizeof(int32_t));
  float* kpts = kp ? (float*)malloc(kp * sizeof(float)) : NULL;
  if (!frames || !boxes || !scores || !cls || !src || !counts || (kp && !kpts) || fread(frames, 1, bytes, f) != bytes) {
    fprintf(stderr, "yolo_detect: %s: fewer than %d frames of %d x %d\n", argv[2], n, h, w);
    return 1;
  }
  fclose(f);

  lmx_yolo* model = NULL;
  if (lmx_yolo_open_host(argv[1], max_batch, &model) != LMX_OK) return fail("lmx_yolo_open_host");
  if (lmx_yolo_detect_host(model, frames, n, h, w, precision, 0.25f, 0.7, MAX_DET, boxes, scores, cls, src, counts, kpts) != LMX_OK) {
    lmx_yolo_close(model);
    return fail("lmx_yolo_detect_host");
  }
  int total = 0;
  for (int i = 0; i < n; ++i) {
    total += counts[i];
    for (int j = 0; j < counts[i] && j < 3; ++j) {
      const size_t r = (size_t)i * MAX_DET + (size_t)j;
      const char* name = lmx_yolo_class_name(model, cls[r]);
      printf("frame %d: %s %.3f [%.1f %.1f %.1f %.1f]\n", i, name ? name : "?", scores[r], boxes[4 * r], boxes[4 * r + 1], boxes[4 * r + 2],
             boxes[4 * r + 3]);
    }
  }
  lmx_yolo_close(model);

  f = fopen(argv[3], "wb");
  if (!f || !put(f, counts, (size_t)n * sizeof(int32_t)) || !put(f, boxes, rows * 4 * sizeof(float)) || !put(f, scores, rows * sizeof(float)) ||
      !put(f, cls, rows * sizeof(int32_t)) || !put(f, kpts, kp * sizeof(float)) || fclose(f) != 0) {
    fprintf(stderr, "yolo_detect: cannot write %s\n", argv[3]);
    return 1;
  }
  printf("yolo_detect: %d frames of %d x %d -> %d detections (yolov8%c, %d classes, %s plan)\n", n, h, w, total, (char)info.scale, info.nc,
         precision == LMX_YOLO_EXACT ? "exact" : "f16");
  free(frames);
  free(boxes);
  free(scores);
  free(cls);
  free(src);
  free(counts);
  free(kpts);
  return 0;
}
