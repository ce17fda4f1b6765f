/* sam_segment.c — SAM masks from raw frames and boxes in plain C: no Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/sam_segment.c -o sam_segment -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./sam_segment model.lmx frames.raw masks.bin [max_batch]
 *
 * model.lmx    a weight image, exported once from Python: lmx.native.write_sam_image(encoder, decoder, "model.lmx")
 * frames.raw   int32 n, h, w (little-endian), then n * h * w * 3 bytes: the frames as the service hands them to set_image (BGR, as cv2
 *              delivers them), then float32 [n][4]: one box per frame, xyxy in frame pixels (all zero: no detection)
 * masks.bin    receives what `predictor.set_image(frame); predictor.predict(box=..., multimask_output=False)` yields per frame
 *              (services/sam3-pipeline/app/main.py:74-92): mask bits uint8 [n][h][ceil(w/8)] (numpy.packbits order), then stats
 *              int64 [n][8] (area, sum x, sum y, min x, min y, max x, max y, 0), then the predicted IoU float32 [n]
 * The exact plan is used when the image holds it (the services' plan), the f16 plan otherwise.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "sam_segment: %s: %s\n", what, lmx_last_error());
  return 1;
}

static int put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.lmx frames.raw masks.bin [max_batch]\n", argv[0]);
    return 2;
  }
  const int max_batch = argc > 4 ? atoi(argv[4]) : 4;
  lmx_sam_info_t info;
  if (lmx_sam_image_check_host(argv[1], &info) != LMX_OK) return fail("lmx_sam_image_check_host");
  const int precision = (info.plans & (1 << LMX_SAM_EXACT)) ? LMX_SAM_EXACT : LMX_SAM_F16;

  FILE* f = fopen(argv[2], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) {
    fprintf(stderr, "sam_segment: %s: no int32 n, h, w header\n", argv[2]);
    return 1;
  }
  const int n = hdr[0], h = hdr[1], w = hdr[2];
  const size_t bytes = (size_t)n * h * w * 3, bits_bytes = (size_t)n * h * (((size_t)w + 7) / 8);
  uint8_t* frames = (uint8_t*)malloc(bytes);
  float* boxes = (float*)malloc((size_t)n * 4 * sizeof(float));
  uint8_t* bits = (uint8_t*)malloc(bits_bytes);
  int64_t* stats = (int64_t*)malloc((size_t)n * 8 * sizeof(int64_t));
  float* iou = (float*)malloc((size_t)n * sizeof(float));
  if (!frames || !boxes || !bits || !stats || !iou || fread(frames, 1, bytes, f) != bytes || fread(boxes, 4 * sizeof(float), (size_t)n, f) != (size_t)n) {
    fprintf(stderr, "sam_segment: %s: fewer than %d frames of %d x %d with a box each\n", argv[2], n, h, w);
    return 1;
  }
  fclose(f);

  lmx_sam* model = NULL;
  if (lmx_sam_open_host(argv[1], max_batch, &model) != LMX_OK) return fail("lmx_sam_open_host");
  /* the byte mask, the contour features and the low-resolution logits are not asked for: NULL */
  if (lmx_sam_segment_host(model, frames, n, h, w, boxes, precision, NULL, bits, stats, NULL, iou, NULL) != LMX_OK) {
    lmx_sam_close(model);
    return fail("lmx_sam_segment_host");
  }
  lmx_sam_close(model);
  for (int i = 0; i < n; ++i)
    printf("frame %d: box [%.1f %.1f %.1f %.1f] -> mask of %lld pixels, predicted IoU %.3f\n", i, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2],
           boxes[4 * i + 3], (long long)stats[8 * i], iou[i]);

  f = fopen(argv[3], "wb");
  if (!f || !put(f, bits, bits_bytes) || !put(f, stats, (size_t)n * 8 * sizeof(int64_t)) || !put(f, iou, (size_t)n * sizeof(float)) || fclose(f) != 0) {
    fprintf(stderr, "sam_segment: cannot write %s\n", argv[3]);
    return 1;
  }
  printf("sam_segment: %d frames of %d x %d (ViT %d wide, %d layers, %s plan)\n", n, h, w, info.hidden, info.layers,
         precision == LMX_SAM_EXACT ? "exact" : "f16");
  free(frames);
  free(boxes);
  free(bits);
  free(stats);
  free(iou);
  return 0;
}
