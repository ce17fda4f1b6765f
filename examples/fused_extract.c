/* fused_extract.c — the fused per-frame path in plain C: detections, the top box's mask with its statistics and contour features, and
 * the DINO embedding of every frame as one fixed-stride record.  No Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/fused_extract.c -o fused_extract -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./fused_extract yolo.lmx sam.lmx dino.lmx frames.raw records.bin [sam_chunk [sam_lanes [conf]]]
 *
 * yolo.lmx, sam.lmx, dino.lmx   weight images, exported once from Python: lmx.native.write_yolo_image / write_sam_image / write_dino_image
 * frames.raw    int32 n, h, w (little-endian), then n * h * w * 3 bytes: BGR frames as cv2 delivers them
 * records.bin   receives the record matrix uint8 [n][stride] (lmx_fused_layout; lmx.dist.unpack_records reads it): per frame what
 *               services/yolo-pipeline/app/main.py:74-76, services/sam3-pipeline/app/main.py:74-92 and :118-135 (prompted with the
 *               first detection, :199-206) and services/dinov3-pipeline/app/main.py:98-113 yield.
 * The exact plan is used when both the YOLO and the SAM image hold it (the models' default), the f16 plan otherwise.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "fused_extract: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s yolo.lmx sam.lmx dino.lmx frames.raw records.bin [sam_chunk [sam_lanes [conf]]]\n", argv[0]);
    return 2;
  }
  const int sam_chunk = argc > 6 ? atoi(argv[6]) : 16, sam_lanes = argc > 7 ? atoi(argv[7]) : 2;
  const float conf = argc > 8 ? (float)atof(argv[8]) : 0.5f;
  lmx_yolo_info_t yi;
  lmx_sam_info_t si;
  if (lmx_yolo_image_check_host(argv[1], &yi) != LMX_OK) return fail("lmx_yolo_image_check_host");
  if (lmx_sam_image_check_host(argv[2], &si) != LMX_OK) return fail("lmx_sam_image_check_host");
  const int precision = (yi.plans & si.plans & (1 << LMX_SAM_EXACT)) ? LMX_SAM_EXACT : LMX_SAM_F16;

  FILE* f = fopen(argv[4], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) {
    fprintf(stderr, "fused_extract: %s: no int32 n, h, w header\n", argv[4]);
    return 1;
  }
  const int n = hdr[0], h = hdr[1], w = hdr[2];
  const size_t bytes = (size_t)n * h * w * 3;
  uint8_t* frames = (uint8_t*)malloc(bytes);
  if (!frames || fread(frames, 1, bytes, f) != bytes) {
    fprintf(stderr, "fused_extract: %s: fewer than %d frames of %d x %d\n", argv[4], n, h, w);
    return 1;
  }
  fclose(f);

  lmx_fused* fx = NULL;
  if (lmx_fused_open_host(argv[1], argv[2], argv[3], n, sam_chunk, sam_lanes, 2 + sam_lanes, &fx) != LMX_OK) return fail("lmx_fused_open_host");
  lmx_record_layout_t lay;
  if (lmx_fused_layout(fx, h, w, 0, &lay) != LMX_OK) {
    lmx_fused_close(fx);
    return fail("lmx_fused_layout");
  }
  uint8_t* records = (uint8_t*)malloc((size_t)n * (size_t)lay.stride);
  if (!records) {
    fprintf(stderr, "fused_extract: no memory for %d records of %lld bytes\n", n, (long long)lay.stride);
    return 1;
  }
  if (lmx_fused_step_host(fx, frames, n, h, w, precision, conf, records, n) != LMX_OK) {
    lmx_fused_close(fx);
    return fail("lmx_fused_step_host");
  }
  lmx_fused_close(fx);

  int64_t counts_at = -1;
  for (int i = 0; i < lay.n_fields; ++i)
    if (strcmp(lay.fields[i].name, "counts") == 0) counts_at = lay.fields[i].offset;
  int total = 0;
  for (int i = 0; i < n && counts_at >= 0; ++i) {
    int32_t c;
    memcpy(&c, records + (size_t)i * (size_t)lay.stride + (size_t)counts_at, sizeof(c));
    total += c;
  }
  f = fopen(argv[5], "wb");
  if (!f || fwrite(records, 1, (size_t)n * (size_t)lay.stride, f) != (size_t)n * (size_t)lay.stride || fclose(f) != 0) {
    fprintf(stderr, "fused_extract: cannot write %s\n", argv[5]);
    return 1;
  }
  printf("fused_extract: %d frames of %d x %d -> %d records of %lld bytes, %d detections (%s plan, passes of %d frames on %d lanes)\n", n, h, w, n,
         (long long)lay.stride, total, precision == LMX_SAM_EXACT ? "exact" : "f16", sam_chunk, sam_lanes);
  free(frames);
  free(records);
  return 0;
}
