/* fused_extract_nv12.c — fused_extract.c's flow from frames as a decoder leaves them: rawvideo NV12 (or yuv420p) in, one fixed-stride
 * record per frame out.  The colour conversion runs on the device (lmx_fused_step_yuv_host), so the caller uploads 1.5 bytes per pixel
 * and never makes a BGR frame.  No Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/fused_extract_nv12.c -o fused_extract_nv12 -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./fused_extract_nv12 yolo.lmx sam.lmx dino.lmx frames.yuv W H records.bin [nv12|yuv420p [bt601|bt709 [sam_chunk [sam_lanes [conf]]]]]
 *
 * yolo.lmx, sam.lmx, dino.lmx   weight images, exported once from Python: lmx.native.write_yolo_image / write_sam_image / write_dino_image
 * frames.yuv    tightly packed rawvideo, W x H even, W * H * 3 / 2 bytes a frame — what `ffmpeg -i clip.mp4 -f rawvideo -pix_fmt nv12`
 *               writes: H luma rows, then H / 2 rows of interleaved U V (nv12) or the U plane and the V plane (yuv420p)
 * records.bin   receives the record matrix uint8 [n][stride] (lmx_fused_layout; lmx.dist.unpack_records reads it): per frame what
 *               services/yolo-pipeline/app/main.py:74-76, services/sam3-pipeline/app/main.py:74-92 and :118-135 and
 *               services/dinov3-pipeline/app/main.py:98-113 yield on the frame cv2.VideoCapture would have delivered.
 * Limited range only (bt601: cv2's constants; bt709: what HD streams are usually tagged with); the arithmetic is the text at
 * lmx_k_yuv420_to_bgr in lmx.h, and its parity with OpenCV and swscale is unpinned.  The file is read in steps of at most 64 frames.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time.) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "fused_extract_nv12: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s yolo.lmx sam.lmx dino.lmx frames.yuv W H records.bin [nv12|yuv420p [bt601|bt709 [sam_chunk [sam_lanes [conf]]]]]\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[5]), h = atoi(argv[6]);
  const int layout = argc > 8 && strcmp(argv[8], "yuv420p") == 0 ? LMX_YUV_I420 : LMX_YUV_NV12;
  const int matrix = argc > 9 && strcmp(argv[9], "bt709") == 0 ? LMX_YUV_BT709 : LMX_YUV_BT601;
  const int sam_chunk = argc > 10 ? atoi(argv[10]) : 16, sam_lanes = argc > 11 ? atoi(argv[11]) : 2;
  const float conf = argc > 12 ? (float)atof(argv[12]) : 0.5f;
  if (w < 2 || h < 2 || w % 2 || h % 2) {
    fprintf(stderr, "fused_extract_nv12: 4:2:0 frames have even sizes, not %d x %d\n", w, h);
    return 2;
  }
  lmx_yolo_info_t yi;
  lmx_sam_info_t si;
  if (lmx_yolo_image_check_host(argv[1], &yi) != LMX_OK) return fail("lmx_yolo_image_check_host");
  if (lmx_sam_image_check_host(argv[2], &si) != LMX_OK) return fail("lmx_sam_image_check_host");
  const int precision = (yi.plans & si.plans & (1 << LMX_SAM_EXACT)) ? LMX_SAM_EXACT : LMX_SAM_F16;

  const int max_frames = 64;
  const size_t frame_bytes = (size_t)w * h * 3 / 2;
  lmx_fused* fx = NULL;
  if (lmx_fused_open_host(argv[1], argv[2], argv[3], max_frames, sam_chunk, sam_lanes, 2 + sam_lanes, &fx) != LMX_OK) return fail("lmx_fused_open_host");
  lmx_record_layout_t lay;
  if (lmx_fused_layout(fx, h, w, 0, &lay) != LMX_OK) {
    lmx_fused_close(fx);
    return fail("lmx_fused_layout");
  }
  uint8_t* yuv = (uint8_t*)malloc((size_t)max_frames * frame_bytes);
  uint8_t* records = (uint8_t*)malloc((size_t)max_frames * (size_t)lay.stride);
  FILE* in = fopen(argv[4], "rb");
  FILE* out = fopen(argv[7], "wb");
  if (!yuv || !records || !in || !out) {
    fprintf(stderr, "fused_extract_nv12: cannot open %s / %s, or no memory for %d frames\n", argv[4], argv[7], max_frames);
    lmx_fused_close(fx);
    return 1;
  }
  int64_t counts_at = -1;
  for (int i = 0; i < lay.n_fields; ++i)
    if (strcmp(lay.fields[i].name, "counts") == 0) counts_at = lay.fields[i].offset;
  long frames = 0, total = 0;
  for (;;) {
    const int n = (int)(fread(yuv, 1, (size_t)max_frames * frame_bytes, in) / frame_bytes); /* whole frames; a cut last frame is dropped */
    if (n == 0) break;
    if (lmx_fused_step_yuv_host(fx, yuv, layout, matrix, n, h, w, precision, conf, records, n) != LMX_OK) {
      lmx_fused_close(fx);
      return fail("lmx_fused_step_yuv_host");
    }
    for (int i = 0; i < n && counts_at >= 0; ++i) {
      int32_t c;
      memcpy(&c, records + (size_t)i * (size_t)lay.stride + (size_t)counts_at, sizeof(c));
      total += c;
    }
    if (fwrite(records, 1, (size_t)n * (size_t)lay.stride, out) != (size_t)n * (size_t)lay.stride) {
      fprintf(stderr, "fused_extract_nv12: cannot write %s\n", argv[7]);
      lmx_fused_close(fx);
      return 1;
    }
    frames += n;
  }
  lmx_fused_close(fx);
  fclose(in);
  if (fclose(out) != 0) {
    fprintf(stderr, "fused_extract_nv12: cannot write %s\n", argv[7]);
    return 1;
  }
  printf("fused_extract_nv12: %ld %s frames of %d x %d (%s) -> %ld records of %lld bytes, %ld detections (%s plan, passes of %d frames on %d lanes)\n", frames,
         layout == LMX_YUV_NV12 ? "nv12" : "yuv420p", w, h, matrix == LMX_YUV_BT709 ? "bt709" : "bt601", frames, (long long)lay.stride, total,
         precision == LMX_SAM_EXACT ? "exact" : "f16", sam_chunk, sam_lanes);
  free(yuv);
  free(records);
  return 0;
}
