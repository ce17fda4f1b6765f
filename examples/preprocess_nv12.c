/* preprocess_nv12.c — services/video-preprocessing/app/main.py:39-149 on the original decode, from C: rawvideo NV12 in; the crop box
 * from YOLO on the first 10 frames (lmx_yolo_detect at the model's default confidence, then conf > 0.5, then lmx_h_crop_box: boxes above
 * 10 % of the frame, the median, 50 px of padding); one record per frame from the three pipelines on that WINDOW of the frames
 * (lmx_fused_step_yuv_roi: no re-encode, no second decode); and the cropped clip as rawvideo NV12, what an encoder takes
 * (lmx_k_yuv420_to_bgr_roi, then lmx_k_bgr_to_yuv420).  The frames live on the device, so this example calls the HIP runtime itself.
 *
 *   cc -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/preprocess_nv12.c -o preprocess_nv12 \
 *      -Lvision-sam3-yolo-lameless_amd/lmx -llmx -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx
 *   ./preprocess_nv12 yolo.lmx sam.lmx dino.lmx frames.yuv W H records.bin cropped.yuv [bt601|bt709 [sam_chunk [sam_lanes]]]
 *
 * yolo.lmx, sam.lmx, dino.lmx   weight images, exported once from Python: lmx.native.write_yolo_image / write_sam_image / write_dino_image
 * frames.yuv    tightly packed rawvideo nv12, W x H even, at most 64 frames are read (one step; a longer clip repeats the step)
 * records.bin   the record matrix uint8 [n][stride] of lmx_fused_layout at the WINDOW's size
 * cropped.yuv   rawvideo nv12 of the encoder's box: x2 / y2 one lower where a side of the crop box is odd (libx264 refuses odd
 *               yuv420p sizes, so for such a clip the reference publishes nothing: a documented departure)
 * Prints the crop box and the `video.preprocessed` sizes.  The colour arithmetic is the text in lmx.h; parity with OpenCV and swscale is
 * unpinned. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lmx.h"

#define MAX_FRAMES 64
#define MAX_DET 300

static int fail(const char* what) {
  fprintf(stderr, "preprocess_nv12: %s: %s\n", what, lmx_last_error());
  return 1;
}

static int hip_fail(const char* what, hipError_t e) {
  fprintf(stderr, "preprocess_nv12: %s: %s\n", what, hipGetErrorString(e));
  return 1;
}

#define HIP(call)                                  \
  do {                                             \
    const hipError_t e_ = (call);                  \
    if (e_ != hipSuccess) return hip_fail(#call, e_); \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: %s yolo.lmx sam.lmx dino.lmx frames.yuv W H records.bin cropped.yuv [bt601|bt709 [sam_chunk [sam_lanes]]]\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[5]), h = atoi(argv[6]);
  const int matrix = argc > 9 && strcmp(argv[9], "bt709") == 0 ? LMX_YUV_BT709 : LMX_YUV_BT601;
  const int sam_chunk = argc > 10 ? atoi(argv[10]) : 16, sam_lanes = argc > 11 ? atoi(argv[11]) : 2;
  if (w < 2 || h < 2 || w % 2 || h % 2) {
    fprintf(stderr, "preprocess_nv12: 4:2:0 frames have even sizes, not %d x %d\n", w, h);
    return 2;
  }
  const size_t luma = (size_t)w * h, frame_bytes = luma * 3 / 2;
  uint8_t* host = (uint8_t*)malloc((size_t)MAX_FRAMES * frame_bytes);
  FILE* in = fopen(argv[4], "rb");
  if (!host || !in) {
    fprintf(stderr, "preprocess_nv12: cannot open %s, or no memory\n", argv[4]);
    return 1;
  }
  const int n = (int)(fread(host, 1, (size_t)MAX_FRAMES * frame_bytes, in) / frame_bytes);
  fclose(in);
  if (n == 0) {
    fprintf(stderr, "preprocess_nv12: %s holds no whole frame of %d x %d\n", argv[4], w, h);
    return 1;
  }
  uint8_t* yuv = NULL;
  HIP(hipMalloc((void**)&yuv, (size_t)n * frame_bytes));
  HIP(hipMemcpy(yuv, host, (size_t)n * frame_bytes, hipMemcpyHostToDevice));
  lmx_yuv_frames_t f;
  memset(&f, 0, sizeof(f));
  f.y = yuv;
  f.u = yuv + luma;
  f.pitch_y = f.pitch_c = w;
  f.stride_y = f.stride_c = (int64_t)frame_bytes;
  f.layout = LMX_YUV_NV12;
  f.matrix = matrix;

  /* ---- the crop box: main.py:65-110 */
  lmx_yolo_info_t yi;
  lmx_sam_info_t si;
  if (lmx_yolo_image_check_host(argv[1], &yi) != LMX_OK) return fail("lmx_yolo_image_check_host");
  if (lmx_sam_image_check_host(argv[2], &si) != LMX_OK) return fail("lmx_sam_image_check_host");
  const int precision = (yi.plans & si.plans & (1 << LMX_SAM_EXACT)) ? LMX_SAM_EXACT : LMX_SAM_F16;
  const int sample = n < 10 ? n : 10;
  lmx_yolo* det = NULL;
  if (lmx_yolo_open_host(argv[1], sample, &det) != LMX_OK) return fail("lmx_yolo_open_host");
  uint8_t* bgr = NULL;
  float *d_boxes = NULL, *d_scores = NULL;
  int32_t *d_cls = NULL, *d_src = NULL, *d_counts = NULL;
  HIP(hipMalloc((void**)&bgr, (size_t)sample * luma * 3));
  HIP(hipMalloc((void**)&d_boxes, (size_t)sample * MAX_DET * 4 * sizeof(float)));
  HIP(hipMalloc((void**)&d_scores, (size_t)sample * MAX_DET * sizeof(float)));
  HIP(hipMalloc((void**)&d_cls, (size_t)sample * MAX_DET * sizeof(int32_t)));
  HIP(hipMalloc((void**)&d_src, (size_t)sample * MAX_DET * sizeof(int32_t)));
  HIP(hipMalloc((void**)&d_counts, (size_t)sample * sizeof(int32_t)));
  if (lmx_k_yuv420_to_bgr(&f, sample, h, w, bgr, NULL) != LMX_OK) return fail("lmx_k_yuv420_to_bgr");
  if (lmx_yolo_detect(det, bgr, sample, h, w, precision, 0.25f, 0.7, MAX_DET, d_boxes, d_scores, d_cls, d_src, d_counts, NULL, NULL) != LMX_OK)
    return fail("lmx_yolo_detect");
  HIP(hipDeviceSynchronize());
  float* boxes = (float*)malloc((size_t)sample * MAX_DET * 4 * sizeof(float));
  float* scores = (float*)malloc((size_t)sample * MAX_DET * sizeof(float));
  int32_t counts[10];
  if (!boxes || !scores) return 1;
  HIP(hipMemcpy(boxes, d_boxes, (size_t)sample * MAX_DET * 4 * sizeof(float), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(scores, d_scores, (size_t)sample * MAX_DET * sizeof(float), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(counts, d_counts, (size_t)sample * sizeof(int32_t), hipMemcpyDeviceToHost));
  int k = 0; /* boxes with conf > 0.5, every class, packed to the front in the reference's order */
  for (int i = 0; i < sample; ++i)
    for (int j = 0; j < counts[i]; ++j)
      if (scores[(size_t)i * MAX_DET + j] > 0.5f) memmove(boxes + 4 * (size_t)k++, boxes + 4 * ((size_t)i * MAX_DET + j), 4 * sizeof(float));
  int32_t box[4];
  if (lmx_h_crop_box(boxes, k, h, w, 50, box) != LMX_OK) return fail("lmx_h_crop_box");
  lmx_yolo_close(det);
  HIP(hipFree(bgr));
  HIP(hipFree(d_boxes));
  HIP(hipFree(d_scores));
  HIP(hipFree(d_cls));
  HIP(hipFree(d_src));
  HIP(hipFree(d_counts));
  free(boxes);
  free(scores);
  const lmx_rect_t roi = {box[0], box[1], box[2] - box[0], box[3] - box[1]};
  printf("preprocess_nv12: %d confident boxes on %d frames -> crop_box [%d, %d, %d, %d], width %d, height %d\n", k, sample, box[0], box[1], box[2], box[3],
         roi.w, roi.h);

  /* ---- the three pipelines on the window of the original frames */
  lmx_fused* fx = NULL;
  if (lmx_fused_open_host(argv[1], argv[2], argv[3], MAX_FRAMES, sam_chunk, sam_lanes, 2 + sam_lanes, &fx) != LMX_OK) return fail("lmx_fused_open_host");
  lmx_record_layout_t lay;
  if (lmx_fused_layout(fx, roi.h, roi.w, 0, &lay) != LMX_OK) return fail("lmx_fused_layout");
  const size_t rec_bytes = (size_t)n * (size_t)lay.stride;
  uint8_t* d_records = NULL;
  HIP(hipMalloc((void**)&d_records, rec_bytes));
  if (lmx_fused_step_yuv_roi(fx, &f, n, h, w, &roi, precision, 0.5f, d_records, n, NULL) != LMX_OK) return fail("lmx_fused_step_yuv_roi");
  HIP(hipDeviceSynchronize());
  uint8_t* records = (uint8_t*)malloc(rec_bytes);
  if (!records) return 1;
  HIP(hipMemcpy(records, d_records, rec_bytes, hipMemcpyDeviceToHost));
  lmx_fused_close(fx);
  FILE* out = fopen(argv[7], "wb");
  if (!out || fwrite(records, 1, rec_bytes, out) != rec_bytes || fclose(out) != 0) {
    fprintf(stderr, "preprocess_nv12: cannot write %s\n", argv[7]);
    return 1;
  }
  free(records);
  HIP(hipFree(d_records));

  /* ---- the cropped clip for an encoder: the window to BGR at the box's parity, then back to NV12 at even sizes */
  const lmx_rect_t enc = {roi.x, roi.y, roi.w - (roi.w & 1), roi.h - (roi.h & 1)};
  if (enc.w >= 2 && enc.h >= 2) {
    const size_t eluma = (size_t)enc.w * enc.h, eframe = eluma * 3 / 2;
    uint8_t *ebgr = NULL, *eyuv = NULL;
    HIP(hipMalloc((void**)&ebgr, (size_t)n * eluma * 3));
    HIP(hipMalloc((void**)&eyuv, (size_t)n * eframe));
    lmx_yuv_out_t o;
    memset(&o, 0, sizeof(o));
    o.y = eyuv;
    o.u = eyuv + eluma;
    o.pitch_y = o.pitch_c = enc.w;
    o.stride_y = o.stride_c = (int64_t)eframe;
    o.layout = LMX_YUV_NV12;
    o.matrix = matrix;
    if (lmx_k_yuv420_to_bgr_roi(&f, n, h, w, &enc, ebgr, NULL) != LMX_OK) return fail("lmx_k_yuv420_to_bgr_roi");
    if (lmx_k_bgr_to_yuv420(ebgr, 3 * (int64_t)enc.w, 3 * (int64_t)eluma, n, enc.h, enc.w, &o, NULL) != LMX_OK) return fail("lmx_k_bgr_to_yuv420");
    HIP(hipDeviceSynchronize());
    uint8_t* ehost = (uint8_t*)malloc((size_t)n * eframe);
    if (!ehost) return 1;
    HIP(hipMemcpy(ehost, eyuv, (size_t)n * eframe, hipMemcpyDeviceToHost));
    out = fopen(argv[8], "wb");
    if (!out || fwrite(ehost, 1, (size_t)n * eframe, out) != (size_t)n * eframe || fclose(out) != 0) {
      fprintf(stderr, "preprocess_nv12: cannot write %s\n", argv[8]);
      return 1;
    }
    free(ehost);
    HIP(hipFree(ebgr));
    HIP(hipFree(eyuv));
  }
  HIP(hipFree(yuv));
  free(host);
  printf("preprocess_nv12: %d nv12 frames of %d x %d -> %d records of %lld bytes at %d x %d, cropped clip %d x %d\n", n, w, h, n, (long long)lay.stride,
         roi.w, roi.h, enc.w, enc.h);
  return 0;
}
