// yuv_egress_check_main.cpp — lmx_h_bgr_to_yuv420 and lmx_h_yuv420_to_bgr_roi (csrc/host_yuv.cpp) as a stand-alone program, so that
// they can be built with -fsanitize=address,undefined and run over odd pitches and offsets (tests/test_yuv_egress_host.py).
//   yuv_egress_check_main IN OUT
// IN:  int64 mode, n, h, w, layout, matrix, offset, pitch_bgr, stride_bgr, pitch_y, pitch_c, stride_y, stride_c, roi x, y, w, h, then
//      mode 0 (BGR -> YUV): the bytes of the BGR allocation;  mode 1 (the window): the bytes of the y allocation, of the u (or
//      interleaved) allocation and, for I420, of the v allocation.  Every allocation comes WITHOUT the offset: a buffer, read or
//      written, sits `offset` bytes into a heap block of exactly offset + its bytes (up to the last byte of the last row of the last
//      frame), so an access past it is a heap overflow the sanitizer reports.
// OUT: mode 0: the bytes of the y, u (and v) allocations, pre-filled with 0x5A;  mode 1: the BGR bytes [n][roi h][roi w][3].
// Exit status: the function's return code (0), 2 for a usage or file error.
// The functions report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/lmx.h"

static char g_error[512];

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

static int64_t plane_bytes(int64_t n, int64_t rows, int64_t row, int64_t pitch, int64_t stride) { return (n - 1) * stride + (rows - 1) * pitch + row; }

static uint8_t* read_plane(FILE* f, int64_t offset, int64_t bytes) {
  uint8_t* p = (uint8_t*)malloc((size_t)(offset + bytes));
  if (!p || fread(p + offset, 1, (size_t)bytes, f) != (size_t)bytes) return NULL;
  return p;
}

static uint8_t* blank_plane(int64_t offset, int64_t bytes) {
  uint8_t* p = (uint8_t*)malloc((size_t)(offset + bytes));
  if (p) memset(p, 0x5A, (size_t)(offset + bytes));
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  int64_t hd[17];
  if (!in || fread(hd, sizeof(int64_t), 17, in) != 17) return 2;
  const int64_t mode = hd[0], n = hd[1], h = hd[2], w = hd[3], layout = hd[4], matrix = hd[5], offset = hd[6];
  if (n < 1 || h < 2 || w < 2 || n * h * w > (1 << 26) || offset < 0 || offset > 64) return 2;
  const int64_t row_c = layout == LMX_YUV_NV12 ? w : w / 2;
  const int64_t by = plane_bytes(n, h, w, hd[9], hd[11]), bc = plane_bytes(n, h / 2, row_c, hd[10], hd[12]);
  const bool planar = layout == LMX_YUV_I420;
  FILE* out = NULL;
  int rc;
  if (mode == 0) {
    uint8_t* bgr = read_plane(in, offset, plane_bytes(n, h, 3 * w, hd[7], hd[8]));
    fclose(in);
    uint8_t *y = blank_plane(offset, by), *u = blank_plane(offset, bc), *v = planar ? blank_plane(offset, bc) : NULL;
    if (!bgr || !y || !u || (planar && !v)) return 2;
    lmx_yuv_out_t o;
    memset(&o, 0, sizeof(o));
    o.y = y + offset;
    o.u = u + offset;
    o.v = v ? v + offset : NULL;
    o.pitch_y = hd[9];
    o.pitch_c = hd[10];
    o.stride_y = hd[11];
    o.stride_c = hd[12];
    o.layout = (int32_t)layout;
    o.matrix = (int32_t)matrix;
    rc = lmx_h_bgr_to_yuv420(bgr + offset, hd[7], hd[8], (int)n, (int)h, (int)w, &o);
    if (rc == 0) {
      out = fopen(argv[2], "wb");
      if (!out || fwrite(y + offset, 1, (size_t)by, out) != (size_t)by || fwrite(u + offset, 1, (size_t)bc, out) != (size_t)bc ||
          (v && fwrite(v + offset, 1, (size_t)bc, out) != (size_t)bc) || fclose(out) != 0)
        return 2;
    }
    free(bgr);
    free(y);
    free(u);
    free(v);
  } else {
    uint8_t* y = read_plane(in, offset, by);
    uint8_t* u = read_plane(in, offset, bc);
    uint8_t* v = planar ? read_plane(in, offset, bc) : NULL;
    fclose(in);
    if (!y || !u || (planar && !v)) return 2;
    lmx_yuv_frames_t f;
    memset(&f, 0, sizeof(f));
    f.y = y + offset;
    f.u = u + offset;
    f.v = v ? v + offset : NULL;
    f.pitch_y = hd[9];
    f.pitch_c = hd[10];
    f.stride_y = hd[11];
    f.stride_c = hd[12];
    f.layout = (int32_t)layout;
    f.matrix = (int32_t)matrix;
    lmx_rect_t roi = {(int32_t)hd[13], (int32_t)hd[14], (int32_t)hd[15], (int32_t)hd[16]};
    if (roi.w < 1 || roi.h < 1 || roi.w > w || roi.h > h) return 2;
    const size_t out_bytes = (size_t)(n * roi.h * roi.w * 3);
    uint8_t* bgr = (uint8_t*)malloc(offset + out_bytes);
    if (!bgr) return 2;
    rc = lmx_h_yuv420_to_bgr_roi(&f, (int)n, (int)h, (int)w, &roi, bgr + offset);
    if (rc == 0) {
      out = fopen(argv[2], "wb");
      if (!out || fwrite(bgr + offset, 1, out_bytes, out) != out_bytes || fclose(out) != 0) return 2;
    }
    free(bgr);
    free(y);
    free(u);
    free(v);
  }
  if (rc != 0) {
    fprintf(stderr, "%s\n", g_error);
    return 1;
  }
  return 0;
}
