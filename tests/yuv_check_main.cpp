// yuv_check_main.cpp — lmx_h_yuv420_to_bgr (csrc/host_yuv.cpp) as a stand-alone program, so that it can be built with
// -fsanitize=address,undefined and run over odd pitches and plane offsets (tests/test_yuv_host.py).
//   yuv_check_main IN OUT
// IN:  int64 n, h, w, layout, matrix, offset, pitch_y, pitch_c, stride_y, stride_c, then the bytes of the y allocation, of the u (or
//      interleaved) allocation and, for I420, of the v allocation, each WITHOUT the offset: a plane sits `offset` bytes into a heap block
//      of exactly offset + its bytes, so a read past the last row's last byte is a heap overflow the sanitizer reports.
// OUT: the BGR bytes [n][h][w][3].  Exit status: the function's return code (0), 2 for a usage or file error.
// The function reports through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
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

// bytes an allocation of n frames holds: up to the last byte of the last row of the last frame
static int64_t plane_bytes(int64_t n, int64_t rows, int64_t row, int64_t pitch, int64_t stride) { return (n - 1) * stride + (rows - 1) * pitch + row; }

static uint8_t* read_plane(FILE* f, int64_t offset, int64_t bytes) {
  uint8_t* p = (uint8_t*)malloc((size_t)(offset + bytes));
  if (!p || fread(p + offset, 1, (size_t)bytes, f) != (size_t)bytes) return NULL;
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  int64_t hd[10];
  if (!in || fread(hd, sizeof(int64_t), 10, in) != 10) return 2;
  const int64_t n = hd[0], h = hd[1], w = hd[2], layout = hd[3], matrix = hd[4], offset = hd[5];
  if (n < 1 || h < 2 || w < 2 || n * h * w > (1 << 26)) return 2;
  const int64_t row_c = layout == LMX_YUV_NV12 ? w : w / 2;
  uint8_t* y = read_plane(in, offset, plane_bytes(n, h, w, hd[6], hd[8]));
  uint8_t* u = read_plane(in, offset, plane_bytes(n, h / 2, row_c, hd[7], hd[9]));
  uint8_t* v = layout == LMX_YUV_I420 ? read_plane(in, offset, plane_bytes(n, h / 2, row_c, hd[7], hd[9])) : NULL;
  fclose(in);
  if (!y || !u || (layout == LMX_YUV_I420 && !v)) return 2;
  lmx_yuv_frames_t f;
  memset(&f, 0, sizeof(f));
  f.y = y + offset;
  f.u = u + offset;
  f.v = v ? v + offset : NULL;
  f.pitch_y = hd[6];
  f.pitch_c = hd[7];
  f.stride_y = hd[8];
  f.stride_c = hd[9];
  f.layout = (int32_t)layout;
  f.matrix = (int32_t)matrix;
  const size_t out_bytes = (size_t)(n * h * w * 3);
  uint8_t* bgr = (uint8_t*)malloc(out_bytes);
  const int rc = lmx_h_yuv420_to_bgr(&f, (int)n, (int)h, (int)w, bgr);
  if (rc != 0) {
    fprintf(stderr, "%s\n", g_error);
    return 1;
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || fwrite(bgr, 1, out_bytes, out) != out_bytes || fclose(out) != 0) return 2;
  free(bgr);
  free(y);
  free(u);
  free(v);
  return 0;
}
