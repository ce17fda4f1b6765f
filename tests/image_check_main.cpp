// image_check_main.cpp — the weight-image readers (csrc/host_image.cpp, host_dino_image.cpp, host_yolo_image.cpp) as a stand-alone
// program, so that they can be built with -fsanitize=address,undefined and fed corrupted files (tests/test_image_reader_sanitized.py).
//   image_check_main d|y PATH...     one line per file: "<return code>\t<path>\t<error text>"
// The readers report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../include/lmx.h"

static char g_error[512];  // the size of the library's buffer: a long message is cut at the same place

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int main(int argc, char** argv) {
  if (argc < 2 || (strcmp(argv[1], "d") != 0 && strcmp(argv[1], "y") != 0)) {
    fprintf(stderr, "usage: %s d|y PATH...\n", argv[0]);
    return 2;
  }
  for (int i = 2; i < argc; ++i) {
    g_error[0] = 0;
    int rc;
    if (argv[1][0] == 'd') {
      lmx_dino_info_t info;
      rc = lmx_dino_image_check_host(argv[i], &info);
    } else {
      lmx_yolo_info_t info;
      rc = lmx_yolo_image_check_host(argv[i], &info);
    }
    printf("%d\t%s\t%s\n", rc, argv[i], g_error);
  }
  return 0;
}
