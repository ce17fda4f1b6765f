// sam_image_check_main.cpp — the SAM weight-image reader (csrc/host_image.cpp + host_sam_image.cpp) as a stand-alone program, so that it
// can be built with -fsanitize=address,undefined and fed corrupted files (tests/test_sam_image_reader_sanitized.py).
//   sam_image_check_main check PATH...          one line per file: "<return code>\t<path>\t<error text>"
//   sam_image_check_main resized IMAGE H W ...  one line per (H, W) pair: "<nh>\t<nw>", the arithmetic behind lmx_sam_resized
// The reader reports through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vision-sam3-yolo-lameless_amd/csrc/sam_image.h"

static char g_error[512];  // the size of the library's buffer: a long message is cut at the same place

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "check") == 0) {
    for (int i = 2; i < argc; ++i) {
      g_error[0] = 0;
      lmx_sam_info_t info;
      const int rc = lmx_sam_image_check_host(argv[i], &info);
      printf("%d\t%s\t%s\n", rc, argv[i], g_error);
    }
    return 0;
  }
  if (argc >= 3 && strcmp(argv[1], "resized") == 0 && argc % 2 == 1) {
    for (int i = 3; i + 1 < argc; i += 2) {
      int nh = 0, nw = 0;
      lmx_sam_resized_hw(atoi(argv[2]), atoi(argv[i]), atoi(argv[i + 1]), &nh, &nw);
      printf("%d\t%d\n", nh, nw);
    }
    return 0;
  }
  fprintf(stderr, "usage: %s check PATH... | resized IMAGE H W [H W ...]\n", argv[0]);
  return 2;
}
