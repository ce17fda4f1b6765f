// check_main.h — what the four *_check_main.cpp programs share: the program's own lmx_set_error (the library's lives in api.hip), the
// loader of an image's data section, the loader of a file of tensors into exactly-sized blocks and their binding by a weight table's rows, main's `check PATH...` mode, and for
// the two gait programs the reader of the pose file's common front and main's `score` mode.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static char g_error[512];  // the size of the library's buffer: a long message is cut at the same place

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, g_error);
  return 1;
}

// the data section [data_offset, file_bytes) of `image`, 64-byte aligned as a device allocation is; null if it cannot be read
static char* load_data(const char* image, uint64_t data_offset, uint64_t file_bytes) {
  const size_t bytes = (size_t)(file_bytes - data_offset), room = (bytes + 63) / 64 * 64;
  char* data = static_cast<char*>(aligned_alloc(64, room));
  FILE* f = fopen(image, "rb");
  if (!data || !f || fseek(f, (long)data_offset, SEEK_SET) || fread(data, 1, bytes, f) != bytes) return nullptr;
  fclose(f);
  return data;
}

// the f32 tensors of `path` with counts[i] floats each, one after the other: each into a block of its own, 16-byte aligned and exactly as
// long as the tensor; whole_file: the file holds the tensors and nothing more
static bool load_tensors(const char* path, const std::vector<size_t>& counts, bool whole_file, std::vector<char*>& blocks) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (size_t c : counts) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, c * 4) || fread(p, 4, c, f) != c) return false;
    blocks.push_back(static_cast<char*>(p));
  }
  if (whole_file && fgetc(f) != EOF) return false;
  fclose(f);
  return true;
}

// blocks[i] becomes the tensor of rows[i]: its address goes into the `const float*` of the weights struct `w` at rows[i].at (Row: LmxTensorRow)
template <class Weights, class Row>
static void bind_blocks(const std::vector<Row>& rows, const std::vector<char*>& blocks, Weights* w) {
  for (size_t i = 0; i < rows.size(); ++i)
    *reinterpret_cast<const float**>(reinterpret_cast<char*>(w) + rows[i].at) = reinterpret_cast<const float*>(blocks[i]);
}

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

// the front of a pose file: T0 x 40 f64 keypoints, T0 x 4 f64 boxes, T0 x i32 keypoint counts.  The file stays open for what follows
static FILE* open_pose(const char* pose, int T0, std::vector<double>& kp, std::vector<double>& bbox, std::vector<int>& n_kp) {
  kp.resize((size_t)T0 * 40), bbox.resize((size_t)T0 * 4), n_kp.resize((size_t)T0);
  FILE* f = fopen(pose, "rb");
  return f && read_all(f, kp) && read_all(f, bbox) && read_all(f, n_kp) ? f : nullptr;
}

// check PATH...: one line per file, "<return code>\t<path>\t<error text>"; false if the arguments ask for something else
template <class Info>
static bool check_mode(int argc, char** argv, int (*check)(const char*, Info*)) {
  if (argc < 3 || strcmp(argv[1], "check") != 0) return false;
  for (int i = 2; i < argc; ++i) {
    g_error[0] = 0;
    Info info;
    const int rc = check(argv[i], &info);
    printf("%d\t%s\t%s\n", rc, argv[i], g_error);
  }
  return true;
}

// check PATH... | score IMAGE POSE T0 S SEED
template <class Info>
static int gait_main(int argc, char** argv, int (*check)(const char*, Info*), int (*score)(const char*, const char*, int, int, uint64_t)) {
  if (check_mode(argc, argv, check)) return 0;
  if (argc == 7 && strcmp(argv[1], "score") == 0) return score(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), strtoull(argv[6], nullptr, 10));
  fprintf(stderr, "usage: %s check PATH... | score IMAGE POSE T0 S SEED\n", argv[0]);
  return 2;
}
