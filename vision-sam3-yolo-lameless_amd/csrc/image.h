// image.h — the weight-image container every model-level handle reads (written by lmx/native.py write_image, read by host_image.cpp).
// Host code only: nothing here needs HIP.  The container knows no model: a model's reader (host_<model>_image.cpp for dino, yolo, sam,
// tcn, xfm, gfm and gnn) decodes and validates its own config block, then asks for each tensor the configuration calls for by name, dtype
// and shape (the last four through the model's weight table, weights_table.h).
//
// File layout, little-endian, every offset from the start of the file:
//   header  48 bytes   magic "LMXIMAGE" | u32 version | u32 kind | u32 config_bytes | u32 n_tensors | u64 dir_offset |
//                      u64 data_offset | u64 file_bytes
//   config  at 48      config_bytes of the kind's own block (<model>_image.h of the seven kinds)
//   directory          n_tensors entries of 88 bytes: char name[48] (NUL padded) | u32 dtype | u32 rank | i32 shape[4] |
//                      u64 offset (a multiple of 64, >= data_offset) | u64 nbytes (= elements * element size)
//   data               the tensors, each bit for bit what the Python model holds on the device
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/lmx.h"

#define LMX_IMAGE_VERSION 1u
enum { LMX_IMAGE_DINO = 1, LMX_IMAGE_YOLO = 2, LMX_IMAGE_SAM = 3, LMX_IMAGE_TCN = 4, LMX_IMAGE_XFM = 5, LMX_IMAGE_GFM = 6, LMX_IMAGE_GNN = 7 };  // kinds
enum { LMX_IMG_F16 = 0, LMX_IMG_F32 = 1, LMX_IMG_I32 = 2 };          // directory dtypes (F16 / F32 as LMX_F16 / LMX_F32)
enum { LMX_IMAGE_HEADER_BYTES = 48, LMX_IMAGE_ENTRY_BYTES = 88, LMX_IMAGE_NAME_BYTES = 48, LMX_IMAGE_MAX_CONFIG_BYTES = 1 << 20 };

void lmx_set_error(const char* fmt, ...);  // api.hip

#define IMG_REQUIRE(cond, ...)    \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

template <class T>
inline T rd(const unsigned char* p) {  // the image is little-endian, and so is every host this library is built for
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

struct LmxTensorRef {
  uint64_t offset = 0, nbytes = 0;  // nbytes 0: absent
};

struct LmxImageEntry {
  uint32_t dtype, rank;
  int32_t shape[4];
  uint64_t offset, nbytes;
};

// A parsed container: the validated header fields, the config block's bytes and the directory.  No number in it was taken from
// the file without a check against the file's real size; what the config block SAYS is the model's to validate.
struct LmxImageFile {
  const char* who = "";  // the prefix of every message: "dino image", "yolo image"
  uint64_t data_offset = 0, file_bytes = 0;
  std::vector<unsigned char> config;
  std::map<std::string, LmxImageEntry> dir;  // an entry the model's reader does not ask for is ignored
};

// Open `path` as an image of `kind` (`kind_name`: "DINO" / "YOLO" in the message) and read its header, config block and directory
// (the tensor data is not read).  The config block is at most LMX_IMAGE_MAX_CONFIG_BYTES; the size its kind needs is the model's
// to check.  LMX_EINVAL with the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_image_open(const char* who, const char* path, uint32_t kind, const char* kind_name, LmxImageFile* img);

// the shape a model's reader asks for; `field` names the config numbers it comes from (in the message of a mismatch)
struct LmxImageWant {
  const char* field;
  uint32_t dtype, rank;
  int32_t shape[4];
};

// the tensor `name` with exactly this dtype, rank and shape, 64-byte aligned inside [data_offset, file_bytes)
int lmx_image_take(const LmxImageFile& img, const std::string& name, const LmxImageWant& w, LmxTensorRef* ref);
// the same from inside a model's reader: the shape's dimensions follow the rank; returns the error from the calling function
#define IMG_TAKE(file, name, ref, field, dt, rank, ...)                    \
  do {                                                                     \
    const LmxImageWant w_ = {field, dt, rank, {__VA_ARGS__}};              \
    if (const int rc_ = lmx_image_take(file, name, w_, ref)) return rc_;   \
  } while (0)
