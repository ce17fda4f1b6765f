// dino_image.h — the weight image of a DINO embedder (written by lmx/native.py write_dino_image, read by host_dino_image.cpp) as the
// model handle (dino_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// File layout, little-endian, every offset from the start of the file:
//   header  48 bytes   magic "LMXIMAGE" | u32 version | u32 kind | u32 config_bytes | u32 n_tensors | u64 dir_offset |
//                      u64 data_offset | u64 file_bytes
//   config  at 48      kind DINO: 20 x i32 (LmxDinoCfg's integers in declaration order) then 8 x f64 (eps, rescale, mean[3], std[3])
//   directory          n_tensors entries of 88 bytes: char name[48] (NUL padded) | u32 dtype | u32 rank | i32 shape[4] |
//                      u64 offset (a multiple of 64, >= data_offset) | u64 nbytes (= elements * element size)
//   data               the tensors, each bit for bit what DinoEmbedder holds on the device
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/lmx.h"

#define LMX_IMAGE_VERSION 1u
enum { LMX_IMAGE_DINO = 1, LMX_IMAGE_YOLO = 2, LMX_IMAGE_SAM = 3 };  // kinds; DINO here, YOLO in yolo_image.h; SAM has no reader yet
enum { LMX_IMG_F16 = 0, LMX_IMG_F32 = 1, LMX_IMG_I32 = 2 };          // directory dtypes (F16 / F32 as LMX_F16 / LMX_F32)
enum { LMX_IMAGE_HEADER_BYTES = 48, LMX_IMAGE_ENTRY_BYTES = 88, LMX_IMAGE_NAME_BYTES = 48, LMX_DINO_CONFIG_BYTES = 20 * 4 + 8 * 8 };

struct LmxDinoCfg {
  int32_t arch;  // LMX_DINO_V2 / LMX_DINO_V3
  int32_t hidden, heads, layers, mlp, gated, patch, image, grid, n_prefix, tokens, k_pad;
  int32_t has_pos, has_rope;
  int32_t recipe_kind;    // LMX_RECIPE_PIL / LMX_RECIPE_FLOAT
  int32_t filt;           // LMX_FILT_BILINEAR / LMX_FILT_BICUBIC
  int32_t shortest_edge;  // 0: the recipe resizes to size_h x size_w
  int32_t size_h, size_w;
  int32_t crop;           // 0: no centre crop
  double eps, rescale, mean[3], std[3];
};

struct LmxTensorRef {
  uint64_t offset = 0, nbytes = 0;  // nbytes 0: absent
};

struct LmxDinoLayerRefs {
  LmxTensorRef g1, b1, wqkv, bqkv, wo, bo, ls1, g2, b2, w1, bb1, w2, bb2, ls2;
};

struct LmxDinoImage {
  LmxDinoCfg cfg;
  uint64_t data_offset = 0, file_bytes = 0;
  LmxTensorRef pe_w, pe_b, prefix, pos, rope_cos, rope_sin, gf, bf, lut;
  std::vector<LmxDinoLayerRefs> layers;
};

// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with
// the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_dino_image_parse(const char* path, LmxDinoImage* img);
// (nh, nw) the recipe resizes an h x w frame to; LMX_EINVAL if that is smaller than the network's input
int lmx_dino_resized(const LmxDinoCfg& c, int h, int w, int* nh, int* nw);
void lmx_dino_fill_info(const LmxDinoCfg& c, int max_batch, lmx_dino_info_t* info);
