// dino_image.h — the weight image of a DINO embedder (written by lmx/native.py write_dino_image, read by host_dino_image.cpp) as the
// model handle (dino_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind DINO:
//   config  at 48      20 x i32 (LmxDinoCfg's integers in declaration order) then 8 x f64 (eps, rescale, mean[3], std[3])
//   tensors            each bit for bit what DinoEmbedder holds on the device
#pragma once
#include <stdint.h>

#include <vector>

#include "image.h"

enum { LMX_DINO_CONFIG_BYTES = 20 * 4 + 8 * 8 };

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
