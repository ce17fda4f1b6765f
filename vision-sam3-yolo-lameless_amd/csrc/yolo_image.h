// yolo_image.h — the weight image of a YOLOv8 detector (written by lmx/native.py write_yolo_image, read by host_yolo_image.cpp) as the
// model handle (yolo_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind YOLO:
//   config  at 48      10 x i32 (LmxYoloCfg's integers in declaration order), then the names blob: n_names NUL-terminated UTF-8 strings
//                      in class order, names_bytes long, zero-padded to a multiple of 8
//   tensors            stem.w f32 [3][3][3][C0] (ky, kx, c, co), stem.b f32 [C0];
//                      per convolution `name` of the layer table (model.1, model.2.cv1, model.2.m.0.cv1, ..., model.22.cv3.2.2):
//                        plan f16:    f16.<name>.w f16 [Cout][k*k*Cin] packed (ky, kx, ci), f16.<name>.b f32 [Cout]
//                        plan exact:  x3.<name>.w f16 [Cout][3*k*k*Cin] (per channel group [whi | whi / 2048 | wlo]), x3.<name>.b f32 [Cout]
//                                     (the bias scaled by the row's power of two), x3.<name>.s f32 [Cout] (the row scale)
//                      each bit for bit what YoloDetector holds on the device (Detect's class rows padded to nc_pad, the Pose branch to
//                      multiples of 8 channels and nk_pad rows)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "image.h"

enum { LMX_YOLO_CONFIG_INTS = 10 };

struct LmxYoloCfg {
  int32_t scale;  // 'n' 's' 'm' 'l' 'x'
  int32_t nc, nc_pad, imgsz;
  int32_t kpt_k, kpt_ndim;  // 0, 0: no Pose head
  int32_t nk_pad;
  int32_t plans;  // bit (1 << LMX_YOLO_F16) | bit (1 << LMX_YOLO_EXACT)
  int32_t n_names, names_bytes;
};

// one module of yolov8.yaml with resolved channels (lmx/yolo.py layer_table)
enum { LMX_YM_CONV = 0, LMX_YM_C2F, LMX_YM_SPPF, LMX_YM_UP, LMX_YM_CAT, LMX_YM_DETECT };
struct LmxYoloModule {
  int kind = 0, c1 = 0, c2 = 0, n = 0, shortcut = 0;
};

// one convolution behind the stem: its name and its dimensions as the f16 plan stores them (the exact plan's K is 3 x that)
struct LmxYoloConv {
  std::string name;
  int k = 1, cout = 0, cin = 0;
  LmxTensorRef w, b;        // plan f16
  LmxTensorRef xw, xb, xs;  // plan exact
};

struct LmxYoloImage {
  LmxYoloCfg cfg;
  std::vector<std::string> names;
  uint64_t data_offset = 0, file_bytes = 0;
  std::vector<LmxYoloModule> table;  // 23 modules
  int c2 = 0, c3 = 0, c4p = 0;       // Detect's branch widths (c4p: the Pose branch, padded to 8; 0 without one)
  LmxTensorRef stem_w, stem_b;
  std::vector<LmxYoloConv> convs;  // in the order of YoloDetector.w
};

// the 23 modules and Detect's widths for (scale, nc, keypoint shape); LMX_EINVAL for a configuration the kernels do not serve
int lmx_yolo_layer_table(const LmxYoloCfg& c, std::vector<LmxYoloModule>* table, int* c2, int* c3, int* c4p);
// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with the
// offending field or tensor named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_yolo_image_parse(const char* path, LmxYoloImage* img);
const LmxYoloConv* lmx_yolo_find_conv(const LmxYoloImage& img, const std::string& name);
void lmx_yolo_fill_info(const LmxYoloCfg& c, int max_batch, lmx_yolo_info_t* info);
