// xfm_image.h — the weight image of the gait transformer (written by lmx/native.py write_xfm_image, read by host_xfm_image.cpp) as
// the model handle (gait_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind XFM:
//   config  at 48      8 x i32 (input_dim, d_model, n_heads, n_layers, ff, head, max_len, 0) then 1 x f64 (p)
//   tensors            all f32; a linear layer [K -> N] is [Q][N / 16][64][4] in the kernel's B-operand order (xfm.h, gait.h), Q = ceil(K / 16):
//     in.w [F -> D], in.b [D], pe [max_len][D]
//     layer.{l}.ln1.g / ln1.b [D]; qkv.w [H * D / 16][3 dh / 16][64][4]: per head one linear layer [D -> 3 dh] with the rows q_i | k_i | v_i
//     of in_proj_weight; qkv.b [H][3 dh]; out.w [D -> D], out.b [D]; ln2.g / ln2.b [D]; ff1.w [D -> FF], ff1.b [FF]; ff2.w [FF -> D], ff2.b [D]
//     lnf.g / lnf.b [D]; head.fc1.w [head][D], head.fc1.b [head], head.fc2.w [head], head.fc2.b [1]
#pragma once
#include <stdint.h>

#include "xfm.h"
#include "weights_table.h"

enum { LMX_XFM_CONFIG_BYTES = 8 * 4 + 8 };

typedef LmxTableImage<lmx_xfm_weights_t> LmxXfmImage;  // cfg, p, data_offset, file_bytes, rows, refs

// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with
// the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_xfm_image_parse(const char* path, LmxXfmImage* img);
// the weights with every pointer into `data`, a copy of the image's data section [data_offset, file_bytes) in host or device memory
inline void lmx_xfm_bind(const LmxXfmImage& img, const char* data, lmx_xfm_weights_t* w) { lmx_table_bind(img, data, w); }
void lmx_xfm_fill_info(const LmxXfmImage& img, int max_clips, int max_samples, lmx_xfm_info_t* info);
