// tcn_image.h — the weight image of the TCN gait model (written by lmx/native.py write_tcn_image, read by host_tcn_image.cpp) as the
// model handle (gait_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind TCN:
//   config  at 48      12 x i32 (input_dim, n_blocks, k, head, channels[8]; channels beyond n_blocks are 0) then 1 x f64 (p)
//   tensors            all f32, the FOLDED weight-norm weights g * v / ||v|| as torch's parametrisation evaluates them, in the order the
//                      kernel's B operand wants (gait.h lmx_gait_packed_index; include/lmx.h lmx_tcn_weights_t):
//     block.{i}.conv{1,2}.w   [k * Q][N / 16][64][4]    entry [j * Q + q][nt][l][e] = W[16 nt + (l & 15)][16 q + 4 (l >> 4) + e][j]
//     block.{i}.conv{1,2}.b   [N]
//     block.{i}.res.w         [Q][N / 16][64][4], block.{i}.res.b [N]      only where the block's channel count changes
//     head.fc1.w [head][C], head.fc1.b [head], head.fc2.w [head], head.fc2.b [1]
//   with N = channels[i], Q = ceil(Cin / 16), Cin the convolution's inputs and C = channels[n_blocks - 1]
#pragma once
#include <stdint.h>

#include "tcn.h"
#include "weights_table.h"

enum { LMX_TCN_CONFIG_BYTES = 12 * 4 + 8 };

typedef LmxTableImage<lmx_tcn_weights_t> LmxTcnImage;  // cfg, p, data_offset, file_bytes, rows, refs

// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with
// the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_tcn_image_parse(const char* path, LmxTcnImage* img);
// the weights with every pointer into `data`, a copy of the image's data section [data_offset, file_bytes) in host or device memory
inline void lmx_tcn_bind(const LmxTcnImage& img, const char* data, lmx_tcn_weights_t* w) { lmx_table_bind(img, data, w); }
void lmx_tcn_fill_info(const LmxTcnImage& img, int max_clips, int max_samples, lmx_tcn_info_t* info);
