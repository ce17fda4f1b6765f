// gfm_image.h — the weight image of the graph transformer (written by lmx/native.py write_gfm_image, read by host_gfm_image.cpp) as
// the model handle (graph_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind GFM = 6:
//   config  at 48      8 x i32 (input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd) then 1 x f64 (p)
//   tensors            all f32, named as the fields of lmx_gfm_weights_t (include/lmx.h has their shapes and orders), the per-layer
//                      ones as layer.{l}.<field>: 14 in front (in_w .. e2_b), 17 per layer (ln1_g .. vout_b), 26 behind (vu1_w .. nh2_b);
//                      the table is lmx_gfm_tensor_rows (host_gfm.cpp)
#pragma once
#include <stdint.h>

#include "gfm.h"
#include "weights_table.h"

enum { LMX_GFM_CONFIG_BYTES = 8 * 4 + 8 };

typedef LmxTableImage<lmx_gfm_weights_t> LmxGfmImage;  // cfg, p, data_offset, file_bytes, rows, refs

// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with
// the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_gfm_image_parse(const char* path, LmxGfmImage* img);
// the weights with every pointer into `data`, a copy of the image's data section [data_offset, file_bytes) in host or device memory
inline void lmx_gfm_bind(const LmxGfmImage& img, const char* data, lmx_gfm_weights_t* w) { lmx_table_bind(img, data, w); }
void lmx_gfm_fill_info(const LmxGfmImage& img, int max_graphs, int max_nodes_total, int max_samples, lmx_gfm_info_t* info);
