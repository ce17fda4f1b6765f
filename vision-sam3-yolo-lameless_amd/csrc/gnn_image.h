// gnn_image.h — the weight image of GraphGPS (written by lmx/native.py write_gnn_image, read by host_gnn_image.cpp) as the model handle
// (graph_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind GNN = 7:
//   config  at 48      8 x i32 (input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim, 0) then 1 x f64 (p)
//   tensors            all f32, named as the fields of lmx_gnn_weights_t (include/lmx.h has their shapes and orders), the per-layer
//                      ones as layer.{l}.<field>: 20 in front (in_w .. ee_beta), 32 per layer (ln1_g .. ff2_b; the LAST layer has no
//                      eu1_w .. bne_var, 24 there), 16 behind (lnf_g .. cl3_b): the table of lmx_gnn_tensor_rows (host_gnn.cpp)
#pragma once
#include <stdint.h>

#include "gnn.h"
#include "weights_table.h"

enum { LMX_GNN_CONFIG_BYTES = 8 * 4 + 8 };

typedef LmxTableImage<lmx_gnn_weights_t> LmxGnnImage;  // cfg, p, data_offset, file_bytes, rows, refs

// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with
// the offending field named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_gnn_image_parse(const char* path, LmxGnnImage* img);
// the weights with every pointer into `data`, a copy of the image's data section [data_offset, file_bytes) in host or device memory
inline void lmx_gnn_bind(const LmxGnnImage& img, const char* data, lmx_gnn_weights_t* w) { lmx_table_bind(img, data, w); }
void lmx_gnn_fill_info(const LmxGnnImage& img, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, lmx_gnn_info_t* info);
