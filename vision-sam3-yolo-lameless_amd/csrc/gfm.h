// gfm.h — what the device forward (gfm.hip) and the host side (host_gfm.cpp: graph builder, configuration check, host forward) of the
// graph transformer share beyond gait.h (keep decision, packed weight order): the limits, the shapes, the dropout sites and the call
// checks.  Plain C++ without HIP types.
#pragma once
#include <vector>

#include "gait.h"

struct LmxTensorRow;  // weights_table.h

enum {
  LMX_GFM_MAX_D = 128,      // d_model
  LMX_GFM_MAX_FF = 512,     // feed-forward width
  LMX_GFM_MAX_IN = 64,      // input_dim
  LMX_GFM_MAX_DEGREE = 255, // the degrees travel as u8
  LMX_GFM_MAX_IDX = 32,     // rows of the shortest-path table: max_spd + 2
};

inline int lmx_gfm_head_dim(const lmx_gfm_weights_t& w) { return w.n_heads > 0 ? w.d_model / w.n_heads : 0; }
inline int lmx_gfm_n_sites(int n_layers) { return 6 * n_layers + 4; }
// widths of the small layers: D / 2 rounded up to a column tile (the attention pool and the node head run on the MFMA), D / 2 and D / 4
LMX_GAIT_HD inline int lmx_gfm_pool_dim(int D) { return (D / 2 + 15) / 16 * 16; }
inline int64_t lmx_gfm_packed_index(int o, int c, int K, int N) { return lmx_gait_packed_index(o, c, 0, K, N); }
inline int64_t lmx_gfm_packed_floats(int K, int N) { return lmx_gait_packed_floats(1, K, N); }
// q, k, v of one head are ONE linear layer of 3 dh outputs (rows q_i | k_i | v_i of q_proj, k_proj, v_proj); the heads follow each other
inline int64_t lmx_gfm_qkv_head_floats(const lmx_gfm_weights_t& w) { return lmx_gfm_packed_floats(w.d_model, 3 * lmx_gfm_head_dim(w)); }
// the scale of the scores: float(dh^-0.5), exact for dh = 16, the rounded 0.17677669 for dh = 32
inline float lmx_gfm_score_scale(int dh) { return (float)(1.0 / sqrt((double)dh)); }

// host_gfm.cpp: the configuration list of include/lmx.h (`who` opens the message; the offending field is named) and, with `pointers`,
// that every tensor is there and aligned
int lmx_gfm_check_config(const char* who, const lmx_gfm_weights_t* w, bool pointers);
// host_gfm.cpp: the weight table, stated once: appends every tensor `cfg` calls for (name, shape and the pointer of lmx_gfm_weights_t it
// fills) in the order of the weight image and of pack_tensors; `cfg` has passed lmx_gfm_check_config(.., false)
void lmx_gfm_tensor_rows(const lmx_gfm_weights_t& cfg, std::vector<LmxTensorRow>* rows);
// host_gfm.cpp: what both forwards check of a call after the configuration: the offsets, every N, S, p, the eval-only outputs.  On
// success *nodes = sum N, *cells = sum N^2, *max_n = the largest N.
int lmx_gfm_check_call(const char* who, const lmx_gfm_graphs_t* g, int S, double p, bool eval_outputs, int64_t* nodes, int64_t* cells, int* max_n);
