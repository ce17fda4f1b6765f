// gnn.h — what the device forward (gnn.hip) and the host side (host_gnn.cpp: graph builder, both encodings, configuration check, host
// forward) of GraphGPS share beyond gait.h (keep decision, packed weight order): the limits, the dropout sites and the call checks.
// Plain C++ without HIP types.
#pragma once
#include <vector>

#include "gait.h"

struct LmxTensorRow;  // weights_table.h

enum {
  LMX_GNN_MAX_D = 128,   // d_model
  LMX_GNN_MAX_FF = 512,  // feed-forward width
  LMX_GNN_MAX_IN = 64,   // input_dim
};

inline int lmx_gnn_head_dim(const lmx_gnn_weights_t& w) { return w.n_heads > 0 ? w.d_model / w.n_heads : 0; }
// five sites per live layer and the node head's; the graph classifier's two are never drawn
LMX_GAIT_HD inline int lmx_gnn_n_sites(int n_layers) { return 5 * n_layers + 1; }
inline int64_t lmx_gnn_packed_index(int o, int c, int K, int N) { return lmx_gait_packed_index(o, c, 0, K, N); }
inline int64_t lmx_gnn_packed_floats(int K, int N) { return lmx_gait_packed_floats(1, K, N); }
inline int64_t lmx_gnn_qkv_head_floats(const lmx_gnn_weights_t& w) { return lmx_gnn_packed_floats(w.d_model, 3 * lmx_gnn_head_dim(w)); }
// the scale of the scores: float(dh^-0.5)
inline float lmx_gnn_score_scale(int dh) { return (float)(1.0 / sqrt((double)dh)); }
// floats of one workgroup's workspace slice: Bx | Dx | Ex of every node and, with more than one live layer, ea of every edge
inline int64_t lmx_gnn_slice_floats(int max_nodes, int max_edges, int d_model, int n_layers) {
  return (int64_t)max_nodes * 3 * d_model + (n_layers > 1 ? (int64_t)max_edges * d_model : 0);
}

// host_gnn.cpp: the configuration list of include/lmx.h (`who` opens the message; the offending field is named) and, with `pointers`,
// that every tensor is there and aligned
int lmx_gnn_check_config(const char* who, const lmx_gnn_weights_t* w, bool pointers);
// host_gnn.cpp: the weight table, stated once: appends every tensor `cfg` calls for (name, shape and the pointer of lmx_gnn_weights_t it
// fills) in the order of the weight image and of pack_tensors; `cfg` has passed lmx_gnn_check_config(.., false)
void lmx_gnn_tensor_rows(const lmx_gnn_weights_t& cfg, std::vector<LmxTensorRow>* rows);
// host_gnn.cpp: what both forwards check of a call after the configuration: the offsets, every N and E, S, p, the outputs of the mode.
// On success *nodes = sum N, *max_n and *max_e = the largest N and E.
int lmx_gnn_check_call(const char* who, const lmx_gnn_weights_t* w, const lmx_gnn_graphs_t* g, int S, double p, bool mc_outputs, bool eval_outputs,
                       int64_t* nodes, int* max_n, int* max_e);
