// xfm.h — what the device forward (xfm.hip), the host forward (host_xfm.cpp) and the image reader (host_xfm_image.cpp) of the gait
// transformer share beyond gait.h (keep decision, packed weight order): the limits, the shapes and the configuration check.  Plain C++
// without HIP types.
#pragma once
#include <vector>

#include "gait.h"

struct LmxTensorRow;  // weights_table.h

enum {
  LMX_XFM_MAX_D = 64,     // d_model and input_dim
  LMX_XFM_MAX_FF = 256,   // feed-forward width
  LMX_XFM_MAX_HEAD = 64,  // hidden width of the classifier
  LMX_XFM_MAX_LEN = 160,  // rows of the positional table, and so of a clip
};

inline int lmx_xfm_head_dim(const lmx_xfm_weights_t& w) { return w.n_heads > 0 ? w.d_model / w.n_heads : 0; }
inline int lmx_xfm_n_sites(const lmx_xfm_weights_t& w) { return 4 * w.n_layers + 2; }
// every linear layer W [N][K] is stored as a convolution with one tap in the shared B-operand order (gait.h lmx_gait_packed_index)
inline int64_t lmx_xfm_packed_index(int o, int c, int K, int N) { return lmx_gait_packed_index(o, c, 0, K, N); }
inline int64_t lmx_xfm_packed_floats(int K, int N) { return lmx_gait_packed_floats(1, K, N); }
// q, k, v of one head are ONE linear layer of 3 dh outputs (rows q_i | k_i | v_i of in_proj_weight); the heads follow each other
inline int64_t lmx_xfm_qkv_head_floats(const lmx_xfm_weights_t& w) { return lmx_xfm_packed_floats(w.d_model, 3 * lmx_xfm_head_dim(w)); }
// the scale of q: float(1 / sqrt(dh)), exact for dh = 16, the rounded 0.17677669 for dh = 32
inline float lmx_xfm_q_scale(int dh) { return (float)(1.0 / sqrt((double)dh)); }

// host_xfm.cpp: the configuration list of include/lmx.h (`who` opens the message; the offending field is named) and, with
// `pointers`, that every tensor is there and aligned
int lmx_xfm_check_config(const char* who, const lmx_xfm_weights_t* w, bool pointers);
// host_xfm.cpp: the weight table, stated once: appends every tensor `cfg` calls for (name, shape and the pointer of lmx_xfm_weights_t it
// fills) in the order of the weight image and of pack_tensors; `cfg` has passed lmx_xfm_check_config(.., false)
void lmx_xfm_tensor_rows(const lmx_xfm_weights_t& cfg, std::vector<LmxTensorRow>* rows);
// the checks both forwards and the handle share after the configuration: n, T, S, p, saliency (LMX_EINVAL with the field named)
inline int lmx_xfm_check_call(const char* who, const lmx_xfm_weights_t* w, int n, int T, int S, double p, bool saliency) {
  if (const int rc = lmx_gait_check_call(who, n, T, S, p, w->max_len, "max_len ")) return rc;
  GAIT_REQUIRE(!saliency || S == 0, "%s: saliency is read in eval mode only, S = %d", who, S);
  return LMX_OK;
}
