// tcn.h — what the device forward (tcn.hip), the host forward (host_tcn.cpp) and the image reader (host_tcn_image.cpp) of the TCN gait
// model share beyond gait.h (keep decision, packed weight order): the limits and the configuration check.  Plain C++ without HIP types.
#pragma once
#include <vector>

#include "gait.h"

struct LmxTensorRow;  // weights_table.h

enum {
  LMX_TCN_MAX_CH = 64,    // channels and input_dim
  LMX_TCN_MAX_T = 256,    // time steps of one clip
  LMX_TCN_MAX_HEAD = 64,  // hidden width of the head
};

inline int lmx_tcn_cin(const lmx_tcn_weights_t& w, int block) { return block ? w.channels[block - 1] : w.input_dim; }

// host_tcn.cpp: the configuration list of include/lmx.h (`who` opens the message; the offending field is named) and, with
// `pointers`, that every tensor the configuration calls for is there
int lmx_tcn_check_config(const char* who, const lmx_tcn_weights_t* w, bool pointers);
// host_tcn.cpp: the weight table, stated once: appends every tensor `cfg` calls for (name, shape and the pointer of lmx_tcn_weights_t it
// fills) in the order of the weight image and of pack_tensors; `cfg` has passed lmx_tcn_check_config(.., false)
void lmx_tcn_tensor_rows(const lmx_tcn_weights_t& cfg, std::vector<LmxTensorRow>* rows);
// the checks both forwards and the handle share after the configuration: n, T, S, p (LMX_EINVAL with the field named)
inline int lmx_tcn_check_call(const char* who, int n, int T, int S, double p) { return lmx_gait_check_call(who, n, T, S, p, LMX_TCN_MAX_T, ""); }
// 1 + 2 (k - 1) (2^n_blocks - 1)
int lmx_tcn_receptive_field(int k, int n_blocks);
