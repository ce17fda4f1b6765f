// tcn.h — what the device forward (tcn.hip), the host forward (host_tcn.cpp) and the image reader (host_tcn_image.cpp) of the TCN gait
// model share: the keep decision of MC dropout (include/lmx.h pins its text), the packed weight order and the configuration check.
// Plain C++ without HIP types; the two functions a kernel calls are marked for both sides when hipcc compiles them.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lmx.h"

#if defined(__HIPCC__)
#define LMX_TCN_HD __host__ __device__
#else
#define LMX_TCN_HD
#endif

enum {
  LMX_TCN_MAX_CH = 64,      // channels and input_dim
  LMX_TCN_MAX_T = 256,      // time steps of one clip
  LMX_TCN_MAX_HEAD = 64,    // hidden width of the head
  LMX_TCN_N_KEYPOINTS = 20, // T-LEAP keypoints per frame
  LMX_TCN_FEATURES = 44,    // 2 * 20 + centroid x, centroid y, bbox area, velocity
};

// the splitmix64 finaliser over (seed, stream, element): include/lmx.h has the text
LMX_TCN_HD inline uint64_t lmx_tcn_mix(uint64_t seed, uint64_t stream, uint64_t u) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((stream << 32) + u + 1);
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
LMX_TCN_HD inline bool lmx_tcn_keep(uint64_t seed, uint64_t stream, uint64_t u, uint64_t thr) { return (lmx_tcn_mix(seed, stream, u) >> 32) >= thr; }
// thr = floor(p * 2^32) from the double p, 0 <= p < 1
inline uint64_t lmx_tcn_threshold(double p) { return (uint64_t)floor(p * 4294967296.0); }
inline float lmx_tcn_keep_scale(double p) { return (float)(1.0 / (1.0 - p)); }

// groups of 16 input channels of a convolution with `cin` inputs
inline int lmx_tcn_groups(int cin) { return (cin + 15) / 16; }
// the float index of W[o][c][j] in the packed order [k * Q][N / 16][64][4] (Q = groups of cin, N = cout)
inline int64_t lmx_tcn_packed_index(int o, int c, int j, int cin, int cout) {
  const int Q = lmx_tcn_groups(cin), NT = cout / 16;
  return ((((int64_t)j * Q + c / 16) * NT + o / 16) * 64 + ((c % 16) / 4) * 16 + o % 16) * 4 + c % 4;
}
inline int64_t lmx_tcn_packed_floats(int taps, int cin, int cout) { return (int64_t)taps * lmx_tcn_groups(cin) * (cout / 16) * 256; }
inline int lmx_tcn_cin(const lmx_tcn_weights_t& w, int block) { return block ? w.channels[block - 1] : w.input_dim; }

// host_tcn.cpp: the configuration list of include/lmx.h (`who` opens the message; the offending field is named) and, with
// `pointers`, that every tensor the configuration calls for is there
int lmx_tcn_check_config(const char* who, const lmx_tcn_weights_t* w, bool pointers);
// 1 + 2 (k - 1) (2^n_blocks - 1)
int lmx_tcn_receptive_field(int k, int n_blocks);
