// gait.h — what the gait sequence models (the TCN: tcn.h; the gait transformer: xfm.h) have in common on both sides: the keep decision
// of MC dropout (include/lmx.h pins its text under lmx_h_tcn_keep_bits), the packed weight order of a convolution or linear layer, the
// pose constants, and the host arithmetic both host forwards share (dropout functor, row statistics, classifier head, call checks, clip
// window).  Plain C++ without HIP types, header-only: host_tcn.cpp and host_xfm.cpp compile the arithmetic under their own
// -ffp-contract=off; the function a kernel calls is marked for both sides when hipcc compiles it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lmx.h"

#if defined(__HIPCC__)
#define LMX_GAIT_HD __host__ __device__
#else
#define LMX_GAIT_HD
#endif

void lmx_set_error(const char* fmt, ...);  // api.hip

#define GAIT_REQUIRE(cond, ...)   \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

enum {
  LMX_GAIT_N_KEYPOINTS = 20,  // T-LEAP keypoints per frame
  LMX_GAIT_FEATURES = 44,     // 2 * 20 + centroid x, centroid y, bbox area, velocity
};

// the splitmix64 finaliser over (seed, stream, element): include/lmx.h has the text
LMX_GAIT_HD inline uint64_t lmx_gait_mix(uint64_t seed, uint64_t stream, uint64_t u) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((stream << 32) + u + 1);
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
LMX_GAIT_HD inline bool lmx_gait_keep(uint64_t seed, uint64_t stream, uint64_t u, uint64_t thr) { return (lmx_gait_mix(seed, stream, u) >> 32) >= thr; }
// thr = floor(p * 2^32) from the double p, 0 <= p < 1
inline uint64_t lmx_gait_threshold(double p) { return (uint64_t)floor(p * 4294967296.0); }
inline float lmx_gait_keep_scale(double p) { return (float)(1.0 / (1.0 - p)); }

// groups of 16 input channels of a convolution with `cin` inputs
inline int lmx_gait_groups(int cin) { return (cin + 15) / 16; }
// the float index of W[o][c][j] in the packed order [k * Q][N / 16][64][4] (Q = groups of cin, N = cout); a linear layer has one tap
inline int64_t lmx_gait_packed_index(int o, int c, int j, int cin, int cout) {
  const int Q = lmx_gait_groups(cin), NT = cout / 16;
  return ((((int64_t)j * Q + c / 16) * NT + o / 16) * 64 + ((c % 16) / 4) * 16 + o % 16) * 4 + c % 4;
}
inline int64_t lmx_gait_packed_floats(int taps, int cin, int cout) { return (int64_t)taps * lmx_gait_groups(cin) * (cout / 16) * 256; }

// MC dropout of one (clip, sample) on the host: S = 0 passes every value through
struct LmxGaitDrop {
  bool on;
  uint64_t seed, thr, sample, n_sites;
  float scale;
  LmxGaitDrop(int S, const uint64_t* seeds, int clip, double p, int sample_, int n_sites_)
      : on(S > 0), seed(S > 0 ? seeds[clip] : 0), thr(S > 0 ? lmx_gait_threshold(p) : 0), sample((uint64_t)sample_), n_sites((uint64_t)n_sites_),
        scale(S > 0 ? lmx_gait_keep_scale(p) : 1.0f) {}
  float operator()(float v, int site, uint64_t u) const {
    if (!on) return v;
    return lmx_gait_keep(seed, sample * n_sites + (uint64_t)site, u, thr) ? v * scale : 0.0f;
  }
};

// out = {mean, unbiased standard deviation} of one row of pred, read in sample order (S = 0: the one prediction and 0)
inline void lmx_gait_row_stats(const float* row, int S, float* out) {
  if (S == 0) {
    out[0] = row[0];
    out[1] = 0.0f;
    return;
  }
  float sum = 0.0f, ss = 0.0f;
  for (int s = 0; s < S; ++s) sum += row[s];
  const float mean = sum / (float)S;
  for (int s = 0; s < S; ++s) ss += (row[s] - mean) * (row[s] - mean);
  out[0] = mean;
  out[1] = sqrtf(ss / (float)(S - 1));
}

// the classifier head: z = fc2(drop(relu(fc1(pooled)))) with `site` the head's dropout site; fc1 is [H][C], H <= 64
inline float lmx_gait_head(const float* pooled, int C, int H, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                           const LmxGaitDrop& drop, int site) {
  float hid[64];
  for (int j = 0; j < H; ++j) {
    float sum = fc1_b[j];
    for (int c = 0; c < C; ++c) sum += fc1_w[(size_t)j * C + c] * pooled[c];
    hid[j] = drop(fmaxf(sum, 0.0f), site, (uint64_t)j);
  }
  float z = fc2_b[0];
  for (int j = 0; j < H; ++j) z += fc2_w[j] * hid[j];
  return z;
}

// the checks every forward and every handle makes of n, T, S and p (LMX_EINVAL with the field named); `limit` words T's bound
// ("" for a constant, "max_len " for the transformer's table)
inline int lmx_gait_check_call(const char* who, int n, int T, int S, double p, int max_T, const char* limit) {
  GAIT_REQUIRE(n >= 0, "%s: n = %d clips", who, n);
  GAIT_REQUIRE(T >= 1 && T <= max_T, "%s: T %d outside 1 .. %s%d", who, T, limit, max_T);
  GAIT_REQUIRE(S == 0 || (S >= 2 && S <= 65535), "%s: S %d (0: eval mode; 2 .. 65535 samples; the standard deviation of 1 is undefined)", who, S);
  GAIT_REQUIRE(S == 0 || (p >= 0.0 && p < 1.0), "%s: p %g outside [0, 1)", who, p);
  return LMX_OK;
}

// a clip of T0 frames in `target` steps, centre-cropped or centre-padded with the shorter half in front: frames [first, first + rows)
// land at step `at`
struct LmxGaitWindow {
  int first, rows, at;
};
LMX_GAIT_HD inline LmxGaitWindow lmx_gait_window(int T0, int target) {
  if (T0 >= target) return {(T0 - target) / 2, target, 0};
  return {0, T0, (target - T0) / 2};
}
// what lmx_h_tcn_features and lmx_h_xfm_mask check of a clip before they read it (`pointers`: every array is there)
inline int lmx_gait_check_clip(const char* who, int T0, int target, bool pointers, const int* n_kp) {
  GAIT_REQUIRE(T0 >= 1 && T0 <= (1 << 24), "%s: T0 = %d frames", who, T0);
  GAIT_REQUIRE(target >= 1 && target <= (1 << 24), "%s: target = %d steps", who, target);
  GAIT_REQUIRE(pointers, "%s: null pointer", who);
  for (int t = 0; t < T0; ++t)
    GAIT_REQUIRE(n_kp[t] >= 0 && n_kp[t] <= LMX_GAIT_N_KEYPOINTS, "%s: n_kp[%d] = %d outside 0 .. %d", who, t, n_kp[t], LMX_GAIT_N_KEYPOINTS);
  return LMX_OK;
}
