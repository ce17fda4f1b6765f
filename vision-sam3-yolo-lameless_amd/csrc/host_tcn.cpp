// host_tcn.cpp — the TCN gait model on the HOST (include/lmx.h "The TCN gait model"): the keep bits of MC dropout, the whole forward in
// plain C++ (f32, sequential sums, no contraction: the Makefile builds this file with -ffp-contract=off) and the feature arithmetic of
// services/tcn-pipeline/app/main.py:255-328.  No HIP here: it makes the service testable without a GPU and is what the stand-alone
// sanitizer program (tests/tcn_check_main.cpp) runs.  The device forward is csrc/tcn.hip; both read the packed weights of tcn.h.
#include <string.h>

#include <vector>

#include "tcn.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define TCN_REQUIRE(cond, ...)    \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

int lmx_tcn_receptive_field(int k, int n_blocks) { return 1 + 2 * (k - 1) * ((1 << n_blocks) - 1); }

int lmx_tcn_check_config(const char* who, const lmx_tcn_weights_t* w, bool pointers) {
  TCN_REQUIRE(w != nullptr, "%s: null weights", who);
  TCN_REQUIRE(w->n_blocks >= 1 && w->n_blocks <= LMX_TCN_MAX_BLOCKS, "%s: n_blocks %d outside 1 .. %d", who, w->n_blocks, LMX_TCN_MAX_BLOCKS);
  TCN_REQUIRE(w->input_dim >= 1 && w->input_dim <= LMX_TCN_MAX_CH, "%s: input_dim %d outside 1 .. %d", who, w->input_dim, LMX_TCN_MAX_CH);
  TCN_REQUIRE(w->k == 2 || w->k == 3, "%s: k %d is neither 2 nor 3", who, w->k);
  TCN_REQUIRE(w->head >= 1 && w->head <= LMX_TCN_MAX_HEAD, "%s: head %d outside 1 .. %d", who, w->head, LMX_TCN_MAX_HEAD);
  for (int i = 0; i < w->n_blocks; ++i)
    TCN_REQUIRE(w->channels[i] >= 16 && w->channels[i] <= LMX_TCN_MAX_CH && w->channels[i] % 16 == 0,
                "%s: channels[%d] = %d is not a multiple of 16 up to %d", who, i, w->channels[i], LMX_TCN_MAX_CH);
  if (!pointers) return LMX_OK;
  for (int i = 0; i < w->n_blocks; ++i) {
    for (int s = 0; s < 2; ++s) {
      TCN_REQUIRE(w->conv_w[i][s] && w->conv_b[i][s], "%s: block %d conv%d has no weights", who, i, s + 1);
      TCN_REQUIRE(((uintptr_t)w->conv_w[i][s] & 15) == 0, "%s: block %d conv%d weights are not 16-byte aligned", who, i, s + 1);
    }
    const bool changes = lmx_tcn_cin(*w, i) != w->channels[i];
    TCN_REQUIRE((w->res_w[i] != nullptr) == changes && (w->res_b[i] != nullptr) == changes,
                "%s: block %d has %d inputs and %d outputs, so it %s a residual convolution", who, i, lmx_tcn_cin(*w, i), w->channels[i],
                changes ? "needs" : "must not have");
    TCN_REQUIRE(((uintptr_t)w->res_w[i] & 15) == 0, "%s: block %d residual weights are not 16-byte aligned", who, i);
  }
  TCN_REQUIRE(w->fc1_w && w->fc1_b && w->fc2_w && w->fc2_b, "%s: the head has no weights", who);
  TCN_REQUIRE(((uintptr_t)w->fc1_w & 15) == 0, "%s: the head's fc1 weights are not 16-byte aligned", who);
  return LMX_OK;
}

extern "C" int lmx_h_tcn_keep_bits(uint64_t seed, int sample, int site, int n_sites, int64_t count, double p, uint8_t* keep_host) {
  TCN_REQUIRE(sample >= 0 && n_sites >= 1 && site >= 0 && site < n_sites, "lmx_h_tcn_keep_bits: sample %d, site %d of %d", sample, site, n_sites);
  TCN_REQUIRE(count >= 0 && count <= ((int64_t)1 << 32) - 1, "lmx_h_tcn_keep_bits: count %lld", (long long)count);
  TCN_REQUIRE(p >= 0.0 && p < 1.0, "lmx_h_tcn_keep_bits: p %g outside [0, 1)", p);
  TCN_REQUIRE(keep_host || count == 0, "lmx_h_tcn_keep_bits: null keep_host");
  const uint64_t thr = lmx_tcn_threshold(p), stream = (uint64_t)sample * (uint64_t)n_sites + (uint64_t)site;
  for (int64_t u = 0; u < count; ++u) keep_host[u] = lmx_tcn_keep(seed, stream, (uint64_t)u, thr) ? 1 : 0;
  return LMX_OK;
}

namespace {

struct Drop {
  bool on;
  uint64_t seed, thr, sample, n_sites;
  float scale;
  float operator()(float v, int site, uint64_t u) const {
    if (!on) return v;
    return lmx_tcn_keep(seed, sample * n_sites + (uint64_t)site, u, thr) ? v * scale : 0.0f;
  }
};

// out[t][o] = b[o] + sum over taps j (first to last) and input channels c (ascending) of W[o][c][j] * in[t - (taps - 1 - j) d][c]
void conv(const float* in, int cin, float* out, int cout, const float* w, const float* b, int taps, int d, int T) {
  for (int t = 0; t < T; ++t)
    for (int o = 0; o < cout; ++o) {
      float s = b[o];
      for (int j = 0; j < taps; ++j) {
        const int ts = t - (taps - 1 - j) * d;
        if (ts < 0) continue;
        for (int c = 0; c < cin; ++c) s += w[lmx_tcn_packed_index(o, c, j, cin, cout)] * in[(size_t)ts * cin + c];
      }
      out[(size_t)t * cout + o] = s;
    }
}

}  // namespace

extern "C" int lmx_h_tcn_forward(const lmx_tcn_weights_t* w, const float* x, const uint64_t* seeds, int n, int T, int S, double p, float* pred,
                                 float* stats, float* trunk) {
  if (const int rc = lmx_tcn_check_config("lmx_h_tcn_forward", w, true)) return rc;
  TCN_REQUIRE(n >= 0, "lmx_h_tcn_forward: n = %d clips", n);
  TCN_REQUIRE(T >= 1 && T <= LMX_TCN_MAX_T, "lmx_h_tcn_forward: T %d outside 1 .. %d", T, LMX_TCN_MAX_T);
  TCN_REQUIRE(S == 0 || (S >= 2 && S <= 65535), "lmx_h_tcn_forward: S %d (0: eval mode; 2 .. 65535 samples; the standard deviation of 1 is undefined)", S);
  TCN_REQUIRE(S == 0 || (p >= 0.0 && p < 1.0), "lmx_h_tcn_forward: p %g outside [0, 1)", p);
  if (n == 0) return LMX_OK;
  TCN_REQUIRE(x && pred && stats && (seeds || S == 0), "lmx_h_tcn_forward: null pointer");
  const int F = w->input_dim, nb = w->n_blocks, Smax = S > 0 ? S : 1, C = w->channels[nb - 1], H = w->head;
  std::vector<float> cur((size_t)T * LMX_TCN_MAX_CH), h((size_t)T * LMX_TCN_MAX_CH), y((size_t)T * LMX_TCN_MAX_CH), r((size_t)T * LMX_TCN_MAX_CH);
  for (int i = 0; i < n; ++i) {
    for (int s = 0; s < Smax; ++s) {
      const Drop drop = {S > 0, S > 0 ? seeds[i] : 0, S > 0 ? lmx_tcn_threshold(p) : 0, (uint64_t)s, (uint64_t)(2 * nb + 1),
                         S > 0 ? lmx_tcn_keep_scale(p) : 1.0f};
      memcpy(cur.data(), x + (size_t)i * T * F, (size_t)T * F * sizeof(float));
      for (int b = 0; b < nb; ++b) {
        const int cin = lmx_tcn_cin(*w, b), co = w->channels[b], d = 1 << b;
        conv(cur.data(), cin, h.data(), co, w->conv_w[b][0], w->conv_b[b][0], w->k, d, T);
        for (int t = 0; t < T; ++t)
          for (int o = 0; o < co; ++o) h[(size_t)t * co + o] = drop(fmaxf(h[(size_t)t * co + o], 0.0f), 2 * b, (uint64_t)o * T + t);
        conv(h.data(), co, y.data(), co, w->conv_w[b][1], w->conv_b[b][1], w->k, d, T);
        const float* res = cur.data();
        if (w->res_w[b]) {
          conv(cur.data(), cin, r.data(), co, w->res_w[b], w->res_b[b], 1, 1, T);
          res = r.data();
        }
        for (int t = 0; t < T; ++t)
          for (int o = 0; o < co; ++o) {
            const float v = drop(fmaxf(y[(size_t)t * co + o], 0.0f), 2 * b + 1, (uint64_t)o * T + t);
            y[(size_t)t * co + o] = fmaxf(v + res[(size_t)t * co + o], 0.0f);
          }
        cur.swap(y);
      }
      if (trunk) memcpy(trunk + ((size_t)i * Smax + s) * T * C, cur.data(), (size_t)T * C * sizeof(float));
      float pooled[LMX_TCN_MAX_CH], hid[LMX_TCN_MAX_HEAD];
      for (int c = 0; c < C; ++c) {
        float sum = 0.0f;
        for (int t = 0; t < T; ++t) sum += cur[(size_t)t * C + c];
        pooled[c] = sum / (float)T;
      }
      for (int j = 0; j < H; ++j) {
        float sum = w->fc1_b[j];
        for (int c = 0; c < C; ++c) sum += w->fc1_w[(size_t)j * C + c] * pooled[c];
        hid[j] = drop(fmaxf(sum, 0.0f), 2 * nb, (uint64_t)j);
      }
      float z = w->fc2_b[0];
      for (int j = 0; j < H; ++j) z += w->fc2_w[j] * hid[j];
      pred[(size_t)i * Smax + s] = 1.0f / (1.0f + expf(-z));
    }
    const float* row = pred + (size_t)i * Smax;
    if (S == 0) {
      stats[2 * i] = row[0];
      stats[2 * i + 1] = 0.0f;
    } else {
      float sum = 0.0f, ss = 0.0f;
      for (int s = 0; s < S; ++s) sum += row[s];
      const float mean = sum / (float)S;
      for (int s = 0; s < S; ++s) ss += (row[s] - mean) * (row[s] - mean);
      stats[2 * i] = mean;
      stats[2 * i + 1] = sqrtf(ss / (float)(S - 1));
    }
  }
  return LMX_OK;
}

extern "C" int lmx_h_tcn_features(const double* kp, const int* n_kp, const double* bbox, int T0, int target, float* out) {
  TCN_REQUIRE(T0 >= 1 && T0 <= (1 << 24), "lmx_h_tcn_features: T0 = %d frames", T0);
  TCN_REQUIRE(target >= 1 && target <= (1 << 24), "lmx_h_tcn_features: target = %d steps", target);
  TCN_REQUIRE(kp && n_kp && bbox && out, "lmx_h_tcn_features: null pointer");
  const int F = LMX_TCN_FEATURES, K = LMX_TCN_N_KEYPOINTS;
  for (int t = 0; t < T0; ++t) TCN_REQUIRE(n_kp[t] >= 0 && n_kp[t] <= K, "lmx_h_tcn_features: n_kp[%d] = %d outside 0 .. %d", t, n_kp[t], K);
  // the rows of the clip that reach the output: [first, first + rows) of the clip land at row `at`
  const int first = T0 >= target ? (T0 - target) / 2 : 0, rows = T0 >= target ? target : T0, at = T0 >= target ? 0 : (target - T0) / 2;
  memset(out, 0, (size_t)target * F * sizeof(float));
  auto centroid_x = [&](int t) { return (float)((bbox[4 * t] + bbox[4 * t + 2]) / 2 / 1280); };
  for (int r = 0; r < rows; ++r) {
    const int t = first + r;
    const double* b = bbox + 4 * (size_t)t;
    const double bw = b[2] - b[0], bh = b[3] - b[1], dw = bw > 1 ? bw : 1, dh = bh > 1 ? bh : 1;
    float* o = out + (size_t)(at + r) * F;
    for (int i = 0; i < n_kp[t]; ++i) {
      o[2 * i] = (float)((kp[((size_t)t * K + i) * 2] - b[0]) / dw);
      o[2 * i + 1] = (float)((kp[((size_t)t * K + i) * 2 + 1] - b[1]) / dh);
    }
    o[40] = centroid_x(t);
    o[41] = (float)((b[1] + b[3]) / 2 / 720);
    o[42] = (float)(bw * bh / (1280 * 720));
    o[43] = t > 0 ? centroid_x(t) - centroid_x(t - 1) : 0.0f;  // np.diff of the float32 column: a float32 difference
  }
  return LMX_OK;
}
