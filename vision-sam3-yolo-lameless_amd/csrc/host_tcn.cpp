// host_tcn.cpp — the TCN gait model on the HOST (include/lmx.h "The TCN gait model"): the keep bits of MC dropout, the whole forward in
// plain C++ (f32, sequential sums, no contraction: the Makefile builds this file with -ffp-contract=off) and the feature arithmetic of
// services/tcn-pipeline/app/main.py:255-328.  No HIP here: it makes the service testable without a GPU and is what the stand-alone
// sanitizer program (tests/tcn_check_main.cpp) runs.  The device forward is csrc/tcn.hip; both read the packed weights of gait.h.
#include <string.h>

#include <vector>

#include "tcn.h"
#include "weights_table.h"

int lmx_tcn_receptive_field(int k, int n_blocks) { return 1 + 2 * (k - 1) * ((1 << n_blocks) - 1); }

int lmx_tcn_check_config(const char* who, const lmx_tcn_weights_t* w, bool pointers) {
  GAIT_REQUIRE(w != nullptr, "%s: null weights", who);
  GAIT_REQUIRE(w->n_blocks >= 1 && w->n_blocks <= LMX_TCN_MAX_BLOCKS, "%s: n_blocks %d outside 1 .. %d", who, w->n_blocks, LMX_TCN_MAX_BLOCKS);
  GAIT_REQUIRE(w->input_dim >= 1 && w->input_dim <= LMX_TCN_MAX_CH, "%s: input_dim %d outside 1 .. %d", who, w->input_dim, LMX_TCN_MAX_CH);
  GAIT_REQUIRE(w->k == 2 || w->k == 3, "%s: k %d is neither 2 nor 3", who, w->k);
  GAIT_REQUIRE(w->head >= 1 && w->head <= LMX_TCN_MAX_HEAD, "%s: head %d outside 1 .. %d", who, w->head, LMX_TCN_MAX_HEAD);
  for (int i = 0; i < w->n_blocks; ++i)
    GAIT_REQUIRE(w->channels[i] >= 16 && w->channels[i] <= LMX_TCN_MAX_CH && w->channels[i] % 16 == 0,
                "%s: channels[%d] = %d is not a multiple of 16 up to %d", who, i, w->channels[i], LMX_TCN_MAX_CH);
  if (!pointers) return LMX_OK;
  for (int i = 0; i < w->n_blocks; ++i) {
    for (int s = 0; s < 2; ++s) {
      GAIT_REQUIRE(w->conv_w[i][s] && w->conv_b[i][s], "%s: block %d conv%d has no weights", who, i, s + 1);
      GAIT_REQUIRE(((uintptr_t)w->conv_w[i][s] & 15) == 0, "%s: block %d conv%d weights are not 16-byte aligned", who, i, s + 1);
    }
    const bool changes = lmx_tcn_cin(*w, i) != w->channels[i];
    GAIT_REQUIRE((w->res_w[i] != nullptr) == changes && (w->res_b[i] != nullptr) == changes,
                "%s: block %d has %d inputs and %d outputs, so it %s a residual convolution", who, i, lmx_tcn_cin(*w, i), w->channels[i],
                changes ? "needs" : "must not have");
    GAIT_REQUIRE(((uintptr_t)w->res_w[i] & 15) == 0, "%s: block %d residual weights are not 16-byte aligned", who, i);
  }
  GAIT_REQUIRE(w->fc1_w && w->fc1_b && w->fc2_w && w->fc2_b, "%s: the head has no weights", who);
  GAIT_REQUIRE(((uintptr_t)w->fc1_w & 15) == 0, "%s: the head's fc1 weights are not 16-byte aligned", who);
  return LMX_OK;
}

// The weight table (tcn.h): the tensors of the image and of lmx.tcn.pack_tensors in their order.  A block whose input width equals its
// channels has no residual convolution.
void lmx_tcn_tensor_rows(const lmx_tcn_weights_t& c, std::vector<LmxTensorRow>* rows) {
#define ROW(member, index, name, field, ...) LMX_ROW(lmx_tcn_weights_t, member, index, name, field, __VA_ARGS__)
  for (int i = 0; i < c.n_blocks; ++i) {
    const int cin = lmx_tcn_cin(c, i), N = c.channels[i];
    const std::string b = "block." + std::to_string(i) + ".";
    ROW(conv_w, 2 * i, b + "conv1.w", "k, the block's inputs, channels", c.k * lmx_gait_groups(cin), N / 16, 64, 4);
    ROW(conv_b, 2 * i, b + "conv1.b", "channels", N);
    ROW(conv_w, 2 * i + 1, b + "conv2.w", "k, channels", c.k * lmx_gait_groups(N), N / 16, 64, 4);
    ROW(conv_b, 2 * i + 1, b + "conv2.b", "channels", N);
    if (cin != N) {
      ROW(res_w, i, b + "res.w", "the block's inputs, channels", lmx_gait_groups(cin), N / 16, 64, 4);
      ROW(res_b, i, b + "res.b", "channels", N);
    }
  }
  ROW(fc1_w, 0, "head.fc1.w", "head, channels", c.head, c.channels[c.n_blocks - 1]);
  ROW(fc1_b, 0, "head.fc1.b", "head", c.head);
  ROW(fc2_w, 0, "head.fc2.w", "head", c.head);
  ROW(fc2_b, 0, "head.fc2.b", "one class", 1);
#undef ROW
}

extern "C" int lmx_h_tcn_tensors(const char* who, const lmx_tcn_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host) {
  return lmx_table_export("lmx_h_tcn_tensors", who, config_host, lmx_tcn_check_config, lmx_tcn_tensor_rows, rows_host, cap, n_host);
}

extern "C" int lmx_h_tcn_keep_bits(uint64_t seed, int sample, int site, int n_sites, int64_t count, double p, uint8_t* keep_host) {
  GAIT_REQUIRE(sample >= 0 && n_sites >= 1 && site >= 0 && site < n_sites, "lmx_h_tcn_keep_bits: sample %d, site %d of %d", sample, site, n_sites);
  GAIT_REQUIRE(count >= 0 && count <= ((int64_t)1 << 32) - 1, "lmx_h_tcn_keep_bits: count %lld", (long long)count);
  GAIT_REQUIRE(p >= 0.0 && p < 1.0, "lmx_h_tcn_keep_bits: p %g outside [0, 1)", p);
  GAIT_REQUIRE(keep_host || count == 0, "lmx_h_tcn_keep_bits: null keep_host");
  const uint64_t thr = lmx_gait_threshold(p), stream = (uint64_t)sample * (uint64_t)n_sites + (uint64_t)site;
  for (int64_t u = 0; u < count; ++u) keep_host[u] = lmx_gait_keep(seed, stream, (uint64_t)u, thr) ? 1 : 0;
  return LMX_OK;
}

namespace {

// out[t][o] = b[o] + sum over taps j (first to last) and input channels c (ascending) of W[o][c][j] * in[t - (taps - 1 - j) d][c]
void conv(const float* in, int cin, float* out, int cout, const float* w, const float* b, int taps, int d, int T) {
  for (int t = 0; t < T; ++t)
    for (int o = 0; o < cout; ++o) {
      float s = b[o];
      for (int j = 0; j < taps; ++j) {
        const int ts = t - (taps - 1 - j) * d;
        if (ts < 0) continue;
        for (int c = 0; c < cin; ++c) s += w[lmx_gait_packed_index(o, c, j, cin, cout)] * in[(size_t)ts * cin + c];
      }
      out[(size_t)t * cout + o] = s;
    }
}

}  // namespace

extern "C" int lmx_h_tcn_forward(const lmx_tcn_weights_t* w, const float* x, const uint64_t* seeds, int n, int T, int S, double p, float* pred,
                                 float* stats, float* trunk) {
  if (const int rc = lmx_tcn_check_config("lmx_h_tcn_forward", w, true)) return rc;
  if (const int rc = lmx_tcn_check_call("lmx_h_tcn_forward", n, T, S, p)) return rc;
  if (n == 0) return LMX_OK;
  GAIT_REQUIRE(x && pred && stats && (seeds || S == 0), "lmx_h_tcn_forward: null pointer");
  const int F = w->input_dim, nb = w->n_blocks, Smax = S > 0 ? S : 1, C = w->channels[nb - 1], H = w->head;
  std::vector<float> cur((size_t)T * LMX_TCN_MAX_CH), h((size_t)T * LMX_TCN_MAX_CH), y((size_t)T * LMX_TCN_MAX_CH), r((size_t)T * LMX_TCN_MAX_CH);
  for (int i = 0; i < n; ++i) {
    for (int s = 0; s < Smax; ++s) {
      const LmxGaitDrop drop(S, seeds, i, p, s, 2 * nb + 1);
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
      float pooled[LMX_TCN_MAX_CH];
      for (int c = 0; c < C; ++c) {
        float sum = 0.0f;
        for (int t = 0; t < T; ++t) sum += cur[(size_t)t * C + c];
        pooled[c] = sum / (float)T;
      }
      const float z = lmx_gait_head(pooled, C, H, w->fc1_w, w->fc1_b, w->fc2_w, w->fc2_b, drop, 2 * nb);
      pred[(size_t)i * Smax + s] = 1.0f / (1.0f + expf(-z));
    }
    lmx_gait_row_stats(pred + (size_t)i * Smax, S, stats + 2 * i);
  }
  return LMX_OK;
}

extern "C" int lmx_h_tcn_features(const double* kp, const int* n_kp, const double* bbox, int T0, int target, float* out) {
  if (const int rc = lmx_gait_check_clip("lmx_h_tcn_features", T0, target, kp && n_kp && bbox && out, n_kp)) return rc;
  const int F = LMX_GAIT_FEATURES, K = LMX_GAIT_N_KEYPOINTS;
  const LmxGaitWindow win = lmx_gait_window(T0, target);
  memset(out, 0, (size_t)target * F * sizeof(float));
  auto centroid_x = [&](int t) { return (float)((bbox[4 * t] + bbox[4 * t + 2]) / 2 / 1280); };
  for (int r = 0; r < win.rows; ++r) {
    const int t = win.first + r;
    const double* b = bbox + 4 * (size_t)t;
    const double bw = b[2] - b[0], bh = b[3] - b[1], dw = bw > 1 ? bw : 1, dh = bh > 1 ? bh : 1;
    float* o = out + (size_t)(win.at + r) * F;
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
