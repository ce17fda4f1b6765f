// host_xfm.cpp — the gait transformer on the HOST (include/lmx.h "The gait transformer"): the configuration check both forwards share,
// the whole forward in plain C++ (f32, sequential sums, no contraction: the Makefile builds this file with -ffp-contract=off) with the
// keep bits and the head of gait.h, and the key-padding mask of services/transformer-pipeline/app/main.py:303-392.  No HIP here: it makes the service
// testable without a GPU and is what the stand-alone sanitizer program (tests/xfm_check_main.cpp) runs.  The device forward is
// csrc/xfm.hip; both read the packed weights of xfm.h.
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "xfm.h"
#include "weights_table.h"

int lmx_xfm_check_config(const char* who, const lmx_xfm_weights_t* w, bool pointers) {
  GAIT_REQUIRE(w != nullptr, "%s: null weights", who);
  GAIT_REQUIRE(w->input_dim >= 1 && w->input_dim <= LMX_XFM_MAX_D, "%s: input_dim %d outside 1 .. %d", who, w->input_dim, LMX_XFM_MAX_D);
  GAIT_REQUIRE(w->d_model >= 16 && w->d_model <= LMX_XFM_MAX_D && w->d_model % 16 == 0, "%s: d_model %d is not 16, 32, 48 or 64", who, w->d_model);
  GAIT_REQUIRE(w->n_heads >= 1 && w->d_model % w->n_heads == 0 && (w->d_model / w->n_heads == 16 || w->d_model / w->n_heads == 32),
              "%s: n_heads %d gives d_model %d a head_dim that is neither 16 nor 32", who, w->n_heads, w->d_model);
  GAIT_REQUIRE(w->n_layers >= 1 && w->n_layers <= LMX_XFM_MAX_LAYERS, "%s: n_layers %d outside 1 .. %d", who, w->n_layers, LMX_XFM_MAX_LAYERS);
  GAIT_REQUIRE(w->ff >= 16 && w->ff <= LMX_XFM_MAX_FF && w->ff % 16 == 0, "%s: ff %d is not a multiple of 16 up to %d", who, w->ff, LMX_XFM_MAX_FF);
  GAIT_REQUIRE(w->head >= 1 && w->head <= LMX_XFM_MAX_HEAD, "%s: head %d outside 1 .. %d", who, w->head, LMX_XFM_MAX_HEAD);
  GAIT_REQUIRE(w->max_len >= 1 && w->max_len <= LMX_XFM_MAX_LEN, "%s: max_len %d outside 1 .. %d", who, w->max_len, LMX_XFM_MAX_LEN);
  if (!pointers) return LMX_OK;
  GAIT_REQUIRE(w->in_w && w->in_b && w->pe, "%s: the input projection or the positional table has no weights", who);
  GAIT_REQUIRE(((uintptr_t)w->in_w & 15) == 0, "%s: the input projection is not 16-byte aligned", who);
  for (int l = 0; l < w->n_layers; ++l) {
    GAIT_REQUIRE(w->ln1_g[l] && w->ln1_b[l] && w->qkv_w[l] && w->qkv_b[l] && w->out_w[l] && w->out_b[l] && w->ln2_g[l] && w->ln2_b[l] &&
                    w->ff1_w[l] && w->ff1_b[l] && w->ff2_w[l] && w->ff2_b[l],
                "%s: layer %d lacks a tensor", who, l);
    GAIT_REQUIRE((((uintptr_t)w->qkv_w[l] | (uintptr_t)w->out_w[l] | (uintptr_t)w->ff1_w[l] | (uintptr_t)w->ff2_w[l]) & 15) == 0,
                "%s: layer %d has weights that are not 16-byte aligned", who, l);
  }
  GAIT_REQUIRE(w->lnf_g && w->lnf_b && w->fc1_w && w->fc1_b && w->fc2_w && w->fc2_b, "%s: the final norm or the classifier has no weights", who);
  GAIT_REQUIRE(((uintptr_t)w->fc1_w & 15) == 0, "%s: the classifier's fc1 weights are not 16-byte aligned", who);
  return LMX_OK;
}

// The weight table (xfm.h): the tensors of the image and of lmx.xfm.pack_tensors in their order
void lmx_xfm_tensor_rows(const lmx_xfm_weights_t& c, std::vector<LmxTensorRow>* rows) {
#define ROW(member, index, name, field, ...) LMX_ROW(lmx_xfm_weights_t, member, index, name, field, __VA_ARGS__)
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, QD = D / 16;
  ROW(in_w, 0, "in.w", "input_dim, d_model", lmx_gait_groups(F), QD, 64, 4);
  ROW(in_b, 0, "in.b", "d_model", D);
  ROW(pe, 0, "pe", "max_len, d_model", c.max_len, D);
  for (int l = 0; l < c.n_layers; ++l) {
    const std::string b = "layer." + std::to_string(l) + ".";
    ROW(ln1_g, l, b + "ln1.g", "d_model", D);
    ROW(ln1_b, l, b + "ln1.b", "d_model", D);
    ROW(qkv_w, l, b + "qkv.w", "n_heads, d_model", H * QD, 3 * dh / 16, 64, 4);
    ROW(qkv_b, l, b + "qkv.b", "n_heads, d_model", H, 3 * dh);
    ROW(out_w, l, b + "out.w", "d_model", QD, QD, 64, 4);
    ROW(out_b, l, b + "out.b", "d_model", D);
    ROW(ln2_g, l, b + "ln2.g", "d_model", D);
    ROW(ln2_b, l, b + "ln2.b", "d_model", D);
    ROW(ff1_w, l, b + "ff1.w", "d_model, ff", QD, FF / 16, 64, 4);
    ROW(ff1_b, l, b + "ff1.b", "ff", FF);
    ROW(ff2_w, l, b + "ff2.w", "ff, d_model", FF / 16, QD, 64, 4);
    ROW(ff2_b, l, b + "ff2.b", "d_model", D);
  }
  ROW(lnf_g, 0, "lnf.g", "d_model", D);
  ROW(lnf_b, 0, "lnf.b", "d_model", D);
  ROW(fc1_w, 0, "head.fc1.w", "head, d_model", c.head, D);
  ROW(fc1_b, 0, "head.fc1.b", "head", c.head);
  ROW(fc2_w, 0, "head.fc2.w", "head", c.head);
  ROW(fc2_b, 0, "head.fc2.b", "one class", 1);
#undef ROW
}

extern "C" int lmx_h_xfm_tensors(const char* who, const lmx_xfm_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host) {
  return lmx_table_export("lmx_h_xfm_tensors", who, config_host, lmx_xfm_check_config, lmx_xfm_tensor_rows, rows_host, cap, n_host);
}

namespace {

// out[t][o] = b[o] + sum over c (ascending) of W[o][c] * in[t][c]
void linear(const float* in, int ld_in, int K, float* out, int ld_out, int N, const float* w, const float* b, int T) {
  for (int t = 0; t < T; ++t)
    for (int o = 0; o < N; ++o) {
      float s = b[o];
      for (int c = 0; c < K; ++c) s += w[lmx_xfm_packed_index(o, c, K, N)] * in[(size_t)t * ld_in + c];
      out[(size_t)t * ld_out + o] = s;
    }
}

void layer_norm(const float* in, float* out, const float* g, const float* b, int T, int D) {
  for (int t = 0; t < T; ++t) {
    const float* x = in + (size_t)t * D;
    float sum = 0.0f, ss = 0.0f;
    for (int c = 0; c < D; ++c) sum += x[c];
    const float mean = sum / (float)D;
    for (int c = 0; c < D; ++c) ss += (x[c] - mean) * (x[c] - mean);
    const float rstd = 1.0f / sqrtf(ss / (float)D + 1e-5f);
    for (int c = 0; c < D; ++c) out[(size_t)t * D + c] = (x[c] - mean) * rstd * g[c] + b[c];
  }
}

}  // namespace

extern "C" int lmx_h_xfm_forward(const lmx_xfm_weights_t* w, const float* x, const uint8_t* mask, const uint64_t* seeds, int n, int T, int S,
                                 double p, float* pred, float* stats, float* saliency, float* trunk) {
  if (const int rc = lmx_xfm_check_config("lmx_h_xfm_forward", w, true)) return rc;
  if (const int rc = lmx_xfm_check_call("lmx_h_xfm_forward", w, n, T, S, p, saliency != nullptr)) return rc;
  if (n == 0) return LMX_OK;
  GAIT_REQUIRE(x && pred && stats && (seeds || S == 0), "lmx_h_xfm_forward: null pointer");
  const int F = w->input_dim, D = w->d_model, H = w->n_heads, dh = D / H, L = w->n_layers, FF = w->ff, HD = w->head, Smax = S > 0 ? S : 1;
  const float qs = lmx_xfm_q_scale(dh), ninf = -std::numeric_limits<float>::infinity();
  const int64_t head_floats = lmx_xfm_qkv_head_floats(*w);
  std::vector<float> h((size_t)T * D), a((size_t)T * D), qkv((size_t)T * 3 * dh), o((size_t)T * D), y((size_t)T * D), hid((size_t)T * FF),
      prob((size_t)T), sal((size_t)T), sal_head((size_t)T), sal_rows((size_t)T);
  for (int i = 0; i < n; ++i) {
    const uint8_t* mk = mask ? mask + (size_t)i * T : nullptr;
    for (int s = 0; s < Smax; ++s) {
      const LmxGaitDrop drop(S, seeds, i, p, s, 4 * L + 2);
      linear(x + (size_t)i * T * F, F, F, h.data(), D, D, w->in_w, w->in_b, T);
      for (int t = 0; t < T; ++t)
        for (int c = 0; c < D; ++c) h[(size_t)t * D + c] = drop(h[(size_t)t * D + c] + w->pe[(size_t)t * D + c], 0, (uint64_t)t * D + c);
      for (int l = 0; l < L; ++l) {
        layer_norm(h.data(), a.data(), w->ln1_g[l], w->ln1_b[l], T, D);
        const bool sal_here = saliency && l == L - 1;
        if (sal_here) std::fill(sal.begin(), sal.end(), 0.0f);
        for (int hd = 0; hd < H; ++hd) {
          linear(a.data(), D, D, qkv.data(), 3 * dh, 3 * dh, w->qkv_w[l] + hd * head_floats, w->qkv_b[l] + hd * 3 * dh, T);
          for (int t = 0; t < T; ++t)
            for (int c = 0; c < dh; ++c) qkv[(size_t)t * 3 * dh + c] *= qs;
          // the saliency's column sums in three levels, 16 query rows -> the head -> all heads, as the device adds tile sums: one
          // running f32 sum over H * T terms would lose more than the rule of the tests allows
          std::fill(sal_head.begin(), sal_head.end(), 0.0f);
          std::fill(sal_rows.begin(), sal_rows.end(), 0.0f);
          for (int t = 0; t < T; ++t) {
            float mx = ninf;
            for (int u = 0; u < T; ++u) {
              float sc = ninf;
              if (!(mk && mk[u])) {
                sc = 0.0f;
                for (int c = 0; c < dh; ++c) sc += qkv[(size_t)t * 3 * dh + c] * qkv[(size_t)u * 3 * dh + dh + c];
              }
              prob[u] = sc;
              mx = fmaxf(mx, sc);
            }
            float sum = 0.0f;
            for (int u = 0; u < T; ++u) {
              prob[u] = expf(prob[u] - mx);  // all keys masked: -inf - -inf = NaN, as torch
              sum += prob[u];
            }
            for (int u = 0; u < T; ++u) {
              prob[u] = drop(prob[u] / sum, 1 + 4 * l, ((uint64_t)hd * T + t) * T + u);
              if (sal_here) sal_rows[u] += prob[u];
            }
            if (sal_here && (t % 16 == 15 || t == T - 1))
              for (int u = 0; u < T; ++u) {
                sal_head[u] += sal_rows[u];
                sal_rows[u] = 0.0f;
              }
            for (int c = 0; c < dh; ++c) {
              float acc = 0.0f;
              for (int u = 0; u < T; ++u) acc += prob[u] * qkv[(size_t)u * 3 * dh + 2 * dh + c];
              o[(size_t)t * D + hd * dh + c] = acc;
            }
          }
          if (sal_here)
            for (int u = 0; u < T; ++u) sal[u] += sal_head[u];
        }
        if (sal_here)
          for (int u = 0; u < T; ++u) saliency[(size_t)i * T + u] = sal[u] / (float)H;
        linear(o.data(), D, D, y.data(), D, D, w->out_w[l], w->out_b[l], T);
        for (int t = 0; t < T; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(y[(size_t)t * D + c], 2 + 4 * l, (uint64_t)t * D + c);
        layer_norm(h.data(), a.data(), w->ln2_g[l], w->ln2_b[l], T, D);
        linear(a.data(), D, D, hid.data(), FF, FF, w->ff1_w[l], w->ff1_b[l], T);
        for (int t = 0; t < T; ++t)
          for (int j = 0; j < FF; ++j) {
            const float v = hid[(size_t)t * FF + j];
            hid[(size_t)t * FF + j] = drop(0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)), 3 + 4 * l, (uint64_t)t * FF + j);
          }
        linear(hid.data(), FF, FF, y.data(), D, D, w->ff2_w[l], w->ff2_b[l], T);
        for (int t = 0; t < T; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(y[(size_t)t * D + c], 4 + 4 * l, (uint64_t)t * D + c);
      }
      layer_norm(h.data(), a.data(), w->lnf_g, w->lnf_b, T, D);
      if (trunk) memcpy(trunk + ((size_t)i * Smax + s) * T * D, a.data(), (size_t)T * D * sizeof(float));
      int count = 0;
      for (int t = 0; t < T; ++t) count += !(mk && mk[t]);
      float pooled[LMX_XFM_MAX_D];
      for (int c = 0; c < D; ++c) {
        float sum = 0.0f;
        for (int t = 0; t < T; ++t)
          if (!(mk && mk[t])) sum += a[(size_t)t * D + c];
        pooled[c] = sum / (float)(count > 0 ? count : 1);
      }
      const float z = lmx_gait_head(pooled, D, HD, w->fc1_w, w->fc1_b, w->fc2_w, w->fc2_b, drop, 4 * L + 1);
      // no unmasked step: every softmax of the clip is NaN and torch's pooling (NaN * 0) keeps it; fmaxf would not, so it is said here
      pred[(size_t)i * Smax + s] = count ? 1.0f / (1.0f + expf(-z)) : std::numeric_limits<float>::quiet_NaN();
    }
    lmx_gait_row_stats(pred + (size_t)i * Smax, S, stats + 2 * i);
  }
  return LMX_OK;
}

extern "C" int lmx_h_xfm_mask(const double* kp_conf, const int* n_kp, const double* det_conf, int T0, int target, uint8_t* mask) {
  if (const int rc = lmx_gait_check_clip("lmx_h_xfm_mask", T0, target, kp_conf && n_kp && det_conf && mask, n_kp)) return rc;
  const int K = LMX_GAIT_N_KEYPOINTS;
  const LmxGaitWindow win = lmx_gait_window(T0, target);
  memset(mask, 1, (size_t)target);
  for (int r = 0; r < win.rows; ++r) {
    const int t = win.first + r;
    double sum = 0.0;
    for (int i = 0; i < n_kp[t]; ++i) sum += kp_conf[(size_t)t * K + i];
    mask[win.at + r] = (float)(sum / K * det_conf[t]) < 0.3f ? 1 : 0;
  }
  return LMX_OK;
}
