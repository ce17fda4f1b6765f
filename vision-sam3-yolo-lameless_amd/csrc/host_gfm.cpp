// host_gfm.cpp — the graph transformer on the HOST (include/lmx.h "The graph transformer"): the graph builder lmx_h_gfm_graph (kNN and
// temporal edges, degrees, shortest-path indices, the winning edge per pair), the configuration and call checks both forwards share,
// and the whole forward in plain C++ (f32, sequential sums, no contraction: the Makefile builds this file with -ffp-contract=off) with
// the keep bits of gait.h.  No HIP here: it makes the service testable without a GPU.  The device forward is csrc/gfm.hip; both read
// the weights of gfm.h.  What this file shares with host_gnn.cpp (the batch checks, the kNN and temporal edges, the plain layers) is
// in graph.h.
#include <string.h>

#include <algorithm>
#include <limits>
#include <type_traits>
#include <vector>

#include "gfm.h"
#include "graph.h"
#include "weights_table.h"

using namespace lmx_graph;

int lmx_gfm_check_config(const char* who, const lmx_gfm_weights_t* w, bool pointers) {
  GAIT_REQUIRE(w != nullptr, "%s: null weights", who);
  GAIT_REQUIRE(w->input_dim >= 1 && w->input_dim <= LMX_GFM_MAX_IN, "%s: input_dim %d outside 1 .. %d", who, w->input_dim, LMX_GFM_MAX_IN);
  GAIT_REQUIRE(w->d_model >= 16 && w->d_model <= LMX_GFM_MAX_D && w->d_model % 16 == 0, "%s: d_model %d is not a multiple of 16 up to %d", who,
               w->d_model, LMX_GFM_MAX_D);
  GAIT_REQUIRE(w->n_heads >= 1 && w->d_model % w->n_heads == 0 && (w->d_model / w->n_heads == 16 || w->d_model / w->n_heads == 32),
               "%s: n_heads %d gives d_model %d a head_dim that is neither 16 nor 32", who, w->n_heads, w->d_model);
  GAIT_REQUIRE(w->n_layers >= 1 && w->n_layers <= LMX_GFM_MAX_LAYERS, "%s: n_layers %d outside 1 .. %d", who, w->n_layers, LMX_GFM_MAX_LAYERS);
  GAIT_REQUIRE(w->ff >= 16 && w->ff <= LMX_GFM_MAX_FF && w->ff % 16 == 0, "%s: ff %d is not a multiple of 16 up to %d", who, w->ff, LMX_GFM_MAX_FF);
  GAIT_REQUIRE(w->edge_dim == 3, "%s: edge_dim %d is not 3", who, w->edge_dim);
  GAIT_REQUIRE(w->max_degree >= 0 && w->max_degree <= LMX_GFM_MAX_DEGREE, "%s: max_degree %d outside 0 .. %d", who, w->max_degree, LMX_GFM_MAX_DEGREE);
  GAIT_REQUIRE(w->max_spd >= 0 && w->max_spd + 2 <= LMX_GFM_MAX_IDX, "%s: max_spd %d: max_spd + 2 outside 2 .. %d", who, w->max_spd, LMX_GFM_MAX_IDX);
  if (!pointers) return LMX_OK;
  GAIT_REQUIRE(w->in_w && w->in_b && w->in_g && w->in_beta && w->deg_in && w->deg_out && w->time_w && w->time_b && w->div_term && w->spd &&
                   w->e1_w && w->e1_b && w->e2_w && w->e2_b,
               "%s: the input projection or an encoding has no weights", who);
  GAIT_REQUIRE((((uintptr_t)w->in_w | (uintptr_t)w->time_w) & 15) == 0, "%s: the input or the time projection is not 16-byte aligned", who);
  for (int l = 0; l < w->n_layers; ++l) {
    GAIT_REQUIRE(w->ln1_g[l] && w->ln1_b[l] && w->qkv_w[l] && w->qkv_b[l] && w->out_w[l] && w->out_b[l] && w->ln2_g[l] && w->ln2_b[l] &&
                     w->ff1_w[l] && w->ff1_b[l] && w->ff2_w[l] && w->ff2_b[l] && w->vn[l] && w->vqkv_w[l] && w->vqkv_b[l] && w->vout_w[l] &&
                     w->vout_b[l],
                 "%s: layer %d lacks a tensor", who, l);
    GAIT_REQUIRE((((uintptr_t)w->qkv_w[l] | (uintptr_t)w->out_w[l] | (uintptr_t)w->ff1_w[l] | (uintptr_t)w->ff2_w[l] | (uintptr_t)w->vqkv_w[l] |
                   (uintptr_t)w->vout_w[l]) & 15) == 0,
                 "%s: layer %d has weights that are not 16-byte aligned", who, l);
  }
  GAIT_REQUIRE(w->vu1_w && w->vu1_b && w->vu2_w && w->vu2_b && w->vu_g && w->vu_beta && w->lnf_g && w->lnf_b && w->pool1_w && w->pool1_b &&
                   w->pool2_w && w->pool2_b && w->comb_w && w->comb_b && w->comb_g && w->comb_beta && w->ph1_w && w->ph1_b && w->ph2_w &&
                   w->ph2_b && w->ph3_w && w->ph3_b && w->nh1_w && w->nh1_b && w->nh2_w && w->nh2_b,
               "%s: the virtual node's update, the final norm, the readout or a head has no weights", who);
  GAIT_REQUIRE((((uintptr_t)w->pool1_w | (uintptr_t)w->nh1_w) & 15) == 0, "%s: the attention pool or the node head is not 16-byte aligned", who);
  return LMX_OK;
}

// The weight table (gfm.h): the tensors of the image and of lmx.gfm.pack_tensors, each named as the field of lmx_gfm_weights_t it
// fills, the per-layer ones as layer.{l}.<field>
void lmx_gfm_tensor_rows(const lmx_gfm_weights_t& c, std::vector<LmxTensorRow>* rows) {
// a tensor is named as the field it fills: ONE for a plain pointer, PER_LAYER (inside the loop over l) for an array of one pointer per layer
#define ONE(member, field, ...)                                                                        \
  static_assert(!std::is_array<decltype(lmx_gfm_weights_t::member)>::value, #member " is one pointer"); \
  LMX_ROW(lmx_gfm_weights_t, member, 0, #member, field, __VA_ARGS__)
#define PER_LAYER(member, field, ...)                                                                     \
  static_assert(std::is_array<decltype(lmx_gfm_weights_t::member)>::value, #member " is one pointer per layer"); \
  LMX_ROW(lmx_gfm_weights_t, member, l, layer + #member, field, __VA_ARGS__)
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, Q = D / 16, PD = lmx_gfm_pool_dim(D), NI = c.max_spd + 2,
            ND = c.max_degree + 1;
  ONE(in_w, "input_dim, d_model", lmx_gait_groups(F), Q, 64, 4); ONE(in_b, "d_model", D); ONE(in_g, "d_model", D); ONE(in_beta, "d_model", D);
  ONE(deg_in, "max_degree, d_model", ND, D); ONE(deg_out, "max_degree, d_model", ND, D); ONE(time_w, "d_model", Q, Q, 64, 4);
  ONE(time_b, "d_model", D); ONE(div_term, "d_model", D / 2); ONE(spd, "max_spd, n_heads", NI, H); ONE(e1_w, "n_heads, edge_dim", 2 * H, 3);
  ONE(e1_b, "n_heads", 2 * H); ONE(e2_w, "n_heads", H, 2 * H); ONE(e2_b, "n_heads", H);
  for (int l = 0; l < c.n_layers; ++l) {
    const std::string layer = "layer." + std::to_string(l) + ".";
    PER_LAYER(ln1_g, "d_model", D); PER_LAYER(ln1_b, "d_model", D); PER_LAYER(qkv_w, "n_heads, d_model", H * Q, 3 * dh / 16, 64, 4);
    PER_LAYER(qkv_b, "n_heads, d_model", H, 3 * dh); PER_LAYER(out_w, "d_model", Q, Q, 64, 4); PER_LAYER(out_b, "d_model", D); PER_LAYER(ln2_g, "d_model", D);
    PER_LAYER(ln2_b, "d_model", D); PER_LAYER(ff1_w, "d_model, ff", Q, FF / 16, 64, 4); PER_LAYER(ff1_b, "ff", FF); PER_LAYER(ff2_w, "ff, d_model", FF / 16, Q, 64, 4);
    PER_LAYER(ff2_b, "d_model", D); PER_LAYER(vn, "d_model", D); PER_LAYER(vqkv_w, "n_heads, d_model", H * Q, 3 * dh / 16, 64, 4);
    PER_LAYER(vqkv_b, "n_heads, d_model", H, 3 * dh); PER_LAYER(vout_w, "d_model", Q, Q, 64, 4); PER_LAYER(vout_b, "d_model", D);
  }
  ONE(vu1_w, "d_model", D, 2 * D); ONE(vu1_b, "d_model", 2 * D); ONE(vu2_w, "d_model", 2 * D, D); ONE(vu2_b, "d_model", D); ONE(vu_g, "d_model", D);
  ONE(vu_beta, "d_model", D); ONE(lnf_g, "d_model", D); ONE(lnf_b, "d_model", D); ONE(pool1_w, "d_model", Q, PD / 16, 64, 4);
  ONE(pool1_b, "d_model", PD); ONE(pool2_w, "d_model", PD); ONE(pool2_b, "one score", 1); ONE(comb_w, "d_model", 3 * D, D);
  ONE(comb_b, "d_model", D); ONE(comb_g, "d_model", D); ONE(comb_beta, "d_model", D); ONE(ph1_w, "d_model", D, D / 2); ONE(ph1_b, "d_model", D / 2);
  ONE(ph2_w, "d_model", D / 2, D / 4); ONE(ph2_b, "d_model", D / 4); ONE(ph3_w, "d_model", D / 4); ONE(ph3_b, "one class", 1);
  ONE(nh1_w, "d_model", Q, PD / 16, 64, 4); ONE(nh1_b, "d_model", PD); ONE(nh2_w, "d_model", PD); ONE(nh2_b, "one score", 1);
#undef ONE
#undef PER_LAYER
}

extern "C" int lmx_h_gfm_tensors(const char* who, const lmx_gfm_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host) {
  return lmx_table_export("lmx_h_gfm_tensors", who, config_host, lmx_gfm_check_config, lmx_gfm_tensor_rows, rows_host, cap, n_host);
}

int lmx_gfm_check_call(const char* who, const lmx_gfm_graphs_t* g, int S, double p, bool eval_outputs, int64_t* nodes, int64_t* cells, int* max_n) {
  *cells = 0;
  return lmx_graph_check_call(
      who, g, S, p, LMX_GFM_MAX_NODES,
      [&] {
        GAIT_REQUIRE(!eval_outputs || S == 0, "%s: node_pred and attn_to_target are read in eval mode only, S = %d", who, S);
        return LMX_OK;
      },
      [&](int, int64_t N, int64_t) {
        *cells += N * N;
        return LMX_OK;
      },
      nodes, max_n);
}

extern "C" int lmx_h_gfm_graph(const float* emb, const float* ts, int N, int E, int k, int max_degree, int max_spd, int32_t* edges, float* edge_attr,
                               int32_t* n_edges, uint8_t* deg_in, uint8_t* deg_out, uint8_t* idx, int32_t* win) {
  const char* who = "lmx_h_gfm_graph";
  GAIT_REQUIRE(N >= 1 && N <= LMX_GFM_MAX_NODES, "%s: N %d outside 1 .. %d", who, N, LMX_GFM_MAX_NODES);
  GAIT_REQUIRE(E >= 1 && E <= (1 << 20), "%s: E = %d embedding channels", who, E);
  GAIT_REQUIRE(k >= 0, "%s: k = %d neighbours", who, k);
  GAIT_REQUIRE(max_degree >= 0 && max_degree <= LMX_GFM_MAX_DEGREE, "%s: max_degree %d outside 0 .. %d", who, max_degree, LMX_GFM_MAX_DEGREE);
  GAIT_REQUIRE(max_spd >= 0 && max_spd + 2 <= LMX_GFM_MAX_IDX, "%s: max_spd %d: max_spd + 2 outside 2 .. %d", who, max_spd, LMX_GFM_MAX_IDX);
  k = std::min(k, N - 1);
  const bool no_edges = N * k + (ts ? 2 * (N - 1) : 0) == 0;  // then the two edge arrays may be absent
  GAIT_REQUIRE(emb && ((edges && edge_attr) || no_edges) && n_edges && deg_in && deg_out && idx && win, "%s: null pointer", who);
  // kNN edges weigh max(0, sim), temporal ones exp(-|dt| / a day)
  const int ne = lmx_graph_edges(
      emb, ts, N, E, k, [](double sim) { return (float)std::max(0.0, sim); }, [](double dt) { return (float)exp(-dt / 86400.0); }, edges, edge_attr);
  *n_edges = ne;
  std::vector<int> din((size_t)N, 0), dout((size_t)N, 0);
  std::vector<uint8_t> adj((size_t)N * N, 0);
  for (int i = 0; i < N * N; ++i) win[i] = -1;
  for (int e = 0; e < ne; ++e) {
    const int s = edges[2 * e], d = edges[2 * e + 1];
    ++dout[s], ++din[d];
    win[(size_t)s * N + d] = e;  // the later edge wins
    adj[(size_t)s * N + d] = adj[(size_t)d * N + s] = 1;
  }
  for (int i = 0; i < N; ++i) {
    deg_in[i] = (uint8_t)std::min(din[i], max_degree);
    deg_out[i] = (uint8_t)std::min(dout[i], max_degree);
  }
  std::vector<int> dist((size_t)N), queue((size_t)N);
  for (int i = 0; i < N; ++i) {
    std::fill(dist.begin(), dist.end(), -1);
    int head = 0, tail = 0;
    dist[i] = 0;
    queue[tail++] = i;
    while (head < tail) {
      const int u = queue[head++];
      for (int v = 0; v < N; ++v)
        if (adj[(size_t)u * N + v] && dist[v] < 0) {
          dist[v] = dist[u] + 1;
          queue[tail++] = v;
        }
    }
    for (int j = 0; j < N; ++j) idx[(size_t)i * N + j] = (uint8_t)((dist[j] < 0 || dist[j] > max_spd ? max_spd : dist[j]) + 1);
  }
  return LMX_OK;
}

namespace {

// One attention (qkv_w: the heads' plain [3 dh][D] matrices one after the other, out_w plain [D][D]) over R rows of `in` (R = N: the graph attention, rows are nodes; R = N + 1: the virtual-node attention, row 0 is the
// virtual node and the bias has a zero row and column in front).  y = concat_i(drop_site(softmax(s))_i v_i) Wo^T + bo, no dropout on y.
// colsum (NULL or [N]): += P_head[i][target] per head, graph attention only.
void attention(const lmx_gfm_weights_t& w, const float* in, int R, int N, const float* bias, const float* qkv_w, const float* qkv_b,
               const float* out_w, const float* out_b, const LmxGaitDrop& drop, int site, float* y, float* column, int target,
               std::vector<float>& qkv, std::vector<float>& o, std::vector<float>& prob) {
  const int D = w.d_model, H = w.n_heads, dh = D / H, off = R - N;
  const float c = lmx_gfm_score_scale(dh), ninf = -std::numeric_limits<float>::infinity();
  for (int hd = 0; hd < H; ++hd) {
    linear(in, D, D, qkv.data(), 3 * dh, 3 * dh, qkv_w + (size_t)hd * 3 * dh * D, qkv_b + hd * 3 * dh, R);
    for (int t = 0; t < R; ++t) {
      float mx = ninf;
      for (int u = 0; u < R; ++u) {
        float sc = 0.0f;
        for (int ch = 0; ch < dh; ++ch) sc += qkv[(size_t)t * 3 * dh + ch] * qkv[(size_t)u * 3 * dh + dh + ch];
        const float b = (t >= off && u >= off) ? bias[((size_t)hd * N + (t - off)) * N + (u - off)] : 0.0f;
        prob[u] = sc * c + b;
        mx = fmaxf(mx, prob[u]);
      }
      float sum = 0.0f;
      for (int u = 0; u < R; ++u) {
        prob[u] = expf(prob[u] - mx);
        sum += prob[u];
      }
      for (int u = 0; u < R; ++u) prob[u] = drop(prob[u] / sum, site, ((uint64_t)hd * R + t) * R + u);
      if (column) column[t] += prob[target];
      for (int ch = 0; ch < dh; ++ch) {
        float acc = 0.0f;
        for (int u = 0; u < R; ++u) acc += prob[u] * qkv[(size_t)u * 3 * dh + 2 * dh + ch];
        o[(size_t)t * D + hd * dh + ch] = acc;
      }
    }
  }
  linear(o.data(), D, D, y, D, D, out_w, out_b, R);
}

}  // namespace

extern "C" int lmx_h_gfm_forward(const lmx_gfm_weights_t* w, const lmx_gfm_graphs_t* g, const uint64_t* seeds, int S, double p, float* pred,
                                 float* stats, float* node_pred, float* attn, float* trunk, float* vn_out) {
  const char* who = "lmx_h_gfm_forward";
  if (const int rc = lmx_gfm_check_config(who, w, true)) return rc;
  int64_t nodes = 0, cells = 0;
  int max_n = 0;
  if (const int rc = lmx_gfm_check_call(who, g, S, p, node_pred != nullptr || attn != nullptr, &nodes, &cells, &max_n)) return rc;
  if (g->n == 0) return LMX_OK;
  GAIT_REQUIRE(g->x && g->deg_in && g->deg_out && g->idx && g->win && (g->edge_attr || g->edge_off_host[g->n] == 0) && pred && stats &&
                   (seeds || S == 0),
               "%s: null pointer", who);
  GAIT_REQUIRE(!g->has_time || g->timestamps, "%s: has_time without timestamps", who);
  GAIT_REQUIRE(!attn || g->target, "%s: attn_to_target without target", who);
  const int F = w->input_dim, D = w->d_model, H = w->n_heads, L = w->n_layers, FF = w->ff, Smax = S > 0 ? S : 1, PD = lmx_gfm_pool_dim(D);
  const int NI = w->max_spd + 2;
  const size_t R1 = (size_t)max_n + 1;
  std::vector<float> h(R1 * D), a(R1 * D), y(R1 * D), o(R1 * D), hid(R1 * FF), qkv(R1 * 96), prob(R1), bias((size_t)H * max_n * max_n), pe((size_t)D),
      enc((size_t)max_n * D), column((size_t)max_n), tmp(R1 * D);
  const int dh = D / H;
  const int64_t head_floats = lmx_gfm_qkv_head_floats(*w);
  auto heads = [&](const float* packed) {
    std::vector<float> out;
    for (int hd = 0; hd < H; ++hd) {
      const std::vector<float> one = unpack(packed + hd * head_floats, D, 3 * dh);
      out.insert(out.end(), one.begin(), one.end());
    }
    return out;
  };
  const std::vector<float> in_w = unpack(w->in_w, F, D), time_w = unpack(w->time_w, D, D), pool1_w = unpack(w->pool1_w, D, PD),
                           nh1_w = unpack(w->nh1_w, D, PD);
  std::vector<std::vector<float>> qkv_w, out_w, ff1_w, ff2_w, vqkv_w, vout_w;
  for (int l = 0; l < L; ++l) {
    qkv_w.push_back(heads(w->qkv_w[l])), out_w.push_back(unpack(w->out_w[l], D, D)), ff1_w.push_back(unpack(w->ff1_w[l], D, FF));
    ff2_w.push_back(unpack(w->ff2_w[l], FF, D)), vqkv_w.push_back(heads(w->vqkv_w[l])), vout_w.push_back(unpack(w->vout_w[l], D, D));
  }
  int64_t moff = 0;
  for (int i = 0; i < g->n; ++i) {
    const int n0 = g->node_off_host[i], N = g->node_off_host[i + 1] - n0, e0 = g->edge_off_host[i], NE = g->edge_off_host[i + 1] - e0;
    // the attention bias and the node encoding: once per graph
    for (int t = 0; t < N; ++t)
      for (int u = 0; u < N; ++u) {
        const int id = std::min<int>(g->idx[moff + (int64_t)t * N + u], NI - 1), e = g->win[moff + (int64_t)t * N + u];
        float eh[16], eo[8];
        const bool edge = e >= 0 && e < NE;
        if (edge) {
          const float* at = g->edge_attr + (size_t)(e0 + e) * 3;
          for (int j = 0; j < 2 * H; ++j) {
            float s = w->e1_b[j];
            for (int c = 0; c < 3; ++c) s += w->e1_w[j * 3 + c] * at[c];
            eh[j] = fmaxf(s, 0.0f);
          }
          for (int hd = 0; hd < H; ++hd) {
            float s = w->e2_b[hd];
            for (int j = 0; j < 2 * H; ++j) s += w->e2_w[hd * 2 * H + j] * eh[j];
            eo[hd] = s;
          }
        }
        for (int hd = 0; hd < H; ++hd) bias[((size_t)hd * N + t) * N + u] = w->spd[id * H + hd] + (edge ? eo[hd] : 0.0f);
      }
    const bool timed = g->has_time && g->has_time[i];
    float tmin = 0.0f;
    if (timed) {
      tmin = g->timestamps[n0];
      for (int t = 1; t < N; ++t) tmin = fminf(tmin, g->timestamps[n0 + t]);
    }
    for (int t = 0; t < N; ++t) {
      const int di = std::min<int>(g->deg_in[n0 + t], w->max_degree), dq = std::min<int>(g->deg_out[n0 + t], w->max_degree);
      for (int c = 0; c < D; ++c) enc[(size_t)t * D + c] = w->deg_in[(size_t)di * D + c] + w->deg_out[(size_t)dq * D + c];
      if (timed) {
        const float days = fminf((g->timestamps[n0 + t] - tmin) / 86400.0f, 365.0f);
        for (int c = 0; c < D; ++c) pe[c] = (c & 1) ? cosf(days * w->div_term[c >> 1]) : sinf(days * w->div_term[c >> 1]);
        linear(pe.data(), D, D, tmp.data(), D, D, time_w.data(), w->time_b, 1);
        for (int c = 0; c < D; ++c) enc[(size_t)t * D + c] += tmp[c];
      }
    }
    for (int s = 0; s < Smax; ++s) {
      const LmxGaitDrop drop(S, seeds, i, p, s, lmx_gfm_n_sites(L));
      linear(g->x + (size_t)n0 * F, F, F, y.data(), D, D, in_w.data(), w->in_b, N);
      layer_norm(y.data(), D, h.data(), D, w->in_g, w->in_beta, N, D);
      for (int t = 0; t < N; ++t)
        for (int c = 0; c < D; ++c) h[(size_t)t * D + c] = drop(h[(size_t)t * D + c], 0, (uint64_t)t * D + c) + enc[(size_t)t * D + c];
      float vnv[LMX_GFM_MAX_D];
      for (int l = 0; l < L; ++l) {
        layer_norm(h.data(), D, a.data(), D, w->ln1_g[l], w->ln1_b[l], N, D);
        const bool col = attn && l == L - 1;
        if (col) std::fill(column.begin(), column.end(), 0.0f);
        attention(*w, a.data(), N, N, bias.data(), qkv_w[l].data(), w->qkv_b[l], out_w[l].data(), w->out_b[l], drop, 1 + 6 * l, y.data(),
                  col ? column.data() : nullptr, col ? std::min(std::max(g->target[i], 0), N - 1) : 0, qkv, o, prob);
        if (col)
          for (int t = 0; t < N; ++t) attn[n0 + t] = (g->target[i] >= 0 && g->target[i] < N) ? column[t] / (float)H : 0.0f;
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(y[(size_t)t * D + c], 2 + 6 * l, (uint64_t)t * D + c);
        layer_norm(h.data(), D, a.data(), D, w->ln2_g[l], w->ln2_b[l], N, D);
        linear(a.data(), D, D, hid.data(), FF, FF, ff1_w[l].data(), w->ff1_b[l], N);
        for (int t = 0; t < N; ++t)
          for (int j = 0; j < FF; ++j) hid[(size_t)t * FF + j] = drop(gelu(hid[(size_t)t * FF + j]), 3 + 6 * l, (uint64_t)t * FF + j);
        linear(hid.data(), FF, FF, y.data(), D, D, ff2_w[l].data(), w->ff2_b[l], N);
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(y[(size_t)t * D + c], 4 + 6 * l, (uint64_t)t * D + c);
        // the virtual-node attention over [vn_l ; h]: no norm in front, no residual
        memcpy(tmp.data(), w->vn[l], (size_t)D * sizeof(float));
        memcpy(tmp.data() + D, h.data(), (size_t)N * D * sizeof(float));
        attention(*w, tmp.data(), N + 1, N, bias.data(), vqkv_w[l].data(), w->vqkv_b[l], vout_w[l].data(), w->vout_b[l], drop, 5 + 6 * l, y.data(), nullptr,
                  0, qkv, o, prob);
        for (int t = 0; t <= N; ++t)
          for (int c = 0; c < D; ++c) y[(size_t)t * D + c] = drop(y[(size_t)t * D + c], 6 + 6 * l, (uint64_t)t * D + c);
        memcpy(h.data(), y.data() + D, (size_t)N * D * sizeof(float));
        if (l == L - 1) {
          float u1[2 * LMX_GFM_MAX_D], u2[LMX_GFM_MAX_D];
          linear_t(y.data(), D, u1, 2 * D, w->vu1_w, w->vu1_b);
          for (int j = 0; j < 2 * D; ++j) u1[j] = gelu(u1[j]);
          linear_t(u1, 2 * D, u2, D, w->vu2_w, w->vu2_b);
          layer_norm(u2, D, vnv, D, w->vu_g, w->vu_beta, 1, D);
        }
      }
      layer_norm(h.data(), D, a.data(), D, w->lnf_g, w->lnf_b, N, D);
      if (trunk) memcpy(trunk + ((size_t)n0 * Smax + (size_t)s * N) * D, a.data(), (size_t)N * D * sizeof(float));
      if (vn_out) memcpy(vn_out + ((size_t)i * Smax + s) * D, vnv, (size_t)D * sizeof(float));
      // the readout: mean | vn | attention pool
      float comb[3 * LMX_GFM_MAX_D], r[LMX_GFM_MAX_D], rn[LMX_GFM_MAX_D], score[LMX_GFM_MAX_NODES], ph[LMX_GFM_MAX_D / 2 + 16], h1[LMX_GFM_MAX_D / 2],
          h2[LMX_GFM_MAX_D / 4];
      float mx = -std::numeric_limits<float>::infinity(), esum = 0.0f;
      for (int t = 0; t < N; ++t) {
        linear(a.data() + (size_t)t * D, D, D, ph, PD, PD, pool1_w.data(), w->pool1_b, 1);
        float sc = w->pool2_b[0];
        for (int j = 0; j < PD; ++j) sc += w->pool2_w[j] * tanhf(ph[j]);
        score[t] = sc;
        mx = fmaxf(mx, sc);
      }
      for (int t = 0; t < N; ++t) {
        score[t] = expf(score[t] - mx);
        esum += score[t];
      }
      for (int c = 0; c < D; ++c) {
        float sum = 0.0f, pool = 0.0f;
        for (int t = 0; t < N; ++t) sum += a[(size_t)t * D + c];
        for (int t = 0; t < N; ++t) pool += score[t] / esum * a[(size_t)t * D + c];
        comb[c] = sum / (float)N;
        comb[D + c] = vnv[c];
        comb[2 * D + c] = pool;
      }
      linear_t(comb, 3 * D, r, D, w->comb_w, w->comb_b);
      for (int c = 0; c < D; ++c) r[c] = fmaxf(r[c], 0.0f);
      layer_norm(r, D, rn, D, w->comb_g, w->comb_beta, 1, D);
      linear_t(rn, D, h1, D / 2, w->ph1_w, w->ph1_b);
      for (int j = 0; j < D / 2; ++j) h1[j] = drop(fmaxf(h1[j], 0.0f), 6 * L + 1, (uint64_t)j);
      linear_t(h1, D / 2, h2, D / 4, w->ph2_w, w->ph2_b);
      for (int j = 0; j < D / 4; ++j) h2[j] = drop(fmaxf(h2[j], 0.0f), 6 * L + 2, (uint64_t)j);
      float z = w->ph3_b[0];
      for (int j = 0; j < D / 4; ++j) z += w->ph3_w[j] * h2[j];
      pred[(size_t)i * Smax + s] = 1.0f / (1.0f + expf(-z));
      if (node_pred)
        for (int t = 0; t < N; ++t) {
          linear(a.data() + (size_t)t * D, D, D, ph, PD, PD, nh1_w.data(), w->nh1_b, 1);
          float zn = w->nh2_b[0];
          for (int j = 0; j < PD; ++j) zn += w->nh2_w[j] * fmaxf(ph[j], 0.0f);
          node_pred[n0 + t] = 1.0f / (1.0f + expf(-zn));
        }
    }
    lmx_gait_row_stats(pred + (size_t)i * Smax, S, stats + 2 * i);
    moff += (int64_t)N * N;
  }
  return LMX_OK;
}
