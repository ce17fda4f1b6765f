// graph.h — what the two graph models (the graph transformer: gfm.h; GraphGPS: gnn.h) have in common on the HOST: the checks every
// forward and every handle makes of a batch of graphs, the kNN and temporal edges of the graph builders, and the plain f32 layers of
// the host forwards.  Plain C++ without HIP types, header-only like gait.h: host_gfm.cpp and host_gnn.cpp compile the arithmetic under
// their own -ffp-contract=off.  The device helpers the two kernels share are in graph_tile.h.
#pragma once
#include <algorithm>
#include <vector>

#include "gait.h"

// The checks of n, S, p, the offsets and every graph's size that lmx_gfm_check_call and lmx_gnn_check_call share (G: either graphs
// struct).  mode() checks the outputs against S, each(i, N, E) is the model's own look at graph i; both return LMX_OK or an error.
// *nodes = sum N, *max_n = max N.
template <class G, class Mode, class Each>
inline int lmx_graph_check_call(const char* who, const G* g, int S, double p, int max_nodes, Mode mode, Each each, int64_t* nodes, int* max_n) {
  GAIT_REQUIRE(g != nullptr, "%s: null graphs", who);
  GAIT_REQUIRE(g->n >= 0, "%s: n = %d graphs", who, g->n);
  GAIT_REQUIRE(S == 0 || (S >= 2 && S <= 65535), "%s: S %d (0: eval mode; 2 .. 65535 samples; the standard deviation of 1 is undefined)", who, S);
  GAIT_REQUIRE(S == 0 || (p >= 0.0 && p < 1.0), "%s: p %g outside [0, 1)", who, p);
  if (const int rc = mode()) return rc;
  *nodes = 0;
  *max_n = 0;
  if (g->n == 0) return LMX_OK;
  GAIT_REQUIRE(g->node_off_host && g->edge_off_host, "%s: null offsets", who);
  GAIT_REQUIRE(g->node_off_host[0] == 0 && g->edge_off_host[0] == 0, "%s: offsets start at node_off %d, edge_off %d, not at 0", who,
               g->node_off_host[0], g->edge_off_host[0]);
  for (int i = 0; i < g->n; ++i) {
    const int64_t N = (int64_t)g->node_off_host[i + 1] - g->node_off_host[i], E = (int64_t)g->edge_off_host[i + 1] - g->edge_off_host[i];
    GAIT_REQUIRE(N >= 1 && N <= max_nodes, "%s: graph %d has N = %lld nodes (node_off %d .. %d), outside 1 .. %d", who, i, (long long)N,
                 g->node_off_host[i], g->node_off_host[i + 1], max_nodes);
    GAIT_REQUIRE(E >= 0, "%s: edge_off descends at graph %d (%d after %d)", who, i, g->edge_off_host[i + 1], g->edge_off_host[i]);
    if (const int rc = each(i, N, E)) return rc;
    if (N > *max_n) *max_n = (int)N;
  }
  *nodes = g->node_off_host[g->n];
  return LMX_OK;
}

// The edges of one graph into edges [.][2] and edge_attr [.][3] = {weight, knn, 1 - knn}; returns their number.  First the k nearest
// neighbours of every node by cosine similarity (unit vectors and sums in double; ascending similarity, exact ties to the lower index
// first: the last k are the neighbours) with weight knn_weight(sim), then, with timestamps, both directions between neighbours in time
// with weight time_weight(|dt| in double).  The caller has brought k below N.
template <class TS, class KnnWeight, class TimeWeight>
inline int lmx_graph_edges(const float* emb, const TS* ts, int N, int E, int k, KnnWeight knn_weight, TimeWeight time_weight, int32_t* edges,
                           float* edge_attr) {
  int ne = 0;
  auto add = [&](int src, int dst, float weight, float knn) {
    edges[2 * ne] = src, edges[2 * ne + 1] = dst;
    edge_attr[3 * ne] = weight, edge_attr[3 * ne + 1] = knn, edge_attr[3 * ne + 2] = 1.0f - knn;
    ++ne;
  };
  if (k > 0 && N > 1) {
    std::vector<double> unit((size_t)N * E), sim((size_t)N);
    for (int i = 0; i < N; ++i) {
      double ss = 0.0;
      for (int c = 0; c < E; ++c) ss += (double)emb[(size_t)i * E + c] * (double)emb[(size_t)i * E + c];
      const double norm = sqrt(ss) + 1e-8;
      for (int c = 0; c < E; ++c) unit[(size_t)i * E + c] = (double)emb[(size_t)i * E + c] / norm;
    }
    std::vector<int> order((size_t)N - 1);
    for (int i = 0; i < N; ++i) {
      int m = 0;
      for (int j = 0; j < N; ++j) {
        if (j == i) continue;
        double s = 0.0;
        for (int c = 0; c < E; ++c) s += unit[(size_t)i * E + c] * unit[(size_t)j * E + c];
        sim[j] = s;
        order[m++] = j;
      }
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sim[a] < sim[b]; });
      for (int q = N - 1 - k; q < N - 1; ++q) add(i, order[q], knn_weight(sim[order[q]]), 1.0f);
    }
  }
  if (ts && N > 1) {
    std::vector<int> order((size_t)N);
    for (int i = 0; i < N; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ts[a] < ts[b]; });
    for (int q = 0; q + 1 < N; ++q) {
      const int a = order[q], b = order[q + 1];
      const float weight = time_weight(fabs((double)ts[b] - (double)ts[a]));
      add(a, b, weight, 0.0f);
      add(b, a, weight, 0.0f);
    }
  }
  return ne;
}

namespace lmx_graph {

// a packed linear layer [K -> N] as the plain matrix [N][K]: a forward reads every weight once per row, so it unpacks them once per call
inline std::vector<float> unpack(const float* w, int K, int N) {
  std::vector<float> out((size_t)N * K);
  for (int o = 0; o < N; ++o)
    for (int c = 0; c < K; ++c) out[(size_t)o * K + c] = w[lmx_gait_packed_index(o, c, 0, K, N)];
  return out;
}

// out[t][o] = b[o] + sum over c (ascending) of W[o][c] * in[t][c], W plain [N][K]
inline void linear(const float* in, int ld_in, int K, float* out, int ld_out, int N, const float* w, const float* b, int T) {
  for (int t = 0; t < T; ++t)
    for (int o = 0; o < N; ++o) {
      float s = b[o];
      const float* wr = w + (size_t)o * K;
      for (int c = 0; c < K; ++c) s += wr[c] * in[(size_t)t * ld_in + c];
      out[(size_t)t * ld_out + o] = s;
    }
}

// out[o] = b[o] + sum over c (ascending) of Wt[c][o] * in[c]
inline void linear_t(const float* in, int K, float* out, int N, const float* wt, const float* b) {
  for (int o = 0; o < N; ++o) {
    float s = b[o];
    for (int c = 0; c < K; ++c) s += wt[(size_t)c * N + o] * in[c];
    out[o] = s;
  }
}

inline void layer_norm(const float* in, int ld_in, float* out, int ld_out, const float* g, const float* b, int T, int D) {
  for (int t = 0; t < T; ++t) {
    const float* x = in + (size_t)t * ld_in;
    float sum = 0.0f, ss = 0.0f;
    for (int c = 0; c < D; ++c) sum += x[c];
    const float mean = sum / (float)D;
    for (int c = 0; c < D; ++c) ss += (x[c] - mean) * (x[c] - mean);
    const float rstd = 1.0f / sqrtf(ss / (float)D + 1e-5f);
    for (int c = 0; c < D; ++c) out[(size_t)t * ld_out + c] = (x[c] - mean) * rstd * g[c] + b[c];
  }
}

inline float gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

}  // namespace lmx_graph
