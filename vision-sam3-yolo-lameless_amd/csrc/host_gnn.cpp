// host_gnn.cpp — GraphGPS on the HOST (include/lmx.h "GraphGPS"): the graph builder lmx_h_gnn_graph (kNN and temporal edges, the CSR by
// destination, the raw Laplacian and random-walk encodings in double), the configuration and call checks both forwards share, and the
// whole live network in plain C++ (f32, sequential sums, no contraction: the Makefile builds this file with -ffp-contract=off) with the
// keep bits of gait.h.  No HIP here: it makes the service testable without a GPU.  The device forward is csrc/gnn.hip.  What
// this file shares with host_gfm.cpp (the batch checks, the kNN and temporal edges, the plain layers) is in graph.h.
#include <string.h>

#include <algorithm>
#include <limits>
#include <type_traits>
#include <vector>

#include "gnn.h"
#include "graph.h"
#include "weights_table.h"

using namespace lmx_graph;

int lmx_gnn_check_config(const char* who, const lmx_gnn_weights_t* w, bool pointers) {
  GAIT_REQUIRE(w != nullptr, "%s: null weights", who);
  GAIT_REQUIRE(w->input_dim >= 1 && w->input_dim <= LMX_GNN_MAX_IN, "%s: input_dim %d outside 1 .. %d", who, w->input_dim, LMX_GNN_MAX_IN);
  GAIT_REQUIRE(w->d_model >= 32 && w->d_model <= LMX_GNN_MAX_D && w->d_model % 32 == 0, "%s: d_model %d is not a multiple of 32 up to %d", who,
               w->d_model, LMX_GNN_MAX_D);
  GAIT_REQUIRE(w->n_heads >= 1 && w->d_model % w->n_heads == 0 && (w->d_model / w->n_heads == 16 || w->d_model / w->n_heads == 32),
               "%s: n_heads %d gives d_model %d a head_dim that is neither 16 nor 32", who, w->n_heads, w->d_model);
  GAIT_REQUIRE(w->n_layers >= 1 && w->n_layers <= LMX_GNN_MAX_LAYERS, "%s: n_layers %d outside 1 .. %d live layers", who, w->n_layers,
               LMX_GNN_MAX_LAYERS);
  GAIT_REQUIRE(w->pe_dim >= 8 && w->pe_dim % 8 == 0 && 2 * w->pe_dim < w->d_model, "%s: pe_dim %d is not a multiple of 8 with 2 pe_dim < d_model %d",
               who, w->pe_dim, w->d_model);
  GAIT_REQUIRE(w->ff >= 16 && w->ff <= LMX_GNN_MAX_FF && w->ff % 16 == 0, "%s: ff %d is not a multiple of 16 up to %d", who, w->ff, LMX_GNN_MAX_FF);
  GAIT_REQUIRE(w->edge_dim == 3, "%s: edge_dim %d is not 3", who, w->edge_dim);
  if (!pointers) return LMX_OK;
  GAIT_REQUIRE(w->in_w && w->in_b && w->lap1_w && w->lap1_b && w->lap2_w && w->lap2_b && w->lap_g && w->lap_beta && w->rw1_w && w->rw1_b && w->rw2_w &&
                   w->rw2_b && w->rw_g && w->rw_beta && w->ee1_w && w->ee1_b && w->ee2_w && w->ee2_b && w->ee_g && w->ee_beta,
               "%s: the input projection, an encoding or the edge encoder has no weights", who);
  GAIT_REQUIRE((((uintptr_t)w->in_w | (uintptr_t)w->ee2_w) & 15) == 0, "%s: the input projection or the edge encoder is not 16-byte aligned", who);
  for (int l = 0; l < w->n_layers; ++l) {
    GAIT_REQUIRE(w->ln1_g[l] && w->ln1_b[l] && w->abde_w[l] && w->abde_b[l] && w->c_w[l] && w->c_b[l] && w->bnn_g[l] && w->bnn_b[l] && w->bnn_mean[l] &&
                     w->bnn_var[l] && w->ln2_g[l] && w->ln2_b[l] && w->qkv_w[l] && w->qkv_b[l] && w->out_w[l] && w->out_b[l] && w->lna_g[l] &&
                     w->lna_b[l] && w->ln3_g[l] && w->ln3_b[l] && w->ff1_w[l] && w->ff1_b[l] && w->ff2_w[l] && w->ff2_b[l],
                 "%s: layer %d lacks a tensor", who, l);
    GAIT_REQUIRE(l == w->n_layers - 1 || (w->eu1_w[l] && w->eu1_b[l] && w->eu2_w[l] && w->eu2_b[l] && w->bne_g[l] && w->bne_b[l] && w->bne_mean[l] &&
                                          w->bne_var[l]),
                 "%s: layer %d lacks its edge update", who, l);
    GAIT_REQUIRE((((uintptr_t)w->abde_w[l] | (uintptr_t)w->c_w[l] | (uintptr_t)w->eu1_w[l] | (uintptr_t)w->eu2_w[l] | (uintptr_t)w->qkv_w[l] |
                   (uintptr_t)w->out_w[l] | (uintptr_t)w->ff1_w[l] | (uintptr_t)w->ff2_w[l]) & 15) == 0,
                 "%s: layer %d has weights that are not 16-byte aligned", who, l);
  }
  GAIT_REQUIRE(w->lnf_g && w->lnf_b && w->nh1_w && w->nh1_b && w->nh2_w && w->nh2_b && w->na1_w && w->na1_b && w->na2_w && w->na2_b && w->cl1_w &&
                   w->cl1_b && w->cl2_w && w->cl2_b && w->cl3_w && w->cl3_b,
               "%s: the final norm or a head has no weights", who);
  GAIT_REQUIRE((((uintptr_t)w->nh1_w | (uintptr_t)w->na1_w) & 15) == 0, "%s: the node head or the attention pool is not 16-byte aligned", who);
  return LMX_OK;
}

// The weight table (gnn.h): the tensors of the image and of lmx.gnn.pack_tensors, each named as the field of lmx_gnn_weights_t it
// fills, the per-layer ones as layer.{l}.<field>.  The last live layer's edge update reaches no output and has no tensors.
void lmx_gnn_tensor_rows(const lmx_gnn_weights_t& c, std::vector<LmxTensorRow>* rows) {
// a tensor is named as the field it fills: ONE for a plain pointer, PER_LAYER (inside the loop over l) for an array of one pointer per layer
#define ONE(member, field, ...)                                                                        \
  static_assert(!std::is_array<decltype(lmx_gnn_weights_t::member)>::value, #member " is one pointer"); \
  LMX_ROW(lmx_gnn_weights_t, member, 0, #member, field, __VA_ARGS__)
#define PER_LAYER(member, field, ...)                                                                     \
  static_assert(std::is_array<decltype(lmx_gnn_weights_t::member)>::value, #member " is one pointer per layer"); \
  LMX_ROW(lmx_gnn_weights_t, member, l, layer + #member, field, __VA_ARGS__)
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, Q = D / 16, P = c.pe_dim, D2 = D / 2;
  ONE(in_w, "input_dim, d_model, pe_dim", lmx_gait_groups(F), (D - 2 * P) / 16, 64, 4); ONE(in_b, "d_model, pe_dim", D - 2 * P);
  ONE(lap1_w, "pe_dim", 2 * P, LMX_GNN_LAP_K); ONE(lap1_b, "pe_dim", 2 * P); ONE(lap2_w, "pe_dim", P, 2 * P); ONE(lap2_b, "pe_dim", P);
  ONE(lap_g, "pe_dim", P); ONE(lap_beta, "pe_dim", P);
  ONE(rw1_w, "pe_dim", 2 * P, LMX_GNN_RW_K); ONE(rw1_b, "pe_dim", 2 * P); ONE(rw2_w, "pe_dim", P, 2 * P); ONE(rw2_b, "pe_dim", P);
  ONE(rw_g, "pe_dim", P); ONE(rw_beta, "pe_dim", P);
  ONE(ee1_w, "d_model, edge_dim", D2, 3); ONE(ee1_b, "d_model", D2); ONE(ee2_w, "d_model", D2 / 16, Q, 64, 4); ONE(ee2_b, "d_model", D);
  ONE(ee_g, "d_model", D); ONE(ee_beta, "d_model", D);
  for (int l = 0; l < c.n_layers; ++l) {
    const std::string layer = "layer." + std::to_string(l) + ".";
    PER_LAYER(ln1_g, "d_model", D); PER_LAYER(ln1_b, "d_model", D); PER_LAYER(abde_w, "d_model", Q, 4 * Q, 64, 4); PER_LAYER(abde_b, "d_model", 4 * D);
    PER_LAYER(c_w, "d_model", Q, Q, 64, 4); PER_LAYER(c_b, "d_model", D);
    if (l < c.n_layers - 1) {
      PER_LAYER(eu1_w, "d_model", 3 * Q, Q, 64, 4); PER_LAYER(eu1_b, "d_model", D); PER_LAYER(eu2_w, "d_model", Q, Q, 64, 4); PER_LAYER(eu2_b, "d_model", D);
      PER_LAYER(bne_g, "d_model", D); PER_LAYER(bne_b, "d_model", D); PER_LAYER(bne_mean, "d_model", D); PER_LAYER(bne_var, "d_model", D);
    }
    PER_LAYER(bnn_g, "d_model", D); PER_LAYER(bnn_b, "d_model", D); PER_LAYER(bnn_mean, "d_model", D); PER_LAYER(bnn_var, "d_model", D);
    PER_LAYER(ln2_g, "d_model", D); PER_LAYER(ln2_b, "d_model", D); PER_LAYER(qkv_w, "n_heads, d_model", H * Q, 3 * dh / 16, 64, 4);
    PER_LAYER(qkv_b, "n_heads, d_model", H, 3 * dh); PER_LAYER(out_w, "d_model", Q, Q, 64, 4); PER_LAYER(out_b, "d_model", D);
    PER_LAYER(lna_g, "d_model", D); PER_LAYER(lna_b, "d_model", D); PER_LAYER(ln3_g, "d_model", D); PER_LAYER(ln3_b, "d_model", D);
    PER_LAYER(ff1_w, "d_model, ff", Q, FF / 16, 64, 4); PER_LAYER(ff1_b, "ff", FF); PER_LAYER(ff2_w, "ff, d_model", FF / 16, Q, 64, 4); PER_LAYER(ff2_b, "d_model", D);
  }
  ONE(lnf_g, "d_model", D); ONE(lnf_b, "d_model", D); ONE(nh1_w, "d_model", Q, D2 / 16, 64, 4); ONE(nh1_b, "d_model", D2); ONE(nh2_w, "d_model", D2);
  ONE(nh2_b, "one score", 1); ONE(na1_w, "d_model", Q, D2 / 16, 64, 4); ONE(na1_b, "d_model", D2); ONE(na2_w, "d_model", D2);
  ONE(na2_b, "one score", 1); ONE(cl1_w, "d_model", 2 * D, D); ONE(cl1_b, "d_model", D); ONE(cl2_w, "d_model", D, D2); ONE(cl2_b, "d_model", D2);
  ONE(cl3_w, "d_model", D2); ONE(cl3_b, "one class", 1);
#undef ONE
#undef PER_LAYER
}

extern "C" int lmx_h_gnn_tensors(const char* who, const lmx_gnn_weights_t* config_host, lmx_tensor_row_t* rows_host, int cap, int* n_host) {
  return lmx_table_export("lmx_h_gnn_tensors", who, config_host, lmx_gnn_check_config, lmx_gnn_tensor_rows, rows_host, cap, n_host);
}

int lmx_gnn_check_call(const char* who, const lmx_gnn_weights_t* w, const lmx_gnn_graphs_t* g, int S, double p, bool mc_outputs, bool eval_outputs,
                       int64_t* nodes, int* max_n, int* max_e) {
  *max_e = 0;
  return lmx_graph_check_call(
      who, g, S, p, LMX_GNN_MAX_NODES,
      [&] {
        GAIT_REQUIRE(!eval_outputs || S == 0, "%s: graph_pred, node_pred and attn_weights are read in eval mode only, S = %d", who, S);
        GAIT_REQUIRE(!mc_outputs || S > 0, "%s: node_mc and stats are written with S > 0 only", who);
        return LMX_OK;
      },
      [&](int i, int64_t N, int64_t E) {
        GAIT_REQUIRE(E <= LMX_GNN_MAX_EDGES, "%s: graph %d has E = %lld edges, more than %d", who, i, (long long)E, LMX_GNN_MAX_EDGES);
        GAIT_REQUIRE(S == 0 || N >= 2, "%s: graph %d has N = 1 node: BatchNorm has no batch statistics with S = %d", who, i, S);
        GAIT_REQUIRE(S == 0 || w->n_layers == 1 || E >= 2, "%s: graph %d has E = %lld edges: bn_edge has no batch statistics with S = %d", who, i,
                     (long long)E, S);
        if (E > *max_e) *max_e = (int)E;
        return LMX_OK;
      },
      nodes, max_n);
}

namespace {

// eigenvectors of the symmetric matrix a [N][N] (destroyed: its diagonal becomes the eigenvalues) into v [N][N], columns: cyclic Jacobi
void jacobi(std::vector<double>& a, std::vector<double>& v, int N) {
  std::fill(v.begin(), v.end(), 0.0);
  for (int i = 0; i < N; ++i) v[(size_t)i * N + i] = 1.0;
  double total = 0.0;
  for (size_t i = 0; i < a.size(); ++i) total += a[i] * a[i];
  const double bound = 1e-14 * sqrt(total);
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) off += 2.0 * a[(size_t)p * N + q] * a[(size_t)p * N + q];
    if (sqrt(off) <= bound) break;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[(size_t)p * N + q];
        if (apq == 0.0) continue;
        const double theta = (a[(size_t)q * N + q] - a[(size_t)p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {  // columns p and q
          const double akp = a[(size_t)k * N + p], akq = a[(size_t)k * N + q];
          a[(size_t)k * N + p] = c * akp - s * akq;
          a[(size_t)k * N + q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {  // rows p and q
          const double apk = a[(size_t)p * N + k], aqk = a[(size_t)q * N + k];
          a[(size_t)p * N + k] = c * apk - s * aqk;
          a[(size_t)q * N + k] = s * apk + c * aqk;
        }
        a[(size_t)p * N + q] = a[(size_t)q * N + p] = 0.0;
        for (int k = 0; k < N; ++k) {
          const double vkp = v[(size_t)k * N + p], vkq = v[(size_t)k * N + q];
          v[(size_t)k * N + p] = c * vkp - s * vkq;
          v[(size_t)k * N + q] = s * vkp + c * vkq;
        }
      }
  }
}

// A with multiplicities and one self-loop per node, and its row sums
void adjacency(const int32_t* edges, int ne, int N, std::vector<double>& A, std::vector<double>& rowsum) {
  A.assign((size_t)N * N, 0.0);
  rowsum.assign((size_t)N, 0.0);
  for (int e = 0; e < ne; ++e) A[(size_t)edges[2 * e] * N + edges[2 * e + 1]] += 1.0;
  for (int i = 0; i < N; ++i) A[(size_t)i * N + i] += 1.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) rowsum[i] += A[(size_t)i * N + j];
}

// eigenvalues (ascending, ties by the lower original column) and eigenvectors (column c belongs to eigenvalue c) of L = I - D^-1/2 A D^-1/2
// symmetrised from its lower triangle
void laplacian_eigen(const std::vector<double>& A, const std::vector<double>& rowsum, int N, double* lam, double* vec) {
  std::vector<double> L((size_t)N * N), V((size_t)N * N), dis((size_t)N);
  for (int i = 0; i < N; ++i) dis[i] = rowsum[i] > 0.0 ? 1.0 / sqrt(rowsum[i]) : 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      const double v = (i == j ? 1.0 : 0.0) - (dis[i] * A[(size_t)i * N + j]) * dis[j];
      L[(size_t)i * N + j] = L[(size_t)j * N + i] = v;
    }
  jacobi(L, V, N);
  std::vector<int> order((size_t)N);
  for (int i = 0; i < N; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return L[(size_t)a * N + a] < L[(size_t)b * N + b]; });
  for (int c = 0; c < N; ++c) {
    lam[c] = L[(size_t)order[c] * N + order[c]];
    for (int i = 0; i < N; ++i) vec[(size_t)i * N + c] = V[(size_t)i * N + order[c]];
  }
}

}  // namespace

extern "C" int lmx_h_gnn_laplacian(const int32_t* edges, int n_edges, int N, double* eigenvalues, double* eigenvectors) {
  const char* who = "lmx_h_gnn_laplacian";
  GAIT_REQUIRE(N >= 1 && N <= LMX_GNN_MAX_NODES, "%s: N %d outside 1 .. %d", who, N, LMX_GNN_MAX_NODES);
  GAIT_REQUIRE(n_edges >= 0 && n_edges <= LMX_GNN_MAX_EDGES, "%s: %d edges outside 0 .. %d", who, n_edges, LMX_GNN_MAX_EDGES);
  GAIT_REQUIRE((edges || n_edges == 0) && eigenvalues && eigenvectors, "%s: null pointer", who);
  for (int e = 0; e < n_edges; ++e)
    GAIT_REQUIRE(edges[2 * e] >= 0 && edges[2 * e] < N && edges[2 * e + 1] >= 0 && edges[2 * e + 1] < N, "%s: edge %d (%d -> %d) leaves the graph of %d nodes",
                 who, e, edges[2 * e], edges[2 * e + 1], N);
  std::vector<double> A, rowsum;
  adjacency(edges, n_edges, N, A, rowsum);
  laplacian_eigen(A, rowsum, N, eigenvalues, eigenvectors);
  return LMX_OK;
}

extern "C" int lmx_h_gnn_graph(const float* emb, const double* ts, int N, int E, int k, int32_t* edges, float* edge_attr, int32_t* n_edges,
                               int32_t* csr_ptr, int32_t* csr_edge, int32_t* deg, float* lap, float* rw) {
  const char* who = "lmx_h_gnn_graph";
  GAIT_REQUIRE(N >= 1 && N <= LMX_GNN_MAX_NODES, "%s: N %d outside 1 .. %d", who, N, LMX_GNN_MAX_NODES);
  GAIT_REQUIRE(E >= 1 && E <= (1 << 20), "%s: E = %d embedding channels", who, E);
  GAIT_REQUIRE(k >= 1 && k <= 5, "%s: k = %d neighbours outside 1 .. 5 (E <= 5 N + 2 (N - 1))", who, k);
  if (N <= k) k = std::max(1, N - 1);
  GAIT_REQUIRE(emb && ((edges && edge_attr && csr_edge) || N == 1) && n_edges && csr_ptr && deg && lap && rw, "%s: null pointer", who);
  // kNN edges weigh the raw similarity, temporal ones tanh(|dt| / a day)
  const int ne = lmx_graph_edges(
      emb, ts, N, E, k, [](double sim) { return (float)sim; }, [](double dt) { return (float)tanh(dt / 86400.0); }, edges, edge_attr);
  *n_edges = ne;
  // the edges by destination, those of one destination in edge order
  std::vector<int> din((size_t)N, 0);
  for (int e = 0; e < ne; ++e) ++din[edges[2 * e + 1]];
  csr_ptr[0] = 0;
  for (int i = 0; i < N; ++i) {
    csr_ptr[i + 1] = csr_ptr[i] + din[i];
    deg[i] = std::max(din[i], 1);
  }
  std::vector<int> fill(csr_ptr, csr_ptr + N);
  for (int e = 0; e < ne; ++e) csr_edge[fill[edges[2 * e + 1]]++] = e;
  std::vector<double> A, rowsum;
  adjacency(edges, ne, N, A, rowsum);
  // RWPE: the diagonal of P^k, P = D^-1 A
  std::vector<double> P((size_t)N * N), Pk, next((size_t)N * N);
  for (int i = 0; i < N; ++i) {
    const double inv = rowsum[i] > 0.0 ? 1.0 / rowsum[i] : 0.0;
    for (int j = 0; j < N; ++j) P[(size_t)i * N + j] = inv * A[(size_t)i * N + j];
  }
  Pk = P;
  for (int step = 0; step < LMX_GNN_RW_K; ++step) {
    for (int i = 0; i < N; ++i) rw[(size_t)i * LMX_GNN_RW_K + step] = (float)Pk[(size_t)i * N + i];
    if (step + 1 == LMX_GNN_RW_K) break;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        double s = 0.0;
        for (int m = 0; m < N; ++m) s += Pk[(size_t)i * N + m] * P[(size_t)m * N + j];
        next[(size_t)i * N + j] = s;
      }
    Pk.swap(next);
  }
  // LapPE: |columns 1 .. 8| of the eigenvectors, zero columns where N <= 8
  std::vector<double> lam((size_t)N), V((size_t)N * N);
  laplacian_eigen(A, rowsum, N, lam.data(), V.data());
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < LMX_GNN_LAP_K; ++c) lap[(size_t)i * LMX_GNN_LAP_K + c] = c + 1 < N ? (float)fabs(V[(size_t)i * N + c + 1]) : 0.0f;
  return LMX_OK;
}

namespace {

// BatchNorm over the T rows of x [T][D] in place: batch statistics (mean, biased variance, two passes) or the running ones
void batch_norm(float* x, int T, int D, bool batch, const float* g, const float* b, const float* rmean, const float* rvar) {
  for (int c = 0; c < D; ++c) {
    float mean = rmean[c], var = rvar[c];
    if (batch) {
      float sum = 0.0f, ss = 0.0f;
      for (int t = 0; t < T; ++t) sum += x[(size_t)t * D + c];
      mean = sum / (float)T;
      for (int t = 0; t < T; ++t) ss += (x[(size_t)t * D + c] - mean) * (x[(size_t)t * D + c] - mean);
      var = ss / (float)T;
    }
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int t = 0; t < T; ++t) x[(size_t)t * D + c] = (x[(size_t)t * D + c] - mean) * rstd * g[c] + b[c];
  }
}

inline float sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// LN_P( relu(in W1^T + b1) W2^T + b2 ) of one encoding: K raw columns -> 2P -> P, into out[t][0 .. P) with row stride ld
void encode(const float* in, int K, int N, int P, const float* w1, const float* b1, const float* w2, const float* b2, const float* g, const float* be,
            float* out, int ld) {
  std::vector<float> hid((size_t)2 * P), o((size_t)P);
  for (int t = 0; t < N; ++t) {
    linear(in + (size_t)t * K, K, K, hid.data(), 2 * P, 2 * P, w1, b1, 1);
    for (int j = 0; j < 2 * P; ++j) hid[j] = fmaxf(hid[j], 0.0f);
    linear(hid.data(), 2 * P, 2 * P, o.data(), P, P, w2, b2, 1);
    layer_norm(o.data(), P, out + (size_t)t * ld, ld, g, be, 1, P);
  }
}

}  // namespace

extern "C" int lmx_h_gnn_forward(const lmx_gnn_weights_t* w, const lmx_gnn_graphs_t* g, const uint64_t* seeds, int S, double p, float* node_mc,
                                 float* stats, float* graph_pred, float* node_pred, float* attn_weights, float* trunk) {
  const char* who = "lmx_h_gnn_forward";
  if (const int rc = lmx_gnn_check_config(who, w, true)) return rc;
  int64_t nodes = 0;
  int max_n = 0, max_e = 0;
  if (const int rc = lmx_gnn_check_call(who, w, g, S, p, node_mc || stats, graph_pred || node_pred || attn_weights, &nodes, &max_n, &max_e)) return rc;
  if (g->n == 0) return LMX_OK;
  const bool have_edges = g->edge_off_host[g->n] > 0;
  GAIT_REQUIRE(g->x && g->lap && g->rw && g->csr_ptr && g->deg && (!have_edges || (g->edge_src && g->edge_dst && g->edge_attr && g->csr_edge)) &&
                   (seeds || S == 0),
               "%s: null pointer", who);
  GAIT_REQUIRE(S > 0 ? (node_mc && stats) : (graph_pred && node_pred && attn_weights), "%s: an output of S = %d is null", who, S);
  const int F = w->input_dim, D = w->d_model, H = w->n_heads, dh = D / H, L = w->n_layers, FF = w->ff, P = w->pe_dim, Smax = S > 0 ? S : 1;
  const int DI = D - 2 * P, D2 = D / 2;
  for (int i = 0; i < g->n; ++i) {
    const int n0 = g->node_off_host[i], N = g->node_off_host[i + 1] - n0, e0 = g->edge_off_host[i], NE = g->edge_off_host[i + 1] - e0;
    const int32_t* ptr = g->csr_ptr + n0 + i;
    GAIT_REQUIRE(ptr[0] == 0 && ptr[N] == NE, "%s: graph %d: csr_ptr runs %d .. %d, not 0 .. %d", who, i, ptr[0], ptr[N], NE);
    for (int t = 0; t < N; ++t) {
      GAIT_REQUIRE(ptr[t + 1] >= ptr[t], "%s: graph %d: csr_ptr descends at node %d", who, i, t);
      GAIT_REQUIRE(g->deg[n0 + t] >= 1, "%s: graph %d: deg[%d] = %d is not clamped to 1", who, i, t, g->deg[n0 + t]);
      for (int q = ptr[t]; q < ptr[t + 1]; ++q) {
        const int e = g->csr_edge[e0 + q];
        GAIT_REQUIRE(e >= 0 && e < NE && g->edge_dst[e0 + e] == t, "%s: graph %d: csr_edge[%d] = %d is no edge into node %d", who, i, q, e, t);
      }
    }
    for (int e = 0; e < NE; ++e)
      GAIT_REQUIRE(g->edge_src[e0 + e] >= 0 && g->edge_src[e0 + e] < N && g->edge_dst[e0 + e] >= 0 && g->edge_dst[e0 + e] < N,
                   "%s: graph %d: edge %d (%d -> %d) leaves the graph of %d nodes", who, i, e, g->edge_src[e0 + e], g->edge_dst[e0 + e], N);
  }
  const int64_t head_floats = lmx_gnn_qkv_head_floats(*w);
  const std::vector<float> in_w = unpack(w->in_w, F, DI), ee2_w = unpack(w->ee2_w, D2, D), nh1_w = unpack(w->nh1_w, D, D2), na1_w = unpack(w->na1_w, D, D2);
  std::vector<std::vector<float>> abde_w, c_w, eu1_w, eu2_w, qkv_w, out_w, ff1_w, ff2_w;
  for (int l = 0; l < L; ++l) {
    abde_w.push_back(unpack(w->abde_w[l], D, 4 * D)), c_w.push_back(unpack(w->c_w[l], D, D));
    eu1_w.push_back(l < L - 1 ? unpack(w->eu1_w[l], 3 * D, D) : std::vector<float>());
    eu2_w.push_back(l < L - 1 ? unpack(w->eu2_w[l], D, D) : std::vector<float>());
    std::vector<float> heads;
    for (int hd = 0; hd < H; ++hd) {
      const std::vector<float> one = unpack(w->qkv_w[l] + hd * head_floats, D, 3 * dh);
      heads.insert(heads.end(), one.begin(), one.end());
    }
    qkv_w.push_back(heads), out_w.push_back(unpack(w->out_w[l], D, D));
    ff1_w.push_back(unpack(w->ff1_w[l], D, FF)), ff2_w.push_back(unpack(w->ff2_w[l], FF, D));
  }
  const size_t R = (size_t)max_n, EE = (size_t)std::max(max_e, 1);
  std::vector<float> h0(R * D), h(R * D), a(R * D), y(R * D), o(R * D), proj(R * 4 * D), hid(R * FF), qkv(R * 96), prob(R), ea0(EE * D), ea(EE * D),
      ce(EE * D), cat((size_t)3 * D), u1((size_t)D), ehid((size_t)D2), agg(R * D), nhid((size_t)D2);
  const float cs = lmx_gnn_score_scale(dh), ninf = -std::numeric_limits<float>::infinity();
  for (int i = 0; i < g->n; ++i) {
    const int n0 = g->node_off_host[i], N = g->node_off_host[i + 1] - n0, e0 = g->edge_off_host[i], NE = g->edge_off_host[i + 1] - e0;
    const int32_t *ptr = g->csr_ptr + n0 + i, *cse = g->csr_edge + e0, *src = g->edge_src + e0, *dst = g->edge_dst + e0;
    // no dropout touches the input, the encodings or the edge encoder: once per graph
    linear(g->x + (size_t)n0 * F, F, F, h0.data(), D, DI, in_w.data(), w->in_b, N);
    encode(g->lap + (size_t)n0 * LMX_GNN_LAP_K, LMX_GNN_LAP_K, N, P, w->lap1_w, w->lap1_b, w->lap2_w, w->lap2_b, w->lap_g, w->lap_beta, h0.data() + DI, D);
    encode(g->rw + (size_t)n0 * LMX_GNN_RW_K, LMX_GNN_RW_K, N, P, w->rw1_w, w->rw1_b, w->rw2_w, w->rw2_b, w->rw_g, w->rw_beta, h0.data() + DI + P, D);
    for (int e = 0; e < NE; ++e) {
      linear(g->edge_attr + (size_t)(e0 + e) * 3, 3, 3, ehid.data(), D2, D2, w->ee1_w, w->ee1_b, 1);
      for (int j = 0; j < D2; ++j) ehid[j] = fmaxf(ehid[j], 0.0f);
      linear(ehid.data(), D2, D2, u1.data(), D, D, ee2_w.data(), w->ee2_b, 1);
      layer_norm(u1.data(), D, ea0.data() + (size_t)e * D, D, w->ee_g, w->ee_beta, 1, D);
    }
    for (int s = 0; s < Smax; ++s) {
      const LmxGaitDrop drop(S, seeds, i, p, s, lmx_gnn_n_sites(L));
      memcpy(h.data(), h0.data(), (size_t)N * D * sizeof(float));
      memcpy(ea.data(), ea0.data(), (size_t)NE * D * sizeof(float));
      for (int l = 0; l < L; ++l) {
        layer_norm(h.data(), D, a.data(), D, w->ln1_g[l], w->ln1_b[l], N, D);
        linear(a.data(), D, D, proj.data(), 4 * D, 4 * D, abde_w[l].data(), w->abde_b[l], N);
        if (NE > 0) linear(ea.data(), D, D, ce.data(), D, D, c_w[l].data(), w->c_b[l], NE);
        const float *Ax = proj.data(), *Bx = proj.data() + D, *Dx = proj.data() + 2 * D, *Ex = proj.data() + 3 * D;
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) {
            float sum = 0.0f;
            for (int q = ptr[t]; q < ptr[t + 1]; ++q) {
              const int e = cse[q];
              const float sig = sigmoid((ce[(size_t)e * D + c] + Dx[(size_t)dst[e] * 4 * D + c]) + Ex[(size_t)src[e] * 4 * D + c]);
              sum += sig * Bx[(size_t)src[e] * 4 * D + c];
            }
            agg[(size_t)t * D + c] = Ax[(size_t)t * 4 * D + c] + sum / (float)g->deg[n0 + t];
          }
        if (l < L - 1 && NE > 0) {
          for (int e = 0; e < NE; ++e) {
            memcpy(cat.data(), Dx + (size_t)dst[e] * 4 * D, (size_t)D * sizeof(float));
            memcpy(cat.data() + D, Ex + (size_t)src[e] * 4 * D, (size_t)D * sizeof(float));
            memcpy(cat.data() + 2 * D, ce.data() + (size_t)e * D, (size_t)D * sizeof(float));
            linear(cat.data(), 3 * D, 3 * D, u1.data(), D, D, eu1_w[l].data(), w->eu1_b[l], 1);
            for (int c = 0; c < D; ++c) u1[c] = fmaxf(u1[c], 0.0f);
            linear(u1.data(), D, D, ea.data() + (size_t)e * D, D, D, eu2_w[l].data(), w->eu2_b[l], 1);
          }
          batch_norm(ea.data(), NE, D, S > 0, w->bne_g[l], w->bne_b[l], w->bne_mean[l], w->bne_var[l]);
        }
        batch_norm(agg.data(), N, D, S > 0, w->bnn_g[l], w->bnn_b[l], w->bnn_mean[l], w->bnn_var[l]);
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(fmaxf(agg[(size_t)t * D + c], 0.0f), 5 * l, (uint64_t)t * D + c);
        // the global attention
        layer_norm(h.data(), D, a.data(), D, w->ln2_g[l], w->ln2_b[l], N, D);
        for (int hd = 0; hd < H; ++hd) {
          linear(a.data(), D, D, qkv.data(), 3 * dh, 3 * dh, qkv_w[l].data() + (size_t)hd * 3 * dh * D, w->qkv_b[l] + hd * 3 * dh, N);
          for (int t = 0; t < N; ++t) {
            float mx = ninf, sum = 0.0f;
            for (int u = 0; u < N; ++u) {
              float sc = 0.0f;
              for (int ch = 0; ch < dh; ++ch) sc += qkv[(size_t)t * 3 * dh + ch] * qkv[(size_t)u * 3 * dh + dh + ch];
              prob[u] = sc * cs;
              mx = fmaxf(mx, prob[u]);
            }
            for (int u = 0; u < N; ++u) {
              prob[u] = expf(prob[u] - mx);
              sum += prob[u];
            }
            for (int u = 0; u < N; ++u) prob[u] = drop(prob[u] / sum, 5 * l + 1, ((uint64_t)hd * N + t) * N + u);
            for (int ch = 0; ch < dh; ++ch) {
              float acc = 0.0f;
              for (int u = 0; u < N; ++u) acc += prob[u] * qkv[(size_t)u * 3 * dh + 2 * dh + ch];
              o[(size_t)t * D + hd * dh + ch] = acc;
            }
          }
        }
        linear(o.data(), D, D, y.data(), D, D, out_w[l].data(), w->out_b[l], N);
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) y[(size_t)t * D + c] = a[(size_t)t * D + c] + drop(y[(size_t)t * D + c], 5 * l + 2, (uint64_t)t * D + c);
        layer_norm(y.data(), D, y.data(), D, w->lna_g[l], w->lna_b[l], N, D);
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += y[(size_t)t * D + c] - a[(size_t)t * D + c];
        // the FFN
        layer_norm(h.data(), D, a.data(), D, w->ln3_g[l], w->ln3_b[l], N, D);
        linear(a.data(), D, D, hid.data(), FF, FF, ff1_w[l].data(), w->ff1_b[l], N);
        for (int t = 0; t < N; ++t)
          for (int j = 0; j < FF; ++j) hid[(size_t)t * FF + j] = drop(gelu(hid[(size_t)t * FF + j]), 5 * l + 3, (uint64_t)t * FF + j);
        linear(hid.data(), FF, FF, y.data(), D, D, ff2_w[l].data(), w->ff2_b[l], N);
        for (int t = 0; t < N; ++t)
          for (int c = 0; c < D; ++c) h[(size_t)t * D + c] += drop(y[(size_t)t * D + c], 5 * l + 4, (uint64_t)t * D + c);
      }
      layer_norm(h.data(), D, a.data(), D, w->lnf_g, w->lnf_b, N, D);
      if (trunk) memcpy(trunk + ((size_t)n0 * Smax + (size_t)s * N) * D, a.data(), (size_t)N * D * sizeof(float));
      for (int t = 0; t < N; ++t) {
        linear(a.data() + (size_t)t * D, D, D, nhid.data(), D2, D2, nh1_w.data(), w->nh1_b, 1);
        float z = w->nh2_b[0];
        for (int j = 0; j < D2; ++j) z += w->nh2_w[j] * drop(fmaxf(nhid[j], 0.0f), 5 * L, (uint64_t)t * D2 + j);
        if (S > 0)
          node_mc[(size_t)(n0 + t) * S + s] = sigmoid(z);
        else
          node_pred[n0 + t] = sigmoid(z);
      }
      if (S == 0) {
        float score[LMX_GNN_MAX_NODES], comb[2 * LMX_GNN_MAX_D], k1[LMX_GNN_MAX_D], k2[LMX_GNN_MAX_D / 2];
        float mx = ninf, esum = 0.0f;
        for (int t = 0; t < N; ++t) {
          linear(a.data() + (size_t)t * D, D, D, nhid.data(), D2, D2, na1_w.data(), w->na1_b, 1);
          float sc = w->na2_b[0];
          for (int j = 0; j < D2; ++j) sc += w->na2_w[j] * tanhf(nhid[j]);
          score[t] = sc;
          mx = fmaxf(mx, sc);
        }
        for (int t = 0; t < N; ++t) {
          score[t] = expf(score[t] - mx);
          esum += score[t];
        }
        for (int t = 0; t < N; ++t) attn_weights[n0 + t] = score[t] = score[t] / esum;
        for (int c = 0; c < D; ++c) {
          float sum = 0.0f, pool = 0.0f;
          for (int t = 0; t < N; ++t) sum += a[(size_t)t * D + c];
          for (int t = 0; t < N; ++t) pool += score[t] * a[(size_t)t * D + c];
          comb[c] = sum / (float)N;
          comb[D + c] = pool;
        }
        linear_t(comb, 2 * D, k1, D, w->cl1_w, w->cl1_b);
        for (int c = 0; c < D; ++c) k1[c] = fmaxf(k1[c], 0.0f);
        linear_t(k1, D, k2, D2, w->cl2_w, w->cl2_b);
        float z = w->cl3_b[0];
        for (int j = 0; j < D2; ++j) z += w->cl3_w[j] * fmaxf(k2[j], 0.0f);
        graph_pred[i] = sigmoid(z);
      }
    }
    if (S > 0)
      for (int t = 0; t < N; ++t) lmx_gait_row_stats(node_mc + (size_t)(n0 + t) * S, S, stats + 2 * (size_t)(n0 + t));
  }
  return LMX_OK;
}
