// graph_model.hip — the model-level entry points of the C-ABI for the two graph models, the graph transformer (lmx_gfm_*) and GraphGPS
// (lmx_gnn_*), whose calls take a batch of graphs: ONE handle (model_handle.h has what every handle owns) with the weights of one weight
// image (gfm_image.h, gnn_image.h) and a workspace sized for the handle's limits, and lmx_<model>_score, which is lmx_k_<model>_forward
// (gfm.hip, gnn.hip) with the image's dropout probability.  A model is a traits struct: its image, its weights, its workspace, the
// arrays of its graphs and its outputs, and how a call is checked and run; the handle, its limits and the upload / run / download of
// the *_host calls are written once.  The two gait models have the same arrangement in gait_model.hip.  HOST code only: there is no
// kernel in this file.
#include <type_traits>

#include "gait_launch.h"
#include "gfm_image.h"
#include "gnn_image.h"
#include "model_handle.h"

namespace {

struct GraphSizes {
  int64_t nodes = 0, edges = 0, cells = 0;  // sum N, sum E, sum N^2 (the graph transformer's matrices)
};

template <class M>
struct GraphHandle : LmxHandleCore {
  typename M::Image img;
  typename M::Weights w;  // device pointers into `weights`
  int max_samples = 0, max_nodes_total = 0, max_edges_total = 0;
  char* ws = nullptr;  // M::workspace_bytes of the limits
};

// the graph transformer: a kind-6 image; the workspace holds seeds, offsets and the attention bias of max_graphs graphs of max_nodes_total
// nodes in all (sum N^2 <= LMX_GFM_MAX_NODES sum N).  out = pred, stats, node_pred, attn_to_target
struct Gfm {
  typedef LmxGfmImage Image;
  typedef lmx_gfm_weights_t Weights;
  typedef lmx_gfm_graphs_t Graphs;
  enum { N_IN = 9, N_OUT = 4, MAX_EDGES_TOTAL = 0 };  // the open takes no edge limit
  static constexpr const char* open_name = "lmx_gfm_open_host";
  static constexpr auto parse = lmx_gfm_image_parse;
  static constexpr auto bind = lmx_gfm_bind;
  static constexpr auto check_config = lmx_gfm_check_config;
  static int64_t workspace_bytes(const GraphHandle<Gfm>& m) {
    return lmx_gfm_workspace_bytes(m.max_batch, (int64_t)m.max_nodes_total * LMX_GFM_MAX_NODES, m.w.n_heads);
  }
  static int check_call(const char* fn, const Weights&, double p, const Graphs* g, const uint64_t* seeds, int S, float* const* out, GraphSizes* z) {
    LMX_REQUIRE(out[0] && out[1] && (seeds || S == 0), "%s: null pointer", fn);
    int max_n = 0;
    return lmx_gfm_check_call(fn, g, S, p, out[2] || out[3], &z->nodes, &z->cells, &max_n);
  }
  // what a *_host call needs of the arrays it uploads
  static int check_arrays(const char* fn, const Graphs* g, float* const* out, const GraphSizes& z) {
    LMX_REQUIRE(g->x && g->deg_in && g->deg_out && g->idx && g->win && (g->edge_attr || z.edges == 0), "%s: null pointer", fn);
    LMX_REQUIRE(!g->has_time || g->timestamps, "%s: has_time without timestamps", fn);
    LMX_REQUIRE(!out[3] || g->target, "%s: attn_to_target without target", fn);
    return LMX_OK;
  }
  // f(array of the graphs, its bytes): an array that is not there takes no bytes
  template <class F>
  static void inputs(Graphs& g, const Weights& w, const GraphSizes& z, F f) {
    const size_t n = (size_t)g.n, N = (size_t)z.nodes, C = (size_t)z.cells;
    f(g.x, N * w.input_dim * 4), f(g.timestamps, g.timestamps ? N * 4 : 0), f(g.has_time, g.has_time ? n : 0), f(g.deg_in, N), f(g.deg_out, N);
    f(g.idx, C), f(g.win, C * 4), f(g.edge_attr, (size_t)z.edges * 12), f(g.target, g.target ? n * 4 : 0);
  }
  static void out_bytes(int n, int S, const GraphSizes& z, float* const* out, size_t* bytes) {
    bytes[0] = (size_t)n * (S > 0 ? S : 1) * 4, bytes[1] = (size_t)n * 8;
    bytes[2] = out[2] ? (size_t)z.nodes * 4 : 0, bytes[3] = out[3] ? (size_t)z.nodes * 4 : 0;
  }
  static int forward(const Weights* w, const Graphs* g, const uint64_t* seeds_host, int S, double p, float* const* out, void* ws, lmx_stream_t stream) {
    return lmx_k_gfm_forward(w, g, seeds_host, S, p, out[0], out[1], out[2], out[3], nullptr, nullptr, ws, stream);
  }
};

// GraphGPS: a kind-7 image; the workspace holds one slice per (graph, sample) sized for the handle's limits.
// out = node_mc, stats (S > 0), graph_pred, node_pred, attn_weights (S = 0)
struct Gnn {
  typedef LmxGnnImage Image;
  typedef lmx_gnn_weights_t Weights;
  typedef lmx_gnn_graphs_t Graphs;
  enum { N_IN = 9, N_OUT = 5, MAX_EDGES_TOTAL = 1 << 25 };
  static constexpr const char* open_name = "lmx_gnn_open_host";
  static constexpr auto parse = lmx_gnn_image_parse;
  static constexpr auto bind = lmx_gnn_bind;
  static constexpr auto check_config = lmx_gnn_check_config;
  static int64_t workspace_bytes(const GraphHandle<Gnn>& m) {
    const int mn = m.max_nodes_total < LMX_GNN_MAX_NODES ? m.max_nodes_total : LMX_GNN_MAX_NODES;
    const int me = m.max_edges_total < LMX_GNN_MAX_EDGES ? m.max_edges_total : LMX_GNN_MAX_EDGES;
    return lmx_gnn_workspace_bytes(m.max_batch, m.max_samples, mn, me, m.w.d_model, m.w.n_layers);
  }
  static int check_call(const char* fn, const Weights& w, double p, const Graphs* g, const uint64_t* seeds, int S, float* const* out, GraphSizes* z) {
    int max_n = 0, max_e = 0;
    LMX_TRY(lmx_gnn_check_call(fn, &w, g, S, p, out[0] || out[1], out[2] || out[3] || out[4], &z->nodes, &max_n, &max_e));
    LMX_REQUIRE(S > 0 ? (out[0] && out[1] && seeds) : (out[2] && out[3] && out[4]), "%s: an output of S = %d, or the seeds, is null", fn, S);
    return LMX_OK;
  }
  static int check_arrays(const char* fn, const Graphs* g, float* const*, const GraphSizes& z) {
    LMX_REQUIRE(g->x && g->lap && g->rw && g->csr_ptr && g->deg && (z.edges == 0 || (g->edge_src && g->edge_dst && g->edge_attr && g->csr_edge)),
                "%s: null pointer", fn);
    return LMX_OK;
  }
  template <class F>
  static void inputs(Graphs& g, const Weights& w, const GraphSizes& z, F f) {
    const size_t N = (size_t)z.nodes, E = (size_t)z.edges;
    f(g.x, N * w.input_dim * 4), f(g.lap, N * LMX_GNN_LAP_K * 4), f(g.rw, N * LMX_GNN_RW_K * 4), f(g.edge_src, E * 4), f(g.edge_dst, E * 4);
    f(g.edge_attr, E * 12), f(g.csr_ptr, (N + g.n) * 4), f(g.csr_edge, E * 4), f(g.deg, N * 4);
  }
  static void out_bytes(int n, int S, const GraphSizes& z, float* const*, size_t* bytes) {
    const size_t N = (size_t)z.nodes;
    bytes[0] = S ? N * S * 4 : 0, bytes[1] = S ? N * 8 : 0, bytes[2] = S ? 0 : (size_t)n * 4, bytes[3] = bytes[4] = S ? 0 : N * 4;
  }
  static int forward(const Weights* w, const Graphs* g, const uint64_t* seeds_host, int S, double p, float* const* out, void* ws, lmx_stream_t stream) {
    return lmx_k_gnn_forward(w, g, seeds_host, S, p, out[0], out[1], out[2], out[3], out[4], nullptr, ws, stream);
  }
};

}  // namespace

struct lmx_gfm : GraphHandle<Gfm> {};
struct lmx_gnn : GraphHandle<Gnn> {};

namespace {

template <class H>
void destroy(H* m) {
  (void)hipFree(m->ws);
  lmx_handle_free(m);
  delete m;
}

template <class M, class H>
int open_into(H* m, const char* path) {
  LMX_TRY(M::parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, M::open_name, path, m->img.data_offset, m->img.file_bytes));
  M::bind(m->img, m->weights, &m->w);
  return M::check_config(M::open_name, &m->w, true);
}

template <class M, class H>
int open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, H** out_host) {
  const char* fn = M::open_name;
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", fn);
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "%s: max_samples %d outside 2 .. 65535", fn, max_samples);
  LMX_REQUIRE(max_nodes_total >= 1 && max_nodes_total <= (1 << 22), "%s: max_nodes_total %d outside 1 .. %d", fn, max_nodes_total, 1 << 22);
  LMX_REQUIRE(max_edges_total >= 0 && max_edges_total <= M::MAX_EDGES_TOTAL, "%s: max_edges_total %d outside 0 .. %d", fn, max_edges_total,
              (int)M::MAX_EDGES_TOTAL);
  LMX_TRY(lmx_handle_open(fn, path_host, max_graphs, out_host, open_into<M, H>, destroy<H>));
  H* m = *out_host;
  m->max_samples = max_samples;
  m->max_nodes_total = max_nodes_total;
  m->max_edges_total = max_edges_total;
  const int64_t bytes = M::workspace_bytes(*m);
  if (hipMalloc(reinterpret_cast<void**>(&m->ws), (size_t)bytes) != hipSuccess) {
    lmx_handle_close(m, destroy<H>);
    *out_host = nullptr;
    lmx_set_error("%s: no memory for a workspace of %lld bytes", fn, (long long)bytes);
    return LMX_EINVAL;
  }
  return LMX_OK;
}

// the handle's own limits around the model's checks of a call
template <class M>
int check_call(const GraphHandle<M>* m, const char* fn, const typename M::Graphs* g, const uint64_t* seeds, int S, float* const* out, GraphSizes* z) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(g != nullptr, "%s: null graphs", fn);
  LMX_REQUIRE(g->n > 0 && g->n <= m->max_batch, "%s: n = %d graphs, the handle was opened for 1 .. %d", fn, g->n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  LMX_TRY(M::check_call(fn, m->w, m->img.p, g, seeds, S, out, z));
  z->edges = g->edge_off_host[g->n];
  LMX_REQUIRE(z->nodes <= m->max_nodes_total, "%s: %lld nodes in all, the handle was opened for up to %d", fn, (long long)z->nodes, m->max_nodes_total);
  LMX_REQUIRE(!M::MAX_EDGES_TOTAL || z->edges <= m->max_edges_total, "%s: %lld edges in all, the handle was opened for up to %d", fn,
              (long long)z->edges, m->max_edges_total);
  return LMX_OK;
}

template <class M>
int score(GraphHandle<M>* m, const char* fn, const typename M::Graphs* graphs_host, const uint64_t* seeds_host, int S, float* const* out,
          lmx_stream_t stream) {
  GraphSizes z;
  LMX_TRY(check_call(m, fn, graphs_host, seeds_host, S, out, &z));
  LMX_TRY(lmx_handle_stream_on_device(m, fn, reinterpret_cast<hipStream_t>(stream)));
  return M::forward(&m->w, graphs_host, seeds_host, S, m->img.p, out, m->ws, stream);
}

// upload the arrays that are there, run, download the outputs that are asked for (or that the mode writes), synchronise
template <class M>
int score_host(GraphHandle<M>* m, const char* fn, const typename M::Graphs* g, const uint64_t* seeds_host, int S, float* const* out_host) {
  GraphSizes z;
  LMX_TRY(check_call(m, fn, g, seeds_host, S, out_host, &z));
  LMX_TRY(M::check_arrays(fn, g, out_host, z));
  // staging: the graph arrays, then the outputs, each on a 256-byte boundary
  typename M::Graphs d = *g;
  const void* in_src[M::N_IN];
  size_t in_bytes[M::N_IN], in_at[M::N_IN], out_bytes[M::N_OUT], out_at[M::N_OUT];
  LmxLayout lay;
  int i = 0;
  M::inputs(d, m->w, z, [&](auto* array, size_t bytes) { in_src[i] = array, in_bytes[i] = bytes, in_at[i] = lay.add(bytes), ++i; });
  M::out_bytes(g->n, S, z, out_host, out_bytes);
  for (i = 0; i < M::N_OUT; ++i) out_at[i] = lay.add(out_bytes[i]);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  for (i = 0; i < M::N_IN; ++i)
    if (in_bytes[i]) LMX_HIP(hipMemcpyAsync(m->stage + in_at[i], in_src[i], in_bytes[i], hipMemcpyHostToDevice, m->own));
  i = 0;
  M::inputs(d, m->w, z, [&](auto*& array, size_t) {
    array = in_bytes[i] ? reinterpret_cast<std::remove_reference_t<decltype(array)>>(m->stage + in_at[i]) : nullptr;
    ++i;
  });
  float* out_dev[M::N_OUT];
  for (i = 0; i < M::N_OUT; ++i) out_dev[i] = out_bytes[i] ? reinterpret_cast<float*>(m->stage + out_at[i]) : nullptr;
  LMX_TRY(M::forward(&m->w, &d, seeds_host, S, m->img.p, out_dev, m->ws, m->own));
  for (i = 0; i < M::N_OUT; ++i)
    if (out_bytes[i]) LMX_HIP(hipMemcpyAsync(out_host[i], out_dev[i], out_bytes[i], hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_gfm_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_samples, lmx_gfm** out_host) {
  return open_host<Gfm>(path_host, max_graphs, max_nodes_total, 0, max_samples, out_host);
}
extern "C" int lmx_gnn_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, lmx_gnn** out_host) {
  return open_host<Gnn>(path_host, max_graphs, max_nodes_total, max_edges_total, max_samples, out_host);
}

extern "C" void lmx_gfm_close(lmx_gfm* m) { lmx_handle_close(m, destroy<lmx_gfm>); }
extern "C" void lmx_gnn_close(lmx_gnn* m) { lmx_handle_close(m, destroy<lmx_gnn>); }

extern "C" int lmx_gfm_info(const lmx_gfm* m, lmx_gfm_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_gfm_info: null argument");
  lmx_gfm_fill_info(m->img, m->max_batch, m->max_nodes_total, m->max_samples, info_host);
  return LMX_OK;
}
extern "C" int lmx_gnn_info(const lmx_gnn* m, lmx_gnn_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_gnn_info: null argument");
  lmx_gnn_fill_info(m->img, m->max_batch, m->max_nodes_total, m->max_edges_total, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_gfm_score(lmx_gfm* m, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* pred, float* stats,
                             float* node_pred, float* attn_to_target, lmx_stream_t stream) {
  float* const out[] = {pred, stats, node_pred, attn_to_target};
  return score(m, "lmx_gfm_score", graphs_host, seeds_host, S, out, stream);
}
extern "C" int lmx_gnn_score(lmx_gnn* m, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* node_mc, float* stats,
                             float* graph_pred, float* node_pred, float* attn_weights, lmx_stream_t stream) {
  float* const out[] = {node_mc, stats, graph_pred, node_pred, attn_weights};
  return score(m, "lmx_gnn_score", graphs_host, seeds_host, S, out, stream);
}

extern "C" int lmx_gfm_score_host(lmx_gfm* m, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* pred_host,
                                  float* stats_host, float* node_pred_host, float* attn_host) {
  float* const out[] = {pred_host, stats_host, node_pred_host, attn_host};
  return score_host(m, "lmx_gfm_score_host", graphs_host, seeds_host, S, out);
}
extern "C" int lmx_gnn_score_host(lmx_gnn* m, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* node_mc_host,
                                  float* stats_host, float* graph_pred_host, float* node_pred_host, float* attn_host) {
  float* const out[] = {node_mc_host, stats_host, graph_pred_host, node_pred_host, attn_host};
  return score_host(m, "lmx_gnn_score_host", graphs_host, seeds_host, S, out);
}
