// gait_model.hip — the model-level entry points of the C-ABI for the two gait sequence models, the TCN (lmx_tcn_*) and the gait
// transformer (lmx_xfm_*), and at the end of the file for the graph transformer (lmx_gfm_*), whose calls take graphs and not series: ONE handle (model_handle.h has what every handle owns) with the weights of one weight image (tcn_image.h,
// xfm_image.h) and the seed workspace of max_clips clips, and lmx_<model>_score, which is lmx_k_<model>_forward (tcn.hip, xfm.hip) with
// the image's configuration and dropout probability (services/tcn-pipeline/app/main.py:357-364,
// services/transformer-pipeline/app/main.py:421-441).  A model is a traits struct: its image, its weights, and how a call is checked
// and run.  HOST code only: there is no kernel in this file.
#include "gait_launch.h"
#include "gfm_image.h"
#include "gnn_image.h"
#include "model_handle.h"
#include "tcn_image.h"
#include "xfm_image.h"

namespace {

struct Tcn {
  typedef LmxTcnImage Image;
  typedef lmx_tcn_weights_t Weights;
  static constexpr const char* open_name = "lmx_tcn_open_host";
  static constexpr auto parse = lmx_tcn_image_parse;
  static constexpr auto bind = lmx_tcn_bind;
  static constexpr auto check_config = lmx_tcn_check_config;
  // T only: S = 1 and p are lmx_k_tcn_forward's to refuse, under its own name
  static int check_call(const char* fn, const Weights&, int n, int T, int, double, bool) {
    return lmx_gait_check_call(fn, n, T, 0, 0.0, LMX_TCN_MAX_T, "");
  }
  static int forward(const Weights* w, const float* x, const uint8_t*, const uint64_t* seeds_host, int n, int T, int S, double p, float* pred,
                     float* stats, float*, void* workspace, lmx_stream_t stream) {
    return lmx_k_tcn_forward(w, x, seeds_host, n, T, S, p, pred, stats, nullptr, workspace, stream);
  }
};

struct Xfm {
  typedef LmxXfmImage Image;
  typedef lmx_xfm_weights_t Weights;
  static constexpr const char* open_name = "lmx_xfm_open_host";
  static constexpr auto parse = lmx_xfm_image_parse;
  static constexpr auto bind = lmx_xfm_bind;
  static constexpr auto check_config = lmx_xfm_check_config;
  static int check_call(const char* fn, const Weights& w, int n, int T, int S, double p, bool saliency) {
    return lmx_xfm_check_call(fn, &w, n, T, S, p, saliency);
  }
  static int forward(const Weights* w, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S, double p, float* pred,
                     float* stats, float* saliency, void* workspace, lmx_stream_t stream) {
    return lmx_k_xfm_forward(w, x, mask, seeds_host, n, T, S, p, pred, stats, saliency, nullptr, workspace, stream);
  }
};

template <class M>
struct GaitHandle : LmxHandleCore {
  typename M::Image img;
  typename M::Weights w;  // device pointers into `weights`
  int max_samples = 0;
  char* seeds = nullptr;  // lmx_gait_workspace_bytes(max_clips)
};

}  // namespace

struct lmx_tcn : GaitHandle<Tcn> {};
struct lmx_xfm : GaitHandle<Xfm> {};

namespace {

template <class H>
void destroy(H* m) {
  (void)hipFree(m->seeds);
  lmx_handle_free(m);
  delete m;
}

template <class M, class H>
int open_into(H* m, const char* path) {
  LMX_TRY(M::parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, M::open_name, path, m->img.data_offset, m->img.file_bytes));
  M::bind(m->img, m->weights, &m->w);
  LMX_TRY(M::check_config(M::open_name, &m->w, true));
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->seeds), (size_t)lmx_gait_workspace_bytes(m->max_batch)));
  return LMX_OK;
}

template <class M, class H>
int open_host(const char* path_host, int max_clips, int max_samples, H** out_host) {
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", M::open_name);
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "%s: max_samples %d outside 2 .. 65535", M::open_name, max_samples);
  LMX_TRY(lmx_handle_open(M::open_name, path_host, max_clips, out_host, open_into<M, H>, destroy<H>));
  (*out_host)->max_samples = max_samples;
  return LMX_OK;
}

template <class M>
int check_call(const GaitHandle<M>* m, const char* fn, const void* x, const uint64_t* seeds, int n, int T, int S, const void* pred, const void* stats,
               const void* saliency) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0 && n <= m->max_batch, "%s: n = %d clips, the handle was opened for 1 .. %d", fn, n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  LMX_REQUIRE(x && pred && stats && (seeds || S == 0), "%s: null pointer", fn);
  return M::check_call(fn, m->w, n, T, S, m->img.p, saliency != nullptr);
}

template <class M>
int score(GaitHandle<M>* m, const char* fn, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S, float* pred,
          float* stats, float* saliency, lmx_stream_t stream) {
  LMX_TRY(check_call(m, fn, x, seeds_host, n, T, S, pred, stats, saliency));
  LMX_TRY(lmx_handle_stream_on_device(m, fn, reinterpret_cast<hipStream_t>(stream)));
  return M::forward(&m->w, x, mask, seeds_host, n, T, S, m->img.p, pred, stats, saliency, m->seeds, stream);
}

// upload the inputs that are there, run, download the outputs that are asked for, synchronise
template <class M>
int score_host(GaitHandle<M>* m, const char* fn, const float* x_host, const uint8_t* mask_host, const uint64_t* seeds_host, int n, int T, int S,
               float* pred_host, float* stats_host, float* saliency_host) {
  LMX_TRY(check_call(m, fn, x_host, seeds_host, n, T, S, pred_host, stats_host, saliency_host));
  // staging: series | mask | predictions | stats | saliency, each on a 256-byte boundary; a buffer that is not there takes no bytes
  const size_t x_bytes = (size_t)n * T * m->w.input_dim * sizeof(float), mask_bytes = mask_host ? (size_t)n * T : 0,
               pred_bytes = (size_t)n * (S > 0 ? S : 1) * sizeof(float), stats_bytes = (size_t)n * 2 * sizeof(float),
               sal_bytes = saliency_host ? (size_t)n * T * sizeof(float) : 0;
  LmxLayout lay;
  const size_t o_x = lay.add(x_bytes), o_mask = lay.add(mask_bytes), o_pred = lay.add(pred_bytes), o_stats = lay.add(stats_bytes),
               o_sal = lay.add(sal_bytes);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  float* x = reinterpret_cast<float*>(m->stage + o_x);
  uint8_t* mask = mask_host ? reinterpret_cast<uint8_t*>(m->stage + o_mask) : nullptr;
  float* pred = reinterpret_cast<float*>(m->stage + o_pred);
  float* stats = reinterpret_cast<float*>(m->stage + o_stats);
  float* sal = saliency_host ? reinterpret_cast<float*>(m->stage + o_sal) : nullptr;
  LMX_HIP(hipMemcpyAsync(x, x_host, x_bytes, hipMemcpyHostToDevice, m->own));
  if (mask) LMX_HIP(hipMemcpyAsync(mask, mask_host, mask_bytes, hipMemcpyHostToDevice, m->own));
  LMX_TRY(M::forward(&m->w, x, mask, seeds_host, n, T, S, m->img.p, pred, stats, sal, m->seeds, m->own));
  LMX_HIP(hipMemcpyAsync(pred_host, pred, pred_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipMemcpyAsync(stats_host, stats, stats_bytes, hipMemcpyDeviceToHost, m->own));
  if (sal) LMX_HIP(hipMemcpyAsync(saliency_host, sal, sal_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_tcn_open_host(const char* path_host, int max_clips, int max_samples, lmx_tcn** out_host) {
  return open_host<Tcn>(path_host, max_clips, max_samples, out_host);
}
extern "C" int lmx_xfm_open_host(const char* path_host, int max_clips, int max_samples, lmx_xfm** out_host) {
  return open_host<Xfm>(path_host, max_clips, max_samples, out_host);
}

extern "C" void lmx_tcn_close(lmx_tcn* m) { lmx_handle_close(m, destroy<lmx_tcn>); }
extern "C" void lmx_xfm_close(lmx_xfm* m) { lmx_handle_close(m, destroy<lmx_xfm>); }

extern "C" int lmx_tcn_info(const lmx_tcn* m, lmx_tcn_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_tcn_info: null argument");
  lmx_tcn_fill_info(m->img, m->max_batch, m->max_samples, info_host);
  return LMX_OK;
}
extern "C" int lmx_xfm_info(const lmx_xfm* m, lmx_xfm_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_xfm_info: null argument");
  lmx_xfm_fill_info(m->img, m->max_batch, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_tcn_score(lmx_tcn* m, const float* x, const uint64_t* seeds_host, int n, int T, int S, float* pred, float* stats,
                             lmx_stream_t stream) {
  return score(m, "lmx_tcn_score", x, nullptr, seeds_host, n, T, S, pred, stats, nullptr, stream);
}
extern "C" int lmx_xfm_score(lmx_xfm* m, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S, float* pred,
                             float* stats, float* saliency, lmx_stream_t stream) {
  return score(m, "lmx_xfm_score", x, mask, seeds_host, n, T, S, pred, stats, saliency, stream);
}

extern "C" int lmx_tcn_score_host(lmx_tcn* m, const float* x_host, const uint64_t* seeds_host, int n, int T, int S, float* pred_host,
                                  float* stats_host) {
  return score_host(m, "lmx_tcn_score_host", x_host, nullptr, seeds_host, n, T, S, pred_host, stats_host, nullptr);
}
extern "C" int lmx_xfm_score_host(lmx_xfm* m, const float* x_host, const uint8_t* mask_host, const uint64_t* seeds_host, int n, int T, int S,
                                  float* pred_host, float* stats_host, float* saliency_host) {
  return score_host(m, "lmx_xfm_score_host", x_host, mask_host, seeds_host, n, T, S, pred_host, stats_host, saliency_host);
}

// ---- the graph transformer: the same handle core, the weights of a kind-6 image, a workspace for max_graphs graphs of max_nodes_total
// nodes in all (seeds, offsets and the attention bias), and lmx_gfm_score = lmx_k_gfm_forward with the image's dropout probability ----
struct lmx_gfm : LmxHandleCore {
  LmxGfmImage img;
  lmx_gfm_weights_t w;  // device pointers into `weights`
  int max_samples = 0, max_nodes_total = 0;
  char* ws = nullptr;   // lmx_gfm_workspace_bytes(max_graphs, max_nodes_total * LMX_GFM_MAX_NODES, H): sum N^2 <= LMX_GFM_MAX_NODES sum N
};

namespace {

void gfm_destroy(lmx_gfm* m) {
  (void)hipFree(m->ws);
  lmx_handle_free(m);
  delete m;
}

int gfm_open_into(lmx_gfm* m, const char* path) {
  LMX_TRY(lmx_gfm_image_parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_gfm_open_host", path, m->img.data_offset, m->img.file_bytes));
  lmx_gfm_bind(m->img, m->weights, &m->w);
  return lmx_gfm_check_config("lmx_gfm_open_host", &m->w, true);
}

// the handle's own limits on top of the checks of every forward; *nodes = sum N
int gfm_check_call(const lmx_gfm* m, const char* fn, const lmx_gfm_graphs_t* g, const uint64_t* seeds, int S, const void* pred, const void* stats,
                   bool eval_outputs, int64_t* nodes, int64_t* cells) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(g != nullptr, "%s: null graphs", fn);
  LMX_REQUIRE(g->n > 0 && g->n <= m->max_batch, "%s: n = %d graphs, the handle was opened for 1 .. %d", fn, g->n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  LMX_REQUIRE(pred && stats && (seeds || S == 0), "%s: null pointer", fn);
  int max_n = 0;
  LMX_TRY(lmx_gfm_check_call(fn, g, S, m->img.p, eval_outputs, nodes, cells, &max_n));
  LMX_REQUIRE(*nodes <= m->max_nodes_total, "%s: %lld nodes in all, the handle was opened for up to %d", fn, (long long)*nodes, m->max_nodes_total);
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_gfm_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_samples, lmx_gfm** out_host) {
  const char* fn = "lmx_gfm_open_host";
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", fn);
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "%s: max_samples %d outside 2 .. 65535", fn, max_samples);
  LMX_REQUIRE(max_nodes_total >= 1 && max_nodes_total <= (1 << 22), "%s: max_nodes_total %d outside 1 .. %d", fn, max_nodes_total, 1 << 22);
  LMX_TRY(lmx_handle_open(fn, path_host, max_graphs, out_host, gfm_open_into, gfm_destroy));
  lmx_gfm* m = *out_host;
  m->max_samples = max_samples;
  m->max_nodes_total = max_nodes_total;
  const int64_t bytes = lmx_gfm_workspace_bytes(max_graphs, (int64_t)max_nodes_total * LMX_GFM_MAX_NODES, m->w.n_heads);
  if (hipMalloc(reinterpret_cast<void**>(&m->ws), (size_t)bytes) != hipSuccess) {
    lmx_handle_close(m, gfm_destroy);
    *out_host = nullptr;
    lmx_set_error("%s: no memory for a workspace of %lld bytes", fn, (long long)bytes);
    return LMX_EINVAL;
  }
  return LMX_OK;
}

extern "C" void lmx_gfm_close(lmx_gfm* m) { lmx_handle_close(m, gfm_destroy); }

extern "C" int lmx_gfm_info(const lmx_gfm* m, lmx_gfm_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_gfm_info: null argument");
  lmx_gfm_fill_info(m->img, m->max_batch, m->max_nodes_total, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_gfm_score(lmx_gfm* m, const lmx_gfm_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* pred, float* stats,
                             float* node_pred, float* attn_to_target, lmx_stream_t stream) {
  const char* fn = "lmx_gfm_score";
  int64_t nodes = 0, cells = 0;
  LMX_TRY(gfm_check_call(m, fn, graphs_host, seeds_host, S, pred, stats, node_pred || attn_to_target, &nodes, &cells));
  LMX_TRY(lmx_handle_stream_on_device(m, fn, reinterpret_cast<hipStream_t>(stream)));
  return lmx_k_gfm_forward(&m->w, graphs_host, seeds_host, S, m->img.p, pred, stats, node_pred, attn_to_target, nullptr, nullptr, m->ws, stream);
}

// upload the arrays that are there, run, download the outputs that are asked for, synchronise
extern "C" int lmx_gfm_score_host(lmx_gfm* m, const lmx_gfm_graphs_t* g, const uint64_t* seeds_host, int S, float* pred_host, float* stats_host,
                                  float* node_pred_host, float* attn_host) {
  const char* fn = "lmx_gfm_score_host";
  int64_t nodes = 0, cells = 0;
  LMX_TRY(gfm_check_call(m, fn, g, seeds_host, S, pred_host, stats_host, node_pred_host || attn_host, &nodes, &cells));
  const int n = g->n;
  const size_t edges = (size_t)g->edge_off_host[n];
  LMX_REQUIRE(g->x && g->deg_in && g->deg_out && g->idx && g->win && (g->edge_attr || edges == 0), "%s: null pointer", fn);
  LMX_REQUIRE(!g->has_time || g->timestamps, "%s: has_time without timestamps", fn);
  LMX_REQUIRE(!attn_host || g->target, "%s: attn_to_target without target", fn);
  // staging: the graph arrays, then the outputs, each on a 256-byte boundary; an array that is not there takes no bytes
  const size_t in_bytes[9] = {(size_t)nodes * m->w.input_dim * 4, g->timestamps ? (size_t)nodes * 4 : 0, g->has_time ? (size_t)n : 0, (size_t)nodes,
                              (size_t)nodes, (size_t)cells, (size_t)cells * 4, edges * 12, g->target ? (size_t)n * 4 : 0};
  const void* in_src[9] = {g->x, g->timestamps, g->has_time, g->deg_in, g->deg_out, g->idx, g->win, g->edge_attr, g->target};
  const size_t out_bytes[4] = {(size_t)n * (S > 0 ? S : 1) * 4, (size_t)n * 8, node_pred_host ? (size_t)nodes * 4 : 0, attn_host ? (size_t)nodes * 4 : 0};
  void* out_dst[4] = {pred_host, stats_host, node_pred_host, attn_host};
  LmxLayout lay;
  size_t in_at[9], out_at[4];
  for (int i = 0; i < 9; ++i) in_at[i] = lay.add(in_bytes[i]);
  for (int i = 0; i < 4; ++i) out_at[i] = lay.add(out_bytes[i]);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  void* in_dev[9];
  for (int i = 0; i < 9; ++i) {
    in_dev[i] = in_bytes[i] ? m->stage + in_at[i] : nullptr;
    if (in_bytes[i]) LMX_HIP(hipMemcpyAsync(in_dev[i], in_src[i], in_bytes[i], hipMemcpyHostToDevice, m->own));
  }
  float* out_dev[4];
  for (int i = 0; i < 4; ++i) out_dev[i] = out_bytes[i] ? reinterpret_cast<float*>(m->stage + out_at[i]) : nullptr;
  lmx_gfm_graphs_t d = *g;
  d.x = static_cast<const float*>(in_dev[0]), d.timestamps = static_cast<const float*>(in_dev[1]), d.has_time = static_cast<const uint8_t*>(in_dev[2]);
  d.deg_in = static_cast<const uint8_t*>(in_dev[3]), d.deg_out = static_cast<const uint8_t*>(in_dev[4]), d.idx = static_cast<const uint8_t*>(in_dev[5]);
  d.win = static_cast<const int32_t*>(in_dev[6]), d.edge_attr = static_cast<const float*>(in_dev[7]), d.target = static_cast<const int32_t*>(in_dev[8]);
  LMX_TRY(lmx_k_gfm_forward(&m->w, &d, seeds_host, S, m->img.p, out_dev[0], out_dev[1], out_dev[2], out_dev[3], nullptr, nullptr, m->ws, m->own));
  for (int i = 0; i < 4; ++i)
    if (out_bytes[i]) LMX_HIP(hipMemcpyAsync(out_dst[i], out_dev[i], out_bytes[i], hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}

// ---- GraphGPS: the same handle core, the weights of a kind-7 image, a workspace of one slice per (graph, sample) sized for the handle's
// limits, and lmx_gnn_score = lmx_k_gnn_forward with the image's dropout probability ----------------------------------------------------
struct lmx_gnn : LmxHandleCore {
  LmxGnnImage img;
  lmx_gnn_weights_t w;  // device pointers into `weights`
  int max_samples = 0, max_nodes_total = 0, max_edges_total = 0;
  char* ws = nullptr;
};

namespace {

void gnn_destroy(lmx_gnn* m) {
  (void)hipFree(m->ws);
  lmx_handle_free(m);
  delete m;
}

int gnn_open_into(lmx_gnn* m, const char* path) {
  LMX_TRY(lmx_gnn_image_parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_gnn_open_host", path, m->img.data_offset, m->img.file_bytes));
  lmx_gnn_bind(m->img, m->weights, &m->w);
  return lmx_gnn_check_config("lmx_gnn_open_host", &m->w, true);
}

// the handle's own limits on top of the checks of every forward; *nodes = sum N, *edges = sum E
int gnn_check_call(const lmx_gnn* m, const char* fn, const lmx_gnn_graphs_t* g, const uint64_t* seeds, int S, const void* node_mc, const void* stats,
                   const void* graph_pred, const void* node_pred, const void* attw, int64_t* nodes, int64_t* edges) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(g != nullptr, "%s: null graphs", fn);
  LMX_REQUIRE(g->n > 0 && g->n <= m->max_batch, "%s: n = %d graphs, the handle was opened for 1 .. %d", fn, g->n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  int max_n = 0, max_e = 0;
  LMX_TRY(lmx_gnn_check_call(fn, &m->w, g, S, m->img.p, node_mc || stats, graph_pred || node_pred || attw, nodes, &max_n, &max_e));
  LMX_REQUIRE(S > 0 ? (node_mc && stats && seeds) : (graph_pred && node_pred && attw), "%s: an output of S = %d, or the seeds, is null", fn, S);
  *edges = g->edge_off_host[g->n];
  LMX_REQUIRE(*nodes <= m->max_nodes_total, "%s: %lld nodes in all, the handle was opened for up to %d", fn, (long long)*nodes, m->max_nodes_total);
  LMX_REQUIRE(*edges <= m->max_edges_total, "%s: %lld edges in all, the handle was opened for up to %d", fn, (long long)*edges, m->max_edges_total);
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_gnn_open_host(const char* path_host, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, lmx_gnn** out_host) {
  const char* fn = "lmx_gnn_open_host";
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", fn);
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "%s: max_samples %d outside 2 .. 65535", fn, max_samples);
  LMX_REQUIRE(max_nodes_total >= 1 && max_nodes_total <= (1 << 22), "%s: max_nodes_total %d outside 1 .. %d", fn, max_nodes_total, 1 << 22);
  LMX_REQUIRE(max_edges_total >= 0 && max_edges_total <= (1 << 25), "%s: max_edges_total %d outside 0 .. %d", fn, max_edges_total, 1 << 25);
  LMX_TRY(lmx_handle_open(fn, path_host, max_graphs, out_host, gnn_open_into, gnn_destroy));
  lmx_gnn* m = *out_host;
  m->max_samples = max_samples;
  m->max_nodes_total = max_nodes_total;
  m->max_edges_total = max_edges_total;
  const int mn = max_nodes_total < LMX_GNN_MAX_NODES ? max_nodes_total : LMX_GNN_MAX_NODES;
  const int me = max_edges_total < LMX_GNN_MAX_EDGES ? max_edges_total : LMX_GNN_MAX_EDGES;
  const int64_t bytes = lmx_gnn_workspace_bytes(max_graphs, max_samples, mn, me, m->w.d_model, m->w.n_layers);
  if (hipMalloc(reinterpret_cast<void**>(&m->ws), (size_t)bytes) != hipSuccess) {
    lmx_handle_close(m, gnn_destroy);
    *out_host = nullptr;
    lmx_set_error("%s: no memory for a workspace of %lld bytes", fn, (long long)bytes);
    return LMX_EINVAL;
  }
  return LMX_OK;
}

extern "C" void lmx_gnn_close(lmx_gnn* m) { lmx_handle_close(m, gnn_destroy); }

extern "C" int lmx_gnn_info(const lmx_gnn* m, lmx_gnn_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_gnn_info: null argument");
  lmx_gnn_fill_info(m->img, m->max_batch, m->max_nodes_total, m->max_edges_total, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_gnn_score(lmx_gnn* m, const lmx_gnn_graphs_t* graphs_host, const uint64_t* seeds_host, int S, float* node_mc, float* stats,
                             float* graph_pred, float* node_pred, float* attn_weights, lmx_stream_t stream) {
  const char* fn = "lmx_gnn_score";
  int64_t nodes = 0, edges = 0;
  LMX_TRY(gnn_check_call(m, fn, graphs_host, seeds_host, S, node_mc, stats, graph_pred, node_pred, attn_weights, &nodes, &edges));
  LMX_TRY(lmx_handle_stream_on_device(m, fn, reinterpret_cast<hipStream_t>(stream)));
  return lmx_k_gnn_forward(&m->w, graphs_host, seeds_host, S, m->img.p, node_mc, stats, graph_pred, node_pred, attn_weights, nullptr, m->ws, stream);
}

// upload the arrays that are there, run, download the outputs of the mode, synchronise
extern "C" int lmx_gnn_score_host(lmx_gnn* m, const lmx_gnn_graphs_t* g, const uint64_t* seeds_host, int S, float* node_mc_host, float* stats_host,
                                  float* graph_pred_host, float* node_pred_host, float* attn_host) {
  const char* fn = "lmx_gnn_score_host";
  int64_t nodes = 0, edges = 0;
  LMX_TRY(gnn_check_call(m, fn, g, seeds_host, S, node_mc_host, stats_host, graph_pred_host, node_pred_host, attn_host, &nodes, &edges));
  const int n = g->n;
  LMX_REQUIRE(g->x && g->lap && g->rw && g->csr_ptr && g->deg && (edges == 0 || (g->edge_src && g->edge_dst && g->edge_attr && g->csr_edge)),
              "%s: null pointer", fn);
  // staging: the graph arrays, then the outputs, each on a 256-byte boundary; an array that is not there takes no bytes
  const size_t E = (size_t)edges, N = (size_t)nodes;
  const size_t in_bytes[9] = {N * m->w.input_dim * 4, N * LMX_GNN_LAP_K * 4, N * LMX_GNN_RW_K * 4, E * 4, E * 4, E * 12, (N + n) * 4, E * 4, N * 4};
  const void* in_src[9] = {g->x, g->lap, g->rw, g->edge_src, g->edge_dst, g->edge_attr, g->csr_ptr, g->csr_edge, g->deg};
  const size_t out_bytes[5] = {S ? N * S * 4 : 0, S ? N * 8 : 0, S ? 0 : (size_t)n * 4, S ? 0 : N * 4, S ? 0 : N * 4};
  void* out_dst[5] = {node_mc_host, stats_host, graph_pred_host, node_pred_host, attn_host};
  LmxLayout lay;
  size_t in_at[9], out_at[5];
  for (int i = 0; i < 9; ++i) in_at[i] = lay.add(in_bytes[i]);
  for (int i = 0; i < 5; ++i) out_at[i] = lay.add(out_bytes[i]);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  void* in_dev[9];
  for (int i = 0; i < 9; ++i) {
    in_dev[i] = in_bytes[i] ? m->stage + in_at[i] : nullptr;
    if (in_bytes[i]) LMX_HIP(hipMemcpyAsync(in_dev[i], in_src[i], in_bytes[i], hipMemcpyHostToDevice, m->own));
  }
  float* out_dev[5];
  for (int i = 0; i < 5; ++i) out_dev[i] = out_bytes[i] ? reinterpret_cast<float*>(m->stage + out_at[i]) : nullptr;
  lmx_gnn_graphs_t d = *g;
  d.x = static_cast<const float*>(in_dev[0]), d.lap = static_cast<const float*>(in_dev[1]), d.rw = static_cast<const float*>(in_dev[2]);
  d.edge_src = static_cast<const int32_t*>(in_dev[3]), d.edge_dst = static_cast<const int32_t*>(in_dev[4]);
  d.edge_attr = static_cast<const float*>(in_dev[5]), d.csr_ptr = static_cast<const int32_t*>(in_dev[6]);
  d.csr_edge = static_cast<const int32_t*>(in_dev[7]), d.deg = static_cast<const int32_t*>(in_dev[8]);
  LMX_TRY(lmx_k_gnn_forward(&m->w, &d, seeds_host, S, m->img.p, out_dev[0], out_dev[1], out_dev[2], out_dev[3], out_dev[4], nullptr, m->ws, m->own));
  for (int i = 0; i < 5; ++i)
    if (out_bytes[i]) LMX_HIP(hipMemcpyAsync(out_dst[i], out_dev[i], out_bytes[i], hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}
