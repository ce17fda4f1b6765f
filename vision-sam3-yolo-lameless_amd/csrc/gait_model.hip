// gait_model.hip — the model-level entry points of the C-ABI for the two gait sequence models, the TCN (lmx_tcn_*) and the gait
// transformer (lmx_xfm_*): ONE handle (model_handle.h has what every handle owns) with the weights of one weight image (tcn_image.h,
// xfm_image.h) and the seed workspace of max_clips clips, and lmx_<model>_score, which is lmx_k_<model>_forward (tcn.hip, xfm.hip) with
// the image's configuration and dropout probability (services/tcn-pipeline/app/main.py:357-364,
// services/transformer-pipeline/app/main.py:421-441).  A model is a traits struct: its image, its weights, and how a call is checked
// and run.  The two graph models, whose calls take graphs and not series, have the same arrangement in graph_model.hip.  HOST code
// only: there is no kernel in this file.
#include "gait_launch.h"
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
