// tcn_model.hip — the model-level entry points of the C-ABI for the TCN gait model: a handle (model_handle.h has what every handle
// owns) with the weights of one weight image (tcn_image.h) and the seed workspace of max_clips clips, and lmx_tcn_score, which is
// lmx_k_tcn_forward (tcn.hip) with the image's configuration and dropout probability (services/tcn-pipeline/app/main.py:357-364).
// HOST code only: there is no kernel in this file.
#include "model_handle.h"
#include "tcn_image.h"

struct lmx_tcn : LmxHandleCore {
  LmxTcnImage img;
  lmx_tcn_weights_t w;       // device pointers into `weights`
  int max_samples = 0;
  char* seeds = nullptr;     // lmx_tcn_workspace_bytes(max_clips)
};

namespace {

void destroy(lmx_tcn* m) {
  (void)hipFree(m->seeds);
  lmx_handle_free(m);
  delete m;
}

int open_into(lmx_tcn* m, const char* path) {
  LMX_TRY(lmx_tcn_image_parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_tcn_open_host", path, m->img.data_offset, m->img.file_bytes));
  lmx_tcn_bind(m->img, m->weights, &m->w);
  LMX_TRY(lmx_tcn_check_config("lmx_tcn_open_host", &m->w, true));
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->seeds), (size_t)lmx_tcn_workspace_bytes(m->max_batch)));
  return LMX_OK;
}

int check_call(const lmx_tcn* m, const char* fn, const void* x, const uint64_t* seeds, int n, int T, int S, const void* pred, const void* stats) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0 && n <= m->max_batch, "%s: n = %d clips, the handle was opened for 1 .. %d", fn, n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  LMX_REQUIRE(x && pred && stats && (seeds || S == 0), "%s: null pointer", fn);
  LMX_REQUIRE(T >= 1 && T <= LMX_TCN_MAX_T, "%s: T %d outside 1 .. %d", fn, T, LMX_TCN_MAX_T);
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_tcn_open_host(const char* path_host, int max_clips, int max_samples, lmx_tcn** out_host) {
  LMX_REQUIRE(out_host != nullptr, "lmx_tcn_open_host: out_host is null");
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "lmx_tcn_open_host: max_samples %d outside 2 .. 65535", max_samples);
  LMX_TRY(lmx_handle_open("lmx_tcn_open_host", path_host, max_clips, out_host, open_into, destroy));
  (*out_host)->max_samples = max_samples;
  return LMX_OK;
}

extern "C" void lmx_tcn_close(lmx_tcn* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_tcn_info(const lmx_tcn* m, lmx_tcn_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_tcn_info: null argument");
  lmx_tcn_fill_info(m->img, m->max_batch, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_tcn_score(lmx_tcn* m, const float* x, const uint64_t* seeds_host, int n, int T, int S, float* pred, float* stats,
                             lmx_stream_t stream) {
  LMX_TRY(check_call(m, "lmx_tcn_score", x, seeds_host, n, T, S, pred, stats));
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_tcn_score", reinterpret_cast<hipStream_t>(stream)));
  return lmx_k_tcn_forward(&m->w, x, seeds_host, n, T, S, m->img.p, pred, stats, nullptr, m->seeds, stream);
}

extern "C" int lmx_tcn_score_host(lmx_tcn* m, const float* x_host, const uint64_t* seeds_host, int n, int T, int S, float* pred_host,
                                  float* stats_host) {
  LMX_TRY(check_call(m, "lmx_tcn_score_host", x_host, seeds_host, n, T, S, pred_host, stats_host));
  // staging: series | predictions | stats, each on a 256-byte boundary
  const size_t x_bytes = (size_t)n * T * m->w.input_dim * sizeof(float), pred_bytes = (size_t)n * (S > 0 ? S : 1) * sizeof(float),
               stats_bytes = (size_t)n * 2 * sizeof(float);
  LmxLayout lay;
  const size_t o_x = lay.add(x_bytes), o_pred = lay.add(pred_bytes), o_stats = lay.add(stats_bytes);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  float* x = reinterpret_cast<float*>(m->stage + o_x);
  float* pred = reinterpret_cast<float*>(m->stage + o_pred);
  float* stats = reinterpret_cast<float*>(m->stage + o_stats);
  LMX_HIP(hipMemcpyAsync(x, x_host, x_bytes, hipMemcpyHostToDevice, m->own));
  LMX_TRY(lmx_k_tcn_forward(&m->w, x, seeds_host, n, T, S, m->img.p, pred, stats, nullptr, m->seeds, m->own));
  LMX_HIP(hipMemcpyAsync(pred_host, pred, pred_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipMemcpyAsync(stats_host, stats, stats_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}
