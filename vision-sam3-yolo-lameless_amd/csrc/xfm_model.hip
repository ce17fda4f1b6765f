// xfm_model.hip — the model-level entry points of the C-ABI for the gait transformer: a handle (model_handle.h has what every handle
// owns) with the weights of one weight image (xfm_image.h) and the seed workspace of max_clips clips, and lmx_xfm_score, which is
// lmx_k_xfm_forward (xfm.hip) with the image's configuration and dropout probability
// (services/transformer-pipeline/app/main.py:421-441).  HOST code only: there is no kernel in this file.
#include "model_handle.h"
#include "xfm_image.h"

struct lmx_xfm : LmxHandleCore {
  LmxXfmImage img;
  lmx_xfm_weights_t w;       // device pointers into `weights`
  int max_samples = 0;
  char* seeds = nullptr;     // lmx_xfm_workspace_bytes(max_clips)
};

namespace {

void destroy(lmx_xfm* m) {
  (void)hipFree(m->seeds);
  lmx_handle_free(m);
  delete m;
}

int open_into(lmx_xfm* m, const char* path) {
  LMX_TRY(lmx_xfm_image_parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_xfm_open_host", path, m->img.data_offset, m->img.file_bytes));
  lmx_xfm_bind(m->img, m->weights, &m->w);
  LMX_TRY(lmx_xfm_check_config("lmx_xfm_open_host", &m->w, true));
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->seeds), (size_t)lmx_xfm_workspace_bytes(m->max_batch)));
  return LMX_OK;
}

int check_call(const lmx_xfm* m, const char* fn, const void* x, const uint64_t* seeds, int n, int T, int S, const void* pred, const void* stats,
               const void* saliency) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0 && n <= m->max_batch, "%s: n = %d clips, the handle was opened for 1 .. %d", fn, n, m->max_batch);
  LMX_REQUIRE(S >= 0 && S <= m->max_samples, "%s: S = %d samples, the handle was opened for up to %d", fn, S, m->max_samples);
  LMX_REQUIRE(x && pred && stats && (seeds || S == 0), "%s: null pointer", fn);
  return lmx_xfm_check_call(fn, &m->w, n, T, S, m->img.p, saliency != nullptr);
}

}  // namespace

extern "C" int lmx_xfm_open_host(const char* path_host, int max_clips, int max_samples, lmx_xfm** out_host) {
  LMX_REQUIRE(out_host != nullptr, "lmx_xfm_open_host: out_host is null");
  *out_host = nullptr;
  LMX_REQUIRE(max_samples >= 2 && max_samples <= 65535, "lmx_xfm_open_host: max_samples %d outside 2 .. 65535", max_samples);
  LMX_TRY(lmx_handle_open("lmx_xfm_open_host", path_host, max_clips, out_host, open_into, destroy));
  (*out_host)->max_samples = max_samples;
  return LMX_OK;
}

extern "C" void lmx_xfm_close(lmx_xfm* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_xfm_info(const lmx_xfm* m, lmx_xfm_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_xfm_info: null argument");
  lmx_xfm_fill_info(m->img, m->max_batch, m->max_samples, info_host);
  return LMX_OK;
}

extern "C" int lmx_xfm_score(lmx_xfm* m, const float* x, const uint8_t* mask, const uint64_t* seeds_host, int n, int T, int S, float* pred,
                             float* stats, float* saliency, lmx_stream_t stream) {
  LMX_TRY(check_call(m, "lmx_xfm_score", x, seeds_host, n, T, S, pred, stats, saliency));
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_xfm_score", reinterpret_cast<hipStream_t>(stream)));
  return lmx_k_xfm_forward(&m->w, x, mask, seeds_host, n, T, S, m->img.p, pred, stats, saliency, nullptr, m->seeds, stream);
}

extern "C" int lmx_xfm_score_host(lmx_xfm* m, const float* x_host, const uint8_t* mask_host, const uint64_t* seeds_host, int n, int T, int S,
                                  float* pred_host, float* stats_host, float* saliency_host) {
  LMX_TRY(check_call(m, "lmx_xfm_score_host", x_host, seeds_host, n, T, S, pred_host, stats_host, saliency_host));
  // staging: series | mask | predictions | stats | saliency, each on a 256-byte boundary
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
  LMX_TRY(lmx_k_xfm_forward(&m->w, x, mask, seeds_host, n, T, S, m->img.p, pred, stats, sal, nullptr, m->seeds, m->own));
  LMX_HIP(hipMemcpyAsync(pred_host, pred, pred_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipMemcpyAsync(stats_host, stats, stats_bytes, hipMemcpyDeviceToHost, m->own));
  if (sal) LMX_HIP(hipMemcpyAsync(saliency_host, sal, sal_bytes, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}
