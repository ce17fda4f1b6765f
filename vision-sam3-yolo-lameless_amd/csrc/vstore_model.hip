// vstore_model.hip — lmx_vstore: a gallery of f32 unit rows in HBM behind a handle for C callers (include/lmx.h, "Vector store").
// The handle maps nothing but slots: row `slot` of one [capacity][dim] allocation; ids and payloads belong to the caller.  It follows
// the device-check and own-stream protocol of model_handle.h; there is no weight image, so it takes only what applies.  Rows enter
// through lmx_h_unit_rows (put_host) or lmx_k_unit_rows (append), which agree bit for bit, and searches are lmx_k_cosine_topk.
#include <vector>

#include "model_handle.h"
#include "vstore.h"

struct lmx_vstore : LmxHandleCore {
  int dim = 0;
  int64_t capacity = 0, count = 0;
  float* gallery = nullptr;  // [capacity][dim]
  // a search's unit queries and its lmx_k_cosine_topk workspace (grown on demand, synchronously)
  char* scratch = nullptr;
  size_t scratch_bytes = 0;
};

namespace {

void vstore_destroy(lmx_vstore* m) {
  (void)hipFree(m->gallery);
  (void)hipFree(m->scratch);
  lmx_handle_free(m);
  delete m;
}

// room for `need` rows: the gallery doubles until it fits.  Synchronous: the old allocation is idle before it is freed
int vstore_reserve(lmx_vstore* m, int64_t need) {
  if (need <= m->capacity) return LMX_OK;
  LMX_REQUIRE(need <= INT32_MAX, "lmx_vstore: %lld rows are more than 2^31 - 1", (long long)need);
  int64_t cap = m->capacity;
  while (cap < need) cap = cap * 2 < INT32_MAX ? cap * 2 : INT32_MAX;
  float* g = nullptr;
  LMX_HIP(hipDeviceSynchronize());
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&g), (size_t)cap * m->dim * sizeof(float)));
  hipError_t e = m->count ? hipMemcpy(g, m->gallery, (size_t)m->count * m->dim * sizeof(float), hipMemcpyDeviceToDevice) : hipSuccess;
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(g);
    LMX_HIP(e);
  }
  (void)hipFree(m->gallery);
  m->gallery = g;
  m->capacity = cap;
  return LMX_OK;
}

int vstore_scratch(lmx_vstore* m, size_t need) {
  if (need <= m->scratch_bytes) return LMX_OK;
  LMX_HIP(hipDeviceSynchronize());
  (void)hipFree(m->scratch);
  m->scratch = nullptr;
  m->scratch_bytes = 0;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->scratch), need));
  m->scratch_bytes = need;
  return LMX_OK;
}

int vstore_check_search(const lmx_vstore* m, const char* fn, const void* raw, int dtype, int Q, int k, const void* scores, const void* slots) {
  LMX_REQUIRE(dtype == LMX_VSTORE_F32 || dtype == LMX_VSTORE_F64, "%s: dtype %d is neither LMX_VSTORE_F32 nor LMX_VSTORE_F64", fn, dtype);
  LMX_REQUIRE(k >= 1 && k <= LMX_VSTORE_MAX_K, "%s: k = %d outside 1 .. %d", fn, k, LMX_VSTORE_MAX_K);
  LMX_REQUIRE(Q >= 0 && Q <= LMX_VSTORE_MAX_Q, "%s: Q = %d queries (0 .. %d)", fn, Q, LMX_VSTORE_MAX_Q);
  LMX_REQUIRE(Q == 0 || (raw && scores && slots), "%s: null pointer (%s)", fn, !raw ? "queries" : !scores ? "scores" : "slots");
  return LMX_OK;
}

// unit queries at the head of the scratch blob, the workspace behind them
int vstore_search_on(lmx_vstore* m, const void* raw_dev, int dtype, int Q, const int32_t* limits_dev, int k, float* scores_dev, int32_t* slots_dev,
                     hipStream_t st) {
  const size_t q_bytes = up256((size_t)Q * m->dim * sizeof(float));
  LMX_TRY(vstore_scratch(m, q_bytes + (size_t)lmx_h_cosine_topk_workspace(m->count, Q, k)));
  float* unit = reinterpret_cast<float*>(m->scratch);
  LMX_TRY(lmx_k_unit_rows(raw_dev, dtype, Q, m->dim, unit, m->dim, st));
  return lmx_k_cosine_topk(m->gallery, m->count, m->dim, m->dim, unit, Q, limits_dev, k, scores_dev, slots_dev, m->scratch + q_bytes, st);
}

}  // namespace

extern "C" int lmx_vstore_open(int dim, int64_t capacity, lmx_vstore** out_host) {
  LMX_REQUIRE(out_host != nullptr, "lmx_vstore_open: out_host is null");
  *out_host = nullptr;
  LMX_TRY(lmx_vstore_check_dim("lmx_vstore_open", dim));
  LMX_REQUIRE(capacity >= 1 && capacity <= INT32_MAX, "lmx_vstore_open: capacity %lld outside 1 .. 2^31 - 1", (long long)capacity);
  lmx_vstore* m = new lmx_vstore();
  m->dim = dim;
  m->capacity = capacity;
  int rc = LMX_OK;
  if (hipGetDevice(&m->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&m->gallery), (size_t)capacity * dim * sizeof(float)) != hipSuccess) {
    lmx_set_error("lmx_vstore_open: no device, or no room for %lld x %d floats", (long long)capacity, dim);
    rc = LMX_EHIP;
  }
  if (rc == LMX_OK) rc = lmx_handle_finish_open(m);
  if (rc != LMX_OK) {
    vstore_destroy(m);
    return rc;
  }
  *out_host = m;
  return LMX_OK;
}

extern "C" void lmx_vstore_close(lmx_vstore* m) { lmx_handle_close(m, vstore_destroy); }

extern "C" int64_t lmx_vstore_count(const lmx_vstore* m) { return m ? m->count : 0; }

extern "C" int lmx_vstore_gallery(const lmx_vstore* m, const float** gallery, int64_t* ldg_host) {
  LMX_REQUIRE(m && gallery && ldg_host, "lmx_vstore_gallery: null pointer");
  *gallery = m->gallery;
  *ldg_host = m->dim;
  return LMX_OK;
}

extern "C" int lmx_vstore_put_host(lmx_vstore* m, int64_t slot, const void* raw_host, int dtype) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_put_host"));
  LMX_REQUIRE(slot >= 0 && slot <= m->count, "lmx_vstore_put_host: slot %lld is neither a stored row nor the next one (%lld stored)", (long long)slot,
              (long long)m->count);
  std::vector<float> unit((size_t)m->dim);
  LMX_TRY(lmx_h_unit_rows(raw_host, dtype, 1, m->dim, unit.data(), m->dim));
  LMX_TRY(vstore_reserve(m, slot + 1));
  LMX_HIP(hipStreamSynchronize(m->own));
  LMX_HIP(hipMemcpy(m->gallery + slot * m->dim, unit.data(), (size_t)m->dim * sizeof(float), hipMemcpyHostToDevice));
  if (slot == m->count) m->count += 1;
  return LMX_OK;
}

extern "C" int lmx_vstore_append(lmx_vstore* m, const void* raw_rows, int dtype, int64_t n) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_append"));
  LMX_TRY(lmx_vstore_check_unit("lmx_vstore_append", raw_rows, dtype, n, m->dim, m->gallery, m->dim));
  if (n == 0) return LMX_OK;
  LMX_TRY(vstore_reserve(m, m->count + n));
  LMX_HIP(hipDeviceSynchronize());  // the rows are the caller's, written on a stream of the caller's
  LMX_TRY(lmx_k_unit_rows(raw_rows, dtype, n, m->dim, m->gallery + m->count * m->dim, m->dim, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  m->count += n;
  return LMX_OK;
}

extern "C" int lmx_vstore_get_host(lmx_vstore* m, int64_t slot, float* out_host) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_get_host"));
  LMX_REQUIRE(slot >= 0 && slot < m->count, "lmx_vstore_get_host: slot %lld of %lld stored", (long long)slot, (long long)m->count);
  LMX_REQUIRE(out_host != nullptr, "lmx_vstore_get_host: out_host is null");
  LMX_HIP(hipMemcpy(out_host, m->gallery + slot * m->dim, (size_t)m->dim * sizeof(float), hipMemcpyDeviceToHost));
  return LMX_OK;
}

extern "C" int lmx_vstore_read_host(lmx_vstore* m, int64_t first, int64_t n, float* out_host) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_read_host"));
  LMX_REQUIRE(first >= 0 && n >= 0 && first + n <= m->count, "lmx_vstore_read_host: rows %lld .. %lld of %lld stored", (long long)first,
              (long long)(first + n), (long long)m->count);
  LMX_REQUIRE(n == 0 || out_host != nullptr, "lmx_vstore_read_host: out_host is null");
  if (n) LMX_HIP(hipMemcpy(out_host, m->gallery + first * m->dim, (size_t)n * m->dim * sizeof(float), hipMemcpyDeviceToHost));
  return LMX_OK;
}

extern "C" int lmx_vstore_restore_host(lmx_vstore* m, const float* unit_rows_host, int64_t n) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_restore_host"));
  LMX_REQUIRE(n >= 0 && (n == 0 || unit_rows_host != nullptr), "lmx_vstore_restore_host: n = %lld rows, rows %s", (long long)n,
              unit_rows_host ? "given" : "null");
  if (n == 0) return LMX_OK;
  LMX_TRY(vstore_reserve(m, m->count + n));
  LMX_HIP(hipStreamSynchronize(m->own));
  LMX_HIP(hipMemcpy(m->gallery + m->count * m->dim, unit_rows_host, (size_t)n * m->dim * sizeof(float), hipMemcpyHostToDevice));
  m->count += n;
  return LMX_OK;
}

extern "C" int lmx_vstore_search(lmx_vstore* m, const void* raw_queries, int dtype, int Q, const int32_t* limits, int k, float* scores, int32_t* slots,
                                 lmx_stream_t stream) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_search"));
  LMX_TRY(vstore_check_search(m, "lmx_vstore_search", raw_queries, dtype, Q, k, scores, slots));
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_vstore_search", (hipStream_t)stream));
  if (Q == 0) return LMX_OK;
  return vstore_search_on(m, raw_queries, dtype, Q, limits, k, scores, slots, (hipStream_t)stream);
}

extern "C" int lmx_vstore_search_host(lmx_vstore* m, const void* raw_queries_host, int dtype, int Q, const int32_t* limits_host, int k, float* scores_host,
                                      int32_t* slots_host) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_vstore_search_host"));
  LMX_TRY(vstore_check_search(m, "lmx_vstore_search_host", raw_queries_host, dtype, Q, k, scores_host, slots_host));
  if (Q == 0) return LMX_OK;
  LmxLayout lay;
  const size_t raw_bytes = (size_t)Q * m->dim * (dtype == LMX_VSTORE_F64 ? 8 : 4);
  const size_t at_raw = lay.add(raw_bytes), at_lim = lay.add((size_t)Q * 4), at_s = lay.add((size_t)Q * k * 4), at_i = lay.add((size_t)Q * k * 4);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  LMX_HIP(hipMemcpyAsync(m->stage + at_raw, raw_queries_host, raw_bytes, hipMemcpyHostToDevice, m->own));
  if (limits_host) LMX_HIP(hipMemcpyAsync(m->stage + at_lim, limits_host, (size_t)Q * 4, hipMemcpyHostToDevice, m->own));
  LMX_TRY(vstore_search_on(m, m->stage + at_raw, dtype, Q, limits_host ? reinterpret_cast<const int32_t*>(m->stage + at_lim) : nullptr, k,
                           reinterpret_cast<float*>(m->stage + at_s), reinterpret_cast<int32_t*>(m->stage + at_i), m->own));
  LMX_HIP(hipMemcpyAsync(scores_host, m->stage + at_s, (size_t)Q * k * 4, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipMemcpyAsync(slots_host, m->stage + at_i, (size_t)Q * k * 4, hipMemcpyDeviceToHost, m->own));
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}
