// host_vstore.cpp — HOST restatement of csrc/vstore.hip: the pinned dot product, the total order of (score, slot) pairs and the unit
// rows, one element at a time, straight from the text at lmx_k_cosine_topk in include/lmx.h.  The device is held to it bit for bit
// (tests/test_gpu_vstore.py); it is held to float64 without a GPU (tests/test_vstore_host.py).  Compiled with -ffp-contract=off: its
// only fused multiply-adds are its fmaf / fma calls.
#include <math.h>
#include <stdint.h>

#include "vstore.h"

namespace {

// 256 partials: partial j takes elements j, j + 256, ... in ascending order by fmaf from +0, then p[j] += p[j + w], w = 128 .. 1
inline float pinned_dot(const float* g, const float* q, int D) {
  float p[256];
  for (int j = 0; j < 256; ++j) p[j] = 0.0f;
  for (int i = 0; i < D; ++i) p[i & 255] = fmaf(g[i], q[i], p[i & 255]);
  for (int w = 128; w >= 1; w >>= 1)
    for (int j = 0; j < w; ++j) p[j] = p[j] + p[j + w];
  return p[0];
}

template <class X>
inline double pinned_sumsq(const X* x, int D) {
  double p[256];
  for (int j = 0; j < 256; ++j) p[j] = 0.0;
  for (int i = 0; i < D; ++i) p[i & 255] = fma((double)x[i], (double)x[i], p[i & 255]);
  for (int w = 128; w >= 1; w >>= 1)
    for (int j = 0; j < w; ++j) p[j] = p[j] + p[j + w];
  return p[0];
}

template <class X>
inline void unit_row(const X* x, int D, float* out) {
  const double den = sqrt(pinned_sumsq(x, D)) + 1e-8;
  for (int i = 0; i < D; ++i) out[i] = (float)((double)x[i] / den);
}

// descending score, compared as float values; exact ties to the lower slot
inline bool better(float sa, int32_t ia, float sb, int32_t ib) { return sa > sb || (sa == sb && ia < ib); }

}  // namespace

extern "C" int64_t lmx_h_cosine_topk_workspace(int64_t N, int Q, int k) {
  if (N < 0 || Q < 0 || k < 1) return 0;
  return lmx_vstore_lists(N) * (int64_t)Q * k * 8;
}

extern "C" int lmx_h_cosine_topk_geometry(int D, int* rows_host, int* tile_host, int* wg_per_cu_host) {
  if (const int rc = lmx_vstore_check_dim("lmx_h_cosine_topk_geometry", D)) return rc;
  LMX_VSTORE_REQUIRE(rows_host && tile_host && wg_per_cu_host, "lmx_h_cosine_topk_geometry: null pointer");
  *rows_host = LMX_VSTORE_ROWS;
  *tile_host = lmx_vstore_tile(D);
  *wg_per_cu_host = LMX_VSTORE_WG_PER_CU;
  return LMX_OK;
}

extern "C" int lmx_h_unit_rows(const void* raw_host, int dtype, int64_t n, int D, float* out_host, int64_t ldo) {
  if (const int rc = lmx_vstore_check_unit("lmx_h_unit_rows", raw_host, dtype, n, D, out_host, ldo)) return rc;
  for (int64_t r = 0; r < n; ++r) {
    if (dtype == LMX_VSTORE_F64)
      unit_row((const double*)raw_host + r * D, D, out_host + r * ldo);
    else
      unit_row((const float*)raw_host + r * D, D, out_host + r * ldo);
  }
  return LMX_OK;
}

extern "C" int lmx_h_cosine_topk(const float* gallery_host, int64_t N, int D, int64_t ldg, const float* queries_host, int Q,
                                 const int32_t* limits_host, int k, float* scores_host, int32_t* slots_host) {
  if (const int rc = lmx_vstore_check_topk("lmx_h_cosine_topk", gallery_host, N, D, ldg, queries_host, Q, k, scores_host, slots_host)) return rc;
  for (int q = 0; q < Q; ++q) {
    int64_t lim = limits_host ? limits_host[q] : N;
    lim = lim < 0 ? 0 : (lim > N ? N : lim);
    float bs[LMX_VSTORE_MAX_K];
    int32_t bi[LMX_VSTORE_MAX_K];
    int have = 0;
    for (int64_t r = 0; r < lim; ++r) {
      const float s = pinned_dot(gallery_host + r * ldg, queries_host + (int64_t)q * D, D);
      if (!(s == s)) continue;  // a NaN never ranks (the device's compares all fail for it too)
      if (have == k && !better(s, (int32_t)r, bs[k - 1], bi[k - 1])) continue;
      int at = have < k ? have++ : k - 1;
      for (; at > 0 && better(s, (int32_t)r, bs[at - 1], bi[at - 1]); --at) bs[at] = bs[at - 1], bi[at] = bi[at - 1];
      bs[at] = s, bi[at] = (int32_t)r;
    }
    for (int j = 0; j < k; ++j) {
      scores_host[(int64_t)q * k + j] = j < have ? bs[j] : 0.0f;
      slots_host[(int64_t)q * k + j] = j < have ? bi[j] : -1;
    }
  }
  return LMX_OK;
}
