// host_records.cpp — the host arithmetic of the fused per-frame record (include/lmx.h, "HOST functions: the fused record"): the C++
// twins of lmx.dist.record_layout over the dict FusedExtractor.step returns, of lmx.pipeline.stream_plan, and of the index_copy_ /
// index_fill_ row scatter of FusedExtractor.step's reference schedule, written as the row map lmx_k_pack_records gathers through.
// HOST code only, integers only, no HIP: compiled by g++ into the library and, with tests/fused_check_main.cpp, into a stand-alone
// program that runs under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_fused_sanitized.py).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);

#define REQUIRE(cond, ...)        \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

namespace {

struct FieldSpec {
  const char* name;
  int dtype, ndim;
  int64_t shape[2];
};

int64_t elem_bytes(int dtype) { return dtype == LMX_REC_U8 ? 1 : dtype == LMX_REC_I64 ? 8 : 4; }

}  // namespace

extern "C" int lmx_h_record_layout(int h, int w, int hidden, int max_det, int scheduled, lmx_record_layout_t* out_host) {
  REQUIRE(out_host != nullptr, "lmx_h_record_layout: out_host is null");
  REQUIRE(h > 0 && w > 0, "lmx_h_record_layout: frame size %d x %d", h, w);
  REQUIRE(hidden > 0, "lmx_h_record_layout: hidden = %d", hidden);
  REQUIRE(max_det > 0, "lmx_h_record_layout: max_det = %d", max_det);
  // the step's dict in sorted name order (lmx.dist.record_layout sorts; strcmp order of these ASCII names is Python's)
  const FieldSpec all[] = {
      {"boxes", LMX_REC_F32, 2, {max_det, 4}},
      {"cls", LMX_REC_I32, 1, {max_det, 0}},
      {"counts", LMX_REC_I32, 0, {0, 0}},
      {"embedding", LMX_REC_F32, 1, {hidden, 0}},
      {"mask_bits", LMX_REC_U8, 2, {h, ((int64_t)w + 7) / 8}},
      {"mask_contour", LMX_REC_I64, 1, {8, 0}},
      {"mask_iou", LMX_REC_F32, 0, {0, 0}},
      {"mask_stats", LMX_REC_I64, 1, {8, 0}},
      {"ran_det", LMX_REC_I32, 0, {0, 0}},
      {"ran_emb", LMX_REC_I32, 0, {0, 0}},
      {"scores", LMX_REC_F32, 1, {max_det, 0}},
  };
  memset(out_host, 0, sizeof(*out_host));
  int64_t off = 8;  // bytes 0..7: the int64 `valid` word
  int nf = 0;
  for (const FieldSpec& f : all) {
    if (!scheduled && strncmp(f.name, "ran_", 4) == 0) continue;
    lmx_record_field_layout_t& o = out_host->fields[nf++];
    snprintf(o.name, sizeof(o.name), "%s", f.name);
    o.dtype = f.dtype;
    o.ndim = f.ndim;
    int64_t nb = elem_bytes(f.dtype);
    for (int d = 0; d < f.ndim; ++d) {
      o.shape[d] = f.shape[d];
      nb *= f.shape[d];
    }
    o.offset = off;
    o.nbytes = nb;
    off += (nb + 7) / 8 * 8;
  }
  out_host->n_fields = nf;
  out_host->stride = off;
  return LMX_OK;
}

extern "C" int lmx_h_stream_plan(int n_chunks, int max_streams, int layout, int* pool_host, int* det_host, int* emb_host, int32_t* sam_host) {
  REQUIRE(layout == LMX_STREAMS_LANES || layout == LMX_STREAMS_RR, "lmx_h_stream_plan: layout %d is neither LMX_STREAMS_LANES (0) nor LMX_STREAMS_RR (1)",
          layout);
  REQUIRE(n_chunks >= 0, "lmx_h_stream_plan: n_chunks = %d", n_chunks);
  REQUIRE(pool_host && det_host && emb_host, "lmx_h_stream_plan: null pointer");
  REQUIRE(n_chunks == 0 || sam_host != nullptr, "lmx_h_stream_plan: null pointer (sam_host)");
  // k = max(3, min(2 + n_chunks, max_streams)), in 64 bits: 2 + n_chunks must not wrap
  int64_t k = (int64_t)n_chunks + 2;
  if (k > max_streams) k = max_streams;
  if (k < 3) k = 3;
  *pool_host = (int)k;
  *det_host = 0;
  *emb_host = 1;
  for (int j = 0; j < n_chunks; ++j) sam_host[j] = layout == LMX_STREAMS_RR ? (int32_t)((2 + (int64_t)j) % k) : (int32_t)(2 + j % (k - 2));
  return LMX_OK;
}

extern "C" int lmx_h_row_map(int n, const int32_t* idx_host, int n_idx, const char* what, int32_t* map_host, int32_t* ran_host) {
  const char* name = what ? what : "idx";
  REQUIRE(n >= 0, "lmx_h_row_map: n = %d rows", n);
  REQUIRE(n_idx >= 0 && n_idx <= n, "lmx_h_row_map: %s names %d frames of %d", name, n_idx, n);
  REQUIRE(n_idx == 0 || idx_host != nullptr, "lmx_h_row_map: null pointer (%s)", name);
  REQUIRE(n == 0 || map_host != nullptr, "lmx_h_row_map: null pointer (map_host)");
  for (int j = 0; j < n_idx; ++j) {
    const int32_t i = idx_host[j];
    REQUIRE(i >= 0 && i < n, "lmx_h_row_map: %s[%d] = %d outside 0 .. %d", name, j, (int)i, n - 1);
    REQUIRE(j == 0 || i != idx_host[j - 1], "lmx_h_row_map: %s[%d] = %d repeats %s[%d]", name, j, (int)i, name, j - 1);
    REQUIRE(j == 0 || i > idx_host[j - 1], "lmx_h_row_map: %s[%d] = %d after %s[%d] = %d: the indices must ascend", name, j, (int)i, name, j - 1,
            (int)idx_host[j - 1]);
  }
  for (int r = 0; r < n; ++r) {
    map_host[r] = -1;
    if (ran_host) ran_host[r] = 0;
  }
  for (int j = 0; j < n_idx; ++j) {
    map_host[idx_host[j]] = j;
    if (ran_host) ran_host[idx_host[j]] = 1;
  }
  return LMX_OK;
}
