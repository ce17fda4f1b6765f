// vstore.h — what the device kernels (vstore.hip), their host restatement (host_vstore.cpp) and the handle (vstore_model.hip) of the
// vector store share: the launch geometry, the limits and the argument checks.  The arithmetic is the text at lmx_k_cosine_topk in
// include/lmx.h; each file writes it itself.  Plain C++, no HIP: host_vstore.cpp is compiled by g++.
#pragma once
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

// the scan kernel's geometry (lmx_h_cosine_topk_geometry hands these to lmx/vstore.py and to the tests).  None of them can change a
// result: a score is the pinned dot product and the order of (score, slot) pairs is total.
const int LMX_VSTORE_WAVES = 4;          // waves per workgroup
const int LMX_VSTORE_ROWS_PER_WAVE = 2;  // gallery rows a wave has in flight
const int LMX_VSTORE_ROWS = LMX_VSTORE_WAVES * LMX_VSTORE_ROWS_PER_WAVE;  // R: rows per workgroup pass
const int LMX_VSTORE_TILE = 8;           // T: queries that ride on one load of a gallery row, at the most (lmx_vstore_tile)
const int LMX_VSTORE_WG_PER_CU = 4;      // workgroups of the scan per CU ...
const int LMX_VSTORE_MAX_WG = 1024;      // ... and in all (sizes the workspace without asking a device)

const int LMX_VSTORE_MAX_DIM = 4096, LMX_VSTORE_MAX_K = 32, LMX_VSTORE_MAX_Q = 65535;

#define LMX_VSTORE_REQUIRE(cond, ...) \
  do {                                \
    if (!(cond)) {                    \
      lmx_set_error(__VA_ARGS__);     \
      return LMX_EINVAL;              \
    }                                 \
  } while (0)

inline int lmx_vstore_check_dim(const char* fn, int D) {
  LMX_VSTORE_REQUIRE(D >= 4 && D <= LMX_VSTORE_MAX_DIM && D % 4 == 0, "%s: D = %d is not a multiple of 4 in 4 .. %d", fn, D, LMX_VSTORE_MAX_DIM);
  return LMX_OK;
}

// queries of a tile at dimension D: the tile's rows take at most 32 KiB of LDS (8 up to D = 1024, 4 up to 2048, 2 above)
inline int lmx_vstore_tile(int D) {
  const int Dp = (D + 255) / 256 * 256, fit = 8192 / Dp;
  return fit < LMX_VSTORE_TILE ? fit : LMX_VSTORE_TILE;
}

// workgroups whose candidate lists the workspace holds per query
inline int64_t lmx_vstore_lists(int64_t N) {
  const int64_t need = (N + LMX_VSTORE_ROWS - 1) / LMX_VSTORE_ROWS;
  return need < LMX_VSTORE_MAX_WG ? need : LMX_VSTORE_MAX_WG;
}

// lmx_k_cosine_topk and lmx_h_cosine_topk (`fn`: the entry point's name); nothing is read, written or launched before these pass
inline int lmx_vstore_check_topk(const char* fn, const void* gallery, int64_t N, int D, int64_t ldg, const void* queries, int Q, int k,
                                 const void* scores, const void* slots) {
  if (const int rc = lmx_vstore_check_dim(fn, D)) return rc;
  LMX_VSTORE_REQUIRE(k >= 1 && k <= LMX_VSTORE_MAX_K, "%s: k = %d outside 1 .. %d", fn, k, LMX_VSTORE_MAX_K);
  LMX_VSTORE_REQUIRE(N >= 0 && N <= INT32_MAX, "%s: N = %lld rows (0 .. 2^31 - 1)", fn, (long long)N);
  LMX_VSTORE_REQUIRE(Q >= 0 && Q <= LMX_VSTORE_MAX_Q, "%s: Q = %d queries (0 .. %d)", fn, Q, LMX_VSTORE_MAX_Q);
  LMX_VSTORE_REQUIRE(ldg >= D && ldg % 4 == 0, "%s: ldg = %lld is not a multiple of 4 at or above D = %d", fn, (long long)ldg, D);
  LMX_VSTORE_REQUIRE(N == 0 || gallery != nullptr, "%s: null gallery with N = %lld", fn, (long long)N);
  LMX_VSTORE_REQUIRE(Q == 0 || (queries != nullptr && scores != nullptr && slots != nullptr), "%s: null pointer (%s)", fn,
                     !queries ? "queries" : !scores ? "scores" : "slots");
  LMX_VSTORE_REQUIRE((((uintptr_t)gallery | (uintptr_t)queries) & 15) == 0, "%s: gallery and queries must be 16-byte aligned", fn);
  return LMX_OK;
}

inline int lmx_vstore_check_unit(const char* fn, const void* raw, int dtype, int64_t n, int D, const void* out, int64_t ldo) {
  if (const int rc = lmx_vstore_check_dim(fn, D)) return rc;
  LMX_VSTORE_REQUIRE(dtype == LMX_VSTORE_F32 || dtype == LMX_VSTORE_F64, "%s: dtype %d is neither LMX_VSTORE_F32 nor LMX_VSTORE_F64", fn, dtype);
  LMX_VSTORE_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n = %lld rows (0 .. 2^31 - 1)", fn, (long long)n);
  LMX_VSTORE_REQUIRE(ldo >= D, "%s: ldo = %lld below D = %d", fn, (long long)ldo, D);
  LMX_VSTORE_REQUIRE(n == 0 || (raw != nullptr && out != nullptr), "%s: null pointer (%s)", fn, !raw ? "raw" : "out");
  return LMX_OK;
}
