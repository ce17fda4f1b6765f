// hiera_bands.h — the arithmetic of lmx_h_hiera_bands (include/lmx.h), shared by the entry point (sam.hip, which validates the
// arguments) and the block plan (host_hiera_plan.cpp).  Host code only: nothing here needs HIP.
#pragma once
#include <stdint.h>

// `d` rows of the grid block i reads carry a pixel's influence; the block runs on the whole windows (and whole pooled pairs) that
// cover them and hands those rows on, halved where it pools.  Arguments already validated: n_blocks > 0, grid > 0, window[i] >= 0,
// q_stride[i] in {0, 1, 2}.
inline void lmx_hiera_bands_rows(const int* window, const int* q_stride, int n_blocks, int grid, int nh, int nw, int* rows) {
  int first_global = -1;
  for (int i = 0; i < n_blocks; ++i)
    if (window[i] == 0 && first_global < 0) first_global = i;
  // padding on the right, block 0 global, or no global block: no band (lmx_h_hiera_band's cases of 0)
  const bool whole = nw < 4 * grid || first_global <= 0;
  int64_t g = grid;                                         // rows of the grid block i reads
  int64_t d = (nh + 2) / 4 + 1 < g ? (nh + 2) / 4 + 1 : g;  // token row r reads pixel rows 4 r - 3 .. 4 r + 3
  for (int i = 0; i < n_blocks; ++i) {
    const bool pools = q_stride[i] == 2;
    if (whole || i >= first_global) {
      d = g;
    } else {
      const int64_t piece = window[i] % 2 == 0 || !pools ? window[i] : 2 * (int64_t)window[i];  // whole windows, an even count where it pools
      d = (d + piece - 1) / piece * piece;
      if (d >= g) d = g;
    }
    rows[i] = (int)d;
    if (pools) {
      d /= 2;
      g /= 2;
    }
  }
}
