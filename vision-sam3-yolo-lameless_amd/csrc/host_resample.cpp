// host_resample.cpp — HOST-side coefficient tables of the preprocessing kernels, the C++ twins of lmx/resample.py (which stays the
// restatement the tests pin against Pillow and torch; tests/test_native_dino_host.py holds these to its bits):
//   lmx_h_pil_tables   Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) in double, for
//                      lmx_k_pil_resize_h / _v                                                    = resample.coeff_tables
//   lmx_h_aa_tables    ATen's antialias weights (HelperInterpBase::_compute_indices_min_size_weights_aa, aten/src/ATen/native/cpu/
//                      UpSampleKernel.cpp) for a float32 tensor, EVERY step in float32 in ATen's order, for
//                      lmx_k_float_resize_patchify                                                = resample.aa_tables
// Built with -ffp-contract=off (csrc/Makefile): the only fused multiply-adds are the fmaf calls of the bicubic filter, the ones
// an FMA build of torch makes; nothing else may contract.
#include <math.h>
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define RS_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

namespace {

const int PRECISION_BITS = 32 - 8 - 2;

double pil_bilinear(double x) {
  x = fabs(x);
  return x < 1.0 ? 1.0 - x : 0.0;
}
double pil_bicubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

float aa_bilinear(float x) {
  x = fabsf(x);
  return x < 1.0f ? 1.0f - x : 0.0f;
}
// upsample_get_cubic_coefficients' two polynomials with A = -0.5, as an FMA build of torch evaluates them
float aa_bicubic(float x) {
  x = fabsf(x);
  if (x < 1.0f) return fmaf(fmaf(x, 1.5f, -2.5f) * x, x, 1.0f);
  if (x < 2.0f) return fmaf(fmaf(fmaf(x, -0.5f, 2.5f), x, -4.0f), x, 2.0f);
  return 0.0f;
}

int check_args(const char* fn, int in_size, int out_size, int filt, const void* bounds, const void* kk, int* ksize) {
  RS_REQUIRE(in_size > 0 && out_size > 0 && in_size <= (1 << 20) && out_size <= (1 << 20), "%s: in_size %d / out_size %d outside 1 .. 2^20", fn,
             in_size, out_size);
  RS_REQUIRE(filt == LMX_FILT_BILINEAR || filt == LMX_FILT_BICUBIC, "%s: filt %d is neither LMX_FILT_BILINEAR nor LMX_FILT_BICUBIC", fn, filt);
  RS_REQUIRE(ksize != nullptr && (bounds == nullptr) == (kk == nullptr), "%s: ksize_host is required; bounds_host and kk_host come together", fn);
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_h_pil_tables(int in_size, int out_size, int filt, int32_t* bounds_host, int32_t* kk_host, int64_t cap, int* ksize_host) {
  if (const int rc = check_args("lmx_h_pil_tables", in_size, out_size, filt, bounds_host, kk_host, ksize_host)) return rc;
  double (*const fn)(double) = filt == LMX_FILT_BILINEAR ? pil_bilinear : pil_bicubic;
  const double fsupport = filt == LMX_FILT_BILINEAR ? 1.0 : 2.0;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = fsupport * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  *ksize_host = ksize;
  if (!bounds_host) return LMX_OK;  // size query
  RS_REQUIRE(cap >= (int64_t)out_size * ksize, "lmx_h_pil_tables: kk_host holds %lld entries, %d x %d are needed", (long long)cap, out_size, ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;  // cannot happen (Pillow sizes ksize for it); the table's bounds do not rest on that
    if (xmax < 0) xmax = 0;
    int32_t* k = kk_host + (int64_t)xx * ksize;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += fn(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < ksize; ++x) {
      double w = x < xmax ? fn(((double)(x + xmin) - center + 0.5) * ss) : 0.0;
      if (x < xmax && ww != 0.0) w /= ww;
      // normalize_coeffs_8bpc: (int)(+-0.5 + k * 2^22), C truncation toward zero
      const double scaled = w * (double)(1 << PRECISION_BITS);
      k[x] = (int32_t)(w < 0 ? -0.5 + scaled : 0.5 + scaled);
    }
    bounds_host[2 * xx] = xmin;
    bounds_host[2 * xx + 1] = xmax;
  }
  return LMX_OK;
}

extern "C" int lmx_h_aa_tables(int in_size, int out_size, int filt, int32_t* bounds_host, float* kk_host, int64_t cap, int* ksize_host) {
  if (const int rc = check_args("lmx_h_aa_tables", in_size, out_size, filt, bounds_host, kk_host, ksize_host)) return rc;
  float (*const fn)(float) = filt == LMX_FILT_BILINEAR ? aa_bilinear : aa_bicubic;
  const float half_interp = filt == LMX_FILT_BILINEAR ? 1.0f : 2.0f;  // interp_size / 2
  const float scale = (float)in_size / (float)out_size;
  const float support = scale >= 1.0f ? half_interp * scale : half_interp;
  const int ksize = (int)ceil((double)support) * 2 + 1;
  *ksize_host = ksize;
  if (!bounds_host) return LMX_OK;  // size query
  RS_REQUIRE(cap >= (int64_t)out_size * ksize, "lmx_h_aa_tables: kk_host holds %lld entries, %d x %d are needed", (long long)cap, out_size, ksize);
  const float invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
  for (int i = 0; i < out_size; ++i) {
    // ATen's literals 0.5 are doubles: `x + 0.5` promotes the float32 difference / sum, and the result is narrowed again
    const float center = (float)((double)scale * (i + 0.5));
    int xmin = (int)((double)(float)(center - support) + 0.5);
    if (xmin < 0) xmin = 0;
    int xend = (int)((double)(float)(center + support) + 0.5);
    if (xend > in_size) xend = in_size;
    int xsize = xend - xmin;
    if (xsize < 0) xsize = 0;
    if (xsize > ksize) xsize = ksize;
    float* k = kk_host + (int64_t)i * ksize;
    float total = 0.0f;
    for (int j = 0; j < xsize; ++j) {
      const double d = (double)(float)((float)(j + xmin) - center);
      k[j] = fn((float)((d + 0.5) * (double)invscale));
      total = (float)(total + k[j]);  // ATen's running float32 sum, tap by tap
    }
    if (total != 0.0f)
      for (int j = 0; j < xsize; ++j) k[j] = k[j] / total;
    for (int j = xsize; j < ksize; ++j) k[j] = 0.0f;
    bounds_host[2 * i] = xmin;
    bounds_host[2 * i + 1] = xsize;
  }
  return LMX_OK;
}

extern "C" int lmx_h_identity_table(int n, int32_t* bounds_host, int32_t* kk_host) {
  RS_REQUIRE(n > 0 && bounds_host && kk_host, "lmx_h_identity_table: n %d / null pointer", n);
  for (int i = 0; i < n; ++i) {
    bounds_host[2 * i] = i;
    bounds_host[2 * i + 1] = 1;
    kk_host[i] = 1 << PRECISION_BITS;
  }
  return LMX_OK;
}

extern "C" int lmx_h_segment_cols(const int32_t* bounds_host, int n_out, int tile) {
  RS_REQUIRE(bounds_host && n_out > 0 && tile > 0, "lmx_h_segment_cols: n_out %d / tile %d / null pointer", n_out, tile);
  int best = 0;
  for (int t = 0; t < n_out; t += tile) {
    int lo = bounds_host[2 * t], hi = bounds_host[2 * t] + bounds_host[2 * t + 1];
    for (int i = t; i < n_out && i < t + tile; ++i) {
      const int b = bounds_host[2 * i], e = b + bounds_host[2 * i + 1];
      if (b < lo) lo = b;
      if (e > hi) hi = e;
    }
    if (hi - lo > best) best = hi - lo;
  }
  return best;
}
