// model_handle.h — what every model-level handle of the C-ABI (dino_model.hip, yolo_model.hip, sam_model.hip) owns and does the same way: the device
// it was opened on, the weights of its image in one allocation, a stream of its own for the *_host entry points, one staging blob,
// and the open / close / device-check protocol around them.  HOST code, header-only: a plain struct and free functions; the model's
// handle derives from the struct and keeps its plan and its prepared entries to itself; how a plan obtains its workspace is plan_run.h's.
// The descriptors of the plans' GEMM and attention launches are filled here, once for all of them.
// Each function that can refuse takes the calling entry point's name (`fn`) for its message.
#pragma once
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "common.h"
#include "plan_run.h"

const int LMX_MAX_PREPARED = 16;  // prepared entries (a frame size, or a frame size and a plan) a handle keeps; each owns its workspace

struct LmxHandleCore {
  int device = -1, max_batch = 0;
  char* weights = nullptr;    // the data section of the image
  hipStream_t own = nullptr;  // the *_host entry points' stream
  // the *_host entry points' staging blob (grown on demand; those calls synchronise anyway)
  char* stage = nullptr;
  size_t stage_bytes = 0;
};

// offsets inside one allocation: every buffer on a 256-byte boundary
struct LmxLayout {
  size_t total = 0;
  size_t add(size_t bytes) {
    const size_t at = total;
    total += up256(bytes);
    return at;
  }
};

// one host table bound for offset `at` of a blob (bytes 0: nothing to copy)
struct LmxUpload {
  size_t at;
  const void* src;
  size_t bytes;
};

// One device allocation of `total` bytes with the `n` host tables copied in, complete when the call returns (the prepare calls are
// documented SYNCHRONOUS).  On failure nothing stays allocated and *blob is null.
inline int lmx_alloc_and_upload(size_t total, const LmxUpload* up, int n, char** blob) {
  *blob = nullptr;
  char* b = nullptr;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&b), total));
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; ++i)
    if (up[i].bytes) e = hipMemcpy(b + up[i].at, up[i].src, up[i].bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(b);
    LMX_HIP(e);
  }
  *blob = b;
  return LMX_OK;
}

inline int lmx_handle_on_device(const LmxHandleCore* m, const char* fn) {
  LMX_REQUIRE(m != nullptr, "%s: null handle", fn);
  int cur = -1;
  LMX_HIP(hipGetDevice(&cur));
  LMX_REQUIRE(cur == m->device, "%s: the handle was opened on device %d, the current device is %d", fn, m->device, cur);
  return LMX_OK;
}

// a caller's stream must belong to the handle's device.  Check it BEFORE preparing anything: a refused call allocates nothing
inline int lmx_handle_stream_on_device(const LmxHandleCore* m, const char* fn, hipStream_t st) {
  int st_dev = -1;
  LMX_TRY(lmx_stream_device(st, &st_dev));
  LMX_REQUIRE(st_dev == m->device, "%s: the stream belongs to device %d, the handle to device %d", fn, st_dev, m->device);
  return LMX_OK;
}

// the handle takes the current device, and the data section [data_offset, file_bytes) of the image into one device allocation
// through a bounded host buffer
inline int lmx_handle_upload_weights(LmxHandleCore* m, const char* fn, const char* path, uint64_t data_offset, uint64_t file_bytes) {
  const uint64_t total = file_bytes - data_offset;
  LMX_REQUIRE(total > 0, "%s: the image holds no tensor data", fn);
  LMX_HIP(hipGetDevice(&m->device));
  FILE* f = fopen(path, "rb");
  LMX_REQUIRE(f, "%s: cannot open '%s'", fn, path);
  std::unique_ptr<FILE, int (*)(FILE*)> closer(f, fclose);
  LMX_REQUIRE(fseeko(f, (off_t)data_offset, SEEK_SET) == 0, "%s: cannot seek to data_offset", fn);
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->weights), (size_t)total));
  const size_t chunk = (size_t)64 << 20;
  std::vector<char> buf((size_t)(total < chunk ? total : chunk));
  for (uint64_t done = 0; done < total;) {
    const size_t n = (size_t)(total - done < chunk ? total - done : chunk);
    LMX_REQUIRE(fread(buf.data(), 1, n, f) == n, "%s: the file ends inside the tensor data (truncated while reading?)", fn);
    LMX_HIP(hipMemcpy(m->weights + done, buf.data(), n, hipMemcpyHostToDevice));
    done += n;
  }
  return LMX_OK;
}

// at least `need` bytes of staging (the old blob is idle once the handle's stream has drained)
inline int lmx_handle_grow_stage(LmxHandleCore* m, size_t need) {
  if (need <= m->stage_bytes) return LMX_OK;
  LMX_HIP(hipStreamSynchronize(m->own));
  (void)hipFree(m->stage);
  m->stage = nullptr;
  m->stage_bytes = 0;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->stage), need));
  m->stage_bytes = need;
  return LMX_OK;
}

// what the core owns; the model's destroy frees its own allocations, calls this, and deletes the handle
inline void lmx_handle_free(LmxHandleCore* m) {
  (void)hipFree(m->stage);
  (void)hipFree(m->weights);
  if (m->own) (void)hipStreamDestroy(m->own);
}

// the last steps of an open: the handle's own stream, and everything the open enqueued is done
inline int lmx_handle_finish_open(LmxHandleCore* m) {
  LMX_HIP(hipStreamCreate(&m->own));
  LMX_HIP(hipDeviceSynchronize());
  return LMX_OK;
}

// lmx_<model>_open_host: `open_into` parses the image, uploads the weights (lmx_handle_upload_weights) and builds the model's own
// state in a fresh handle.  On any failure the handle is destroyed, *out_host stays NULL and the failing step's error text stays.
template <class H>
int lmx_handle_open(const char* fn, const char* path_host, int max_batch, H** out_host, int (*open_into)(H*, const char*), void (*destroy)(H*)) {
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", fn);
  *out_host = nullptr;
  LMX_REQUIRE(path_host != nullptr, "%s: path_host is null", fn);
  LMX_REQUIRE(max_batch > 0 && max_batch <= 65535, "%s: max_batch %d outside 1 .. 65535", fn, max_batch);
  H* m = new H();
  m->max_batch = max_batch;
  int rc = open_into(m, path_host);
  if (rc == LMX_OK) rc = lmx_handle_finish_open(m);
  if (rc != LMX_OK) {
    destroy(m);
    return rc;
  }
  *out_host = m;
  return LMX_OK;
}

// lmx_<model>_close: work that still reads the handle's memory must be done before it is freed; frees follow the handle's device
template <class H>
void lmx_handle_close(H* m, void (*destroy)(H*)) {
  if (!m) return;
  int cur = -1;
  const bool sw = hipGetDevice(&cur) == hipSuccess && cur != m->device && hipSetDevice(m->device) == hipSuccess;
  (void)hipDeviceSynchronize();
  destroy(m);
  if (sw) (void)hipSetDevice(cur);
}

// the stream of a run (plan_run.h carries it as lmx_stream_t)
inline hipStream_t lmx_run_stream(const LmxPlanRun& R) { return reinterpret_cast<hipStream_t>(R.st); }

// ---- the descriptors of the plans' launches, each filled in ONE place as lmx/kernels.py fills it ----------------------------------
// a dense GEMM C = act(A W^T + bias) (* scale) (+ res) as lmx/kernels.py's gemm fills its descriptor.  a_rep = 2: W is [N, 2 K'] =
// [whi | wlo] and A's K' = K / 2 columns are walked twice (K counts W's columns); res_rows > 0: res is a [res_rows, N] table
// broadcast over the rows.  Optional: pool_h > 0: the rows of A are an [n, pool_h, pool_w] grid and C [M / 4][N] its 2 x 2 max-pool;
// ln_out: the LayerNorm of the result's rows (f16, row stride N) from the same launch
inline int lmx_gemm_dense_rep(const void* A, int64_t lda, const void* W, const float* bias, void* C, int64_t ldc, int out_dtype, int M, int N, int K,
                              int act, const float* scale, const void* res, int64_t ldr, int res_rows, int a_rep, hipStream_t st, int pool_h = 0,
                              int pool_w = 0, void* ln_out = nullptr, const float* ln_g = nullptr, const float* ln_b = nullptr, float ln_eps = 0.f) {
  lmx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = A, d.W = W, d.bias = bias, d.scale = scale, d.res = res, d.C = C;
  d.lda = lda, d.ldc = ldc, d.ldr = res ? ldr : 0;
  d.M = M, d.N = N, d.K = K;
  d.act = act, d.out_dtype = out_dtype, d.res_rows = res_rows, d.a_rep = a_rep;
  d.a_mode = 0;
  if (pool_h) d.a_mode = 2, d.H = pool_h, d.W_ = pool_w;
  if (ln_out) d.ln_out = ln_out, d.ln_gamma = ln_g, d.ln_beta = ln_b, d.ld_ln = N, d.ln_eps = ln_eps;
  return lmx_k_gemm(&d, st);
}

inline int lmx_gemm_dense(const void* A, int64_t lda, const void* W, const float* bias, void* C, int64_t ldc, int out_dtype, int M, int N, int K, int act,
                          const float* scale, const void* res, int64_t ldr, hipStream_t st) {
  return lmx_gemm_dense_rep(A, lda, W, bias, C, ldc, out_dtype, M, N, K, act, scale, res, ldr, 0, 1, st);
}

// K.conv3x3: 3 x 3 / pad 1 as implicit GEMM over n frames of x [H, W, Cin] (pixel stride lda) -> C [n, Ho, Wo, N].  res: null or a
// residual of pixel stride ldr; split_k > 1: that many partial sums, one [n, Ho, Wo, N] block each
inline int lmx_gemm_conv3(const void* x, int64_t lda, int n, int H, int W, int Cin, const void* w, const float* bias, const float* scale, void* C,
                          int64_t ldc, int out_dtype, int N, int act, int stride, const void* res, int64_t ldr, int split_k, hipStream_t st) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  lmx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = x, d.W = w, d.bias = bias, d.scale = scale, d.res = res, d.C = C;
  d.lda = lda, d.ldc = ldc, d.ldr = res ? ldr : 0;
  d.M = n * Ho * Wo, d.N = N, d.K = 9 * Cin;
  d.act = act, d.out_dtype = out_dtype;
  d.a_mode = 1, d.H = H, d.W_ = W, d.Cin = Cin, d.conv_stride = stride, d.Ho = Ho, d.Wo = Wo;
  if (split_k > 1) d.split_k = split_k, d.split_stride = (int64_t)n * Ho * Wo * N;
  return lmx_k_gemm(&d, st);
}

// flat attention (mode 0) of B sequences: Tq queries on Tk keys, q / k / v rows of stride ldq / ldkv / ldkv, output rows of stride ldo
inline lmx_attn_desc lmx_attn_flat(const void* Q, int64_t ldq, const void* K, const void* V, int64_t ldkv, void* O, int64_t ldo, int B, int H, int Tq, int Tk,
                                   int hd, float scale) {
  lmx_attn_desc ad;
  memset(&ad, 0, sizeof(ad));
  ad.Q = Q, ad.K = K, ad.V = V, ad.O = O;
  ad.ldq = ldq, ad.ldk = ad.ldv = ldkv, ad.ldo = ldo;
  ad.B = B, ad.H = H, ad.Tq = Tq, ad.Tk = Tk, ad.hd = hd;
  ad.scale = scale;
  ad.mode = 0;
  return ad;
}

// windowed attention (mode 1) of n frames whose keys lie on a [Gh][Gw] grid cut into ws x ws windows (padding keys: pad_k / pad_v);
// pooled: the queries lie on the grid subsampled by 2 (Hiera's Q-pool)
inline lmx_attn_desc lmx_attn_windowed(const void* Q, int64_t ldq, const void* K, const void* V, int64_t ldkv, void* O, int64_t ldo, int n, int H, int hd,
                                       float scale, int Gh, int Gw, int ws, bool pooled, const void* pad_k, const void* pad_v) {
  const int nW = ((Gh + ws - 1) / ws) * ((Gw + ws - 1) / ws), wq = pooled ? ws / 2 : ws;
  lmx_attn_desc ad = lmx_attn_flat(Q, ldq, K, V, ldkv, O, ldo, n * nW, H, wq * wq, ws * ws, hd, scale);
  ad.mode = 1;
  ad.Gh = Gh, ad.Gw = Gw, ad.ws = ws, ad.q_stride = pooled ? 2 : 1;
  ad.pad_k = pad_k, ad.pad_v = pad_v;
  return ad;
}
