// common.h — shared helpers for the liblmx HIP sources (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/lmx.h"

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// thread-local error text (lmx_last_error)
void lmx_set_error(const char* fmt, ...);

#define LMX_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      lmx_set_error(__VA_ARGS__);         \
      return LMX_EINVAL;                  \
    }                                     \
  } while (0)

#define LMX_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      lmx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return LMX_EHIP;                                                                  \
    }                                                                                   \
  } while (0)

// propagate the LMX_* code of a host helper (its error text is already set)
#define LMX_TRY(call)               \
  do {                              \
    const int rc_ = (call);         \
    if (rc_ != LMX_OK) return rc_;  \
  } while (0)

// ---- per-device launch state (api.hip).  A launcher keeps NO static of its own for these: one process drives several
// devices from several threads (lmx/kernels.py _stream), so whatever is learned or set once is keyed by the device the
// stream belongs to and guarded there.
// the ordinal of the device a launch on `st` goes to.  The NULL stream (torch's default stream) belongs to no device: such a launch
// goes to the calling thread's CURRENT device, which the caller must have made the operands' device
int lmx_stream_device(hipStream_t st, int* dev);
// multiProcessorCount of device `dev` (256 if the runtime reports none), queried once per device; < 0: an LMX_* error
int lmx_cu_count(int dev);
// the grid of a persistent kernel: one workgroup per CU of `dev`, or `need` of them if that is fewer
int lmx_persistent_grid(int64_t need, int dev, unsigned* grid);
// allow `kernel` up to `bytes` of dynamic LDS on device `dev` (hipFuncAttributeMaxDynamicSharedMemorySize): the runtime is
// called once per (kernel, device), later calls only look the pair up
int lmx_allow_lds(const void* kernel, int bytes, int dev);
// development switches.  A switch that steers dispatch is read ONCE, as the initialiser of a function-local `static const int`
// (C++11 evaluates it once, thread-safe); only an argument check may ask per call (lmx_k_ln_mlp's LMX_MLP448).
// atoi of the variable or dflt if it is unset | 1 if it is set at all | its first character (0: unset or empty)
int lmx_env_int(const char* name, int dflt);
int lmx_env_set(const char* name);
int lmx_env_char(const char* name);

// ---- kernel selection (Reproducibility).  lmx_k_gemm, lmx_k_attention and lmx_k_layernorm each validate and choose in one
// pure host function (gemm_route, attn_route, ln_route: no HIP call, nothing read behind the descriptor's pointers) and launch in
// another, which holds one switch from the route to the instantiation; lmx_h_*_route return the route's name without a GPU.
// the kernel of a GEMM: the register-staged gemm_kernel (gemm.hip; BM x BN x 64, two LDS buffers) or the LDS-DMA gemm2_kernel
// (gemm2.hip) with its tiling; rowln: gemm2_rowln_kernel, 128 rows x the whole row with the next LayerNorm in its epilogue
// (lmx_gemm_desc.ln_out)
struct GemmRoute {
  bool dma;
  int BM, BN, BK, NSTAGE, STAG;
  bool rowln = false;
};
// a route's name into the caller's buffer (the lmx_h_*_route entry points only: no launch formats a string)
#define LMX_ROUTE_NAME(name, cap, ...)                                                                          \
  do {                                                                                                          \
    LMX_REQUIRE((name) != nullptr && (cap) > 0, "%s: no room for the name", __func__);                          \
    LMX_REQUIRE(snprintf((name), (size_t)(cap), __VA_ARGS__) < (cap), "%s: name buffer of %d bytes is too short", __func__, (cap)); \
  } while (0)

static inline int lmx_launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    lmx_set_error("launch of %s failed: %s", what, hipGetErrorString(e));
    return LMX_EHIP;
  }
  return LMX_OK;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// erf-GELU for two values at once: gelu(v) = v * (0.5 + g(v)), g(v) = 0.5*erf(v/sqrt2) ~ vc * P(vc^2) with
// vc = clamp(v, -4.5, 4.5) and P of degree 9 (weighted least-squares Chebyshev fit, evaluated in f32: |error| <= 3.4e-5
// for every v, i.e. a tenth of the f16 rounding of an O(1) result; tools/fit_gelu.py reproduces the coefficients).
// No transcendental (v_rcp / v_exp are quarter rate) and written on 2-vectors so the Horner chain is v_pk_fma_f32:
// ~7.5 VALU issue slots per value against ~23 for the Abramowitz-Stegun erf it replaces.  (The same polynomial on scalar v_fma_f32
// chains — identical bits — measured the same: fused LN + MLP 0.92 / 0.63 ms against 0.88 / 0.64, bench 596.8 against 597.3
// frames/s, profiles/r03_gelu_scalar_ab.txt.)  At D = 112..448 the GELU of an
// MLP otherwise costs more VALU time than its two GEMMs cost MFMA time.
__device__ __forceinline__ f32x2 gelu_pk(f32x2 v) {
  f32x2 vc;
  vc[0] = __builtin_amdgcn_fmed3f(v[0], -4.5f, 4.5f);
  vc[1] = __builtin_amdgcn_fmed3f(v[1], -4.5f, 4.5f);
  const f32x2 u = vc * vc;
  f32x2 p = {-1.223331157e-12f, -1.223331157e-12f};
  p = p * u + 1.524351007e-10f;
  p = p * u + -8.481037793e-09f;
  p = p * u + 2.798429583e-07f;
  p = p * u + -6.151207192e-06f;
  p = p * u + 9.615961466e-05f;
  p = p * u + -1.114801972e-03f;
  p = p * u + 9.814679350e-03f;
  p = p * u + -6.632144717e-02f;
  p = p * u + 3.988863025e-01f;
  const f32x2 g = vc * p;
  return v * g + 0.5f * v;
}
__device__ __forceinline__ float gelu_1(float v) {
  const f32x2 r = gelu_pk(f32x2{v, v});
  return r[0];
}

// The activation of every GEMM / conv epilogue.  ONE definition for all kernel variants: which variant the launcher picks
// depends on M = frames x pixels, so two variants that rounded differently would make a frame's result depend on the batch
// it rides in (tools/batch_invariance_probe.py).  SiLU by v_exp / v_rcp, erf-GELU by the polynomial above.
__device__ __forceinline__ float lmx_act(float v, int act) {
  if (act == LMX_ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-v * 1.44269504088896340736f));
  if (act == LMX_ACT_GELU) return gelu_1(v);
  if (act == LMX_ACT_RELU) return fmaxf(v, 0.0f);
  return v;
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// One LDS-DMA wave-instruction (buffer_load_dwordx4 ... lds): lane i's 16 bytes land at dst + 16*i.  Kept in a
// NON-template function: inside a kernel template with dependent arguments the amdgcn builtin makes the HOST pass drop
// the kernel's instantiation without a diagnostic (the .so then fails to load with an undefined __device_stub__).
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, char* dst_lds, unsigned voffset, int soffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst_lds, 16, voffset, soffset, 0, 0);
}

// counted wait with a literal immediate per instantiation (an "n"-constrained template-dependent asm operand makes
// hipcc drop the HOST stub of the enclosing kernel template without a diagnostic)
#define LMX_WAIT_CASE(n) \
  if constexpr (N == n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N == 0 || N == 1 || N == 2 || N == 3 || N == 4 || N == 6 || N == 8 || N == 9 || N == 12 || N == 16 || N == 18 || N == 24 ||
                    N == 32,
                "add the literal for this count");
  LMX_WAIT_CASE(0);
  LMX_WAIT_CASE(1);
  LMX_WAIT_CASE(2);
  LMX_WAIT_CASE(3);
  LMX_WAIT_CASE(4);
  LMX_WAIT_CASE(6);
  LMX_WAIT_CASE(8);
  LMX_WAIT_CASE(9);
  LMX_WAIT_CASE(12);
  LMX_WAIT_CASE(16);
  LMX_WAIT_CASE(18);
  LMX_WAIT_CASE(24);
  LMX_WAIT_CASE(32);
}
#undef LMX_WAIT_CASE
// wait until at most y * PT of this wave's vector-memory operations are outstanding (y = 0..4 whole k-tiles of PT DMAs)
template <int PT>
__device__ __forceinline__ void wait_tiles(int y) {
  if (y >= 4)
    wait_vmcnt<4 * PT>();
  else if (y == 3)
    wait_vmcnt<3 * PT>();
  else if (y == 2)
    wait_vmcnt<2 * PT>();
  else if (y == 1)
    wait_vmcnt<PT>();
  else
    wait_vmcnt<0>();
}

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- helpers of the bit-exact files (compiled there with -ffp-contract=off) ----
// SiLU as torch's CPU kernel writes it: x / (1 + exp(-x)) with a true division (the f16 plan's v_exp / v_rcp form is 1-2 ulp
// looser, which the exact plan cannot afford to spend)
__device__ __forceinline__ float act_exact(float v, int act) {
  if (act == LMX_ACT_SILU) return v / (1.0f + expf(-v));
  if (act == LMX_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == LMX_ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));  // the erf form torch's GELU evaluates
  return v;
}

// torch upsample_bilinear2d(align_corners=False) source index: scale*(dst+0.5)-0.5 clamped at 0
__device__ __forceinline__ void bil_idx(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__device__ __forceinline__ float sample_mid(const float* __restrict__ lg, int L, int T, float sLT, int Y, int X) {
  // value of the TxT bilinear upsample of the LxL logits at integer position (Y, X)
  int y0, y1, x0, x1;
  float ly, lx;
  bil_idx(sLT, Y, L, y0, y1, ly);
  bil_idx(sLT, X, L, x0, x1, lx);
  const float t0 = (1.f - lx) * lg[y0 * L + x0] + lx * lg[y0 * L + x1];
  const float t1 = (1.f - lx) * lg[y1 * L + x0] + lx * lg[y1 * L + x1];
  return (1.f - ly) * t0 + ly * t1;
}
