// api.hip — library-level entry points of the C-ABI (version, error text, device probe) and the per-device launch state.
#include "common.h"
#include <stdlib.h>
#include <string.h>
#include <map>
#include <mutex>
#include <set>
#include <utility>

static thread_local char g_err[512] = "";

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- per-device launch state (declared in common.h) ----
static std::mutex g_launch_mu;                         // guards the two tables below
static std::map<int, int> g_cu;                        // device -> CU count
static std::set<std::pair<const void*, int>> g_lds;    // (kernel, device) pairs whose LDS limit has been raised

int lmx_stream_device(hipStream_t st, int* dev) {
  if (st)
    LMX_HIP(hipStreamGetDevice(st, dev));
  else
    LMX_HIP(hipGetDevice(dev));
  return LMX_OK;
}

int lmx_cu_count(int dev) {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  int& n = g_cu[dev];  // 0: not asked yet (and still 0 if the query below fails)
  if (!n) {
    hipDeviceProp_t prop;
    LMX_HIP(hipGetDeviceProperties(&prop, dev));
    n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return n;
}

int lmx_persistent_grid(int64_t need, int dev, unsigned* grid) {
  const int n_cu = lmx_cu_count(dev);
  if (n_cu < 0) return n_cu;
  *grid = (unsigned)(need < n_cu ? need : n_cu);
  return LMX_OK;
}

int lmx_allow_lds(const void* kernel, int bytes, int dev) {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  if (g_lds.count({kernel, dev})) return LMX_OK;
  // hipFuncSetAttribute takes neither a device nor a stream: it acts on the kernel's image for the calling thread's CURRENT device.
  // A launch follows its stream, not the current device, so `dev` is made current for the call and the previous one restored.
  int cur = 0;
  LMX_HIP(hipGetDevice(&cur));
  if (cur != dev) LMX_HIP(hipSetDevice(dev));
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  const hipError_t back = cur != dev ? hipSetDevice(cur) : hipSuccess;
  LMX_HIP(e);
  LMX_HIP(back);
  g_lds.insert({kernel, dev});
  return LMX_OK;
}

int lmx_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
int lmx_env_set(const char* name) { return getenv(name) ? 1 : 0; }
int lmx_env_char(const char* name) {
  const char* e = getenv(name);
  return e ? e[0] : 0;
}

extern "C" int lmx_version(void) { return LMX_VERSION; }
extern "C" const char* lmx_last_error(void) { return g_err; }
extern "C" int lmx_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    lmx_set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    return LMX_EHIP;
  }
  return n;
}
