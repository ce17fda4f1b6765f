// gait_launch.h — the host side of a launch that lmx_k_tcn_forward (tcn.hip) and lmx_k_xfm_forward (xfm.hip) share: one workgroup per
// (clip, sample), the per-clip seeds uploaded into the workspace, and the statistics of pred written by one more kernel.  HOST code.
#pragma once
#include <initializer_list>

#include "common.h"
#include "gait.h"

// stats[i] = {mean, unbiased standard deviation} of row i of pred on `st` (the kernel is in tcn.hip)
int lmx_gait_stats_launch(const float* pred, float* stats, int n, int S, hipStream_t st);

// one 64-bit seed per clip
inline int64_t lmx_gait_workspace_bytes(int n) { return n > 0 ? (int64_t)n * 8 : 0; }

// After the configuration and call checks, for n > 0 clips: the grid of n x max(S, 1) workgroups, the pointers (x, pred and stats must be
// there, `optional` ones may be null, all are f32-aligned), the seeds into the workspace on `st`, and the device `st` belongs to.
inline int lmx_gait_launch_prologue(const char* who, int n, int S, const float* x, const float* pred, const float* stats,
                                    std::initializer_list<const float*> optional, const uint64_t* seeds_host, void* workspace, hipStream_t st,
                                    unsigned* grid, int* dev) {
  const int Smax = S > 0 ? S : 1;
  LMX_REQUIRE((int64_t)n * Smax <= 0x7fffffff, "%s: n %d x S %d workgroups do not fit one grid", who, n, Smax);
  LMX_REQUIRE(x && pred && stats, "%s: null pointer", who);
  LMX_REQUIRE(S == 0 || (seeds_host && workspace), "%s: S = %d needs seeds_host and a workspace", who, S);
  uintptr_t bits = (uintptr_t)x | (uintptr_t)pred | (uintptr_t)stats;
  for (const float* p : optional) bits |= (uintptr_t)p;
  LMX_REQUIRE((bits & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "%s: misaligned pointer", who);
  LMX_TRY(lmx_stream_device(st, dev));
  if (S > 0) LMX_HIP(hipMemcpyAsync(workspace, seeds_host, (size_t)n * 8, hipMemcpyHostToDevice, st));
  *grid = (unsigned)(n * Smax);
  return LMX_OK;
}
