// tleap.hip — lmx_k_tleap_series (include/lmx.h "Pose series"): the detector's outputs, where lmx_yolo_detect leaves them in HBM, become
// tleap's pose records, the target x 44 series and the key-padding mask of n clips in ONE launch, one workgroup of 256 lanes per clip.
//   1. rows: the per-frame row counts of the clip are scanned in chunks of 256 frames (an inclusive scan in each wave by lane shifts, the
//      four wave totals and the carry of the chunks before through LDS; no atomics), and every frame writes the (frame, detection) pair
//      of each of its rows into the row map of the workspace at its exclusive offset;
//   2. records: one lane per row builds the record with the arithmetic of tleap.h, the text the host twin compiles;
//   3. series and mask: one lane per (step, feature) and per step over the clip's own records, lmx_h_tcn_features and lmx_h_xfm_mask
//      restated below.
// The three phases hand over through global memory inside ONE workgroup (a barrier between them; the records and the map of a clip are
// read by the workgroup that wrote them and by no other).  Built with -ffp-contract=off (the Makefile's EXACT list): every double
// operation rounds once, as Python's does.  The kernel is small and is not where a clip's time goes; the pose model is.
#include "common.h"
#include "tleap.h"

namespace {

constexpr int kLanes = 256;

struct TleapOut {
  const int32_t* clip_first;  // [n + 1] in the workspace
  int32_t* map;               // [F * max_det][2] in the workspace
  int32_t* rows;
  lmx_tleap_record_t* records;
  float* series;
  uint8_t* mask;
  int target;
};

__device__ __forceinline__ float centroid_x(const lmx_tleap_record_t& r) { return (float)((r.bbox[0] + r.bbox[2]) / 2 / 1280); }

// feature `col` of row t of the clip (host_tcn.cpp lmx_h_tcn_features)
__device__ float feature(const lmx_tleap_record_t* rec, int t, int col) {
  const lmx_tleap_record_t& r = rec[t];
  const double* b = r.bbox;
  const double bw = b[2] - b[0], bh = b[3] - b[1];
  if (col < 2 * LMX_TLEAP_KEYPOINTS) {
    const int i = col >> 1, xy = col & 1;
    if (i >= r.n_kp) return 0.0f;
    const double d = xy ? (bh > 1 ? bh : 1) : (bw > 1 ? bw : 1);
    return (float)((r.keypoints[i][xy] - b[xy]) / d);
  }
  if (col == 40) return centroid_x(r);
  if (col == 41) return (float)((b[1] + b[3]) / 2 / 720);
  if (col == 42) return (float)(bw * bh / (1280 * 720));
  return t > 0 ? centroid_x(r) - centroid_x(rec[t - 1]) : 0.0f;  // the f32 difference of the f32 column, before the crop
}

__global__ __launch_bounds__(kLanes) void tleap_series_kernel(LmxTleapIn in, TleapOut out) {
  __shared__ int wave_total[kLanes / 64];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int f0 = out.clip_first[c], nf = out.clip_first[c + 1] - f0;
  int32_t* map = out.map + (size_t)f0 * in.max_det * 2;
  lmx_tleap_record_t* rec = out.records + (size_t)f0 * in.max_det;

  int carry = 0;  // rows of the chunks before this one: the same sum of LDS words in every lane
  for (int base = 0; base < nf; base += kLanes) {
    const int rel = base + tid;
    const int cnt = rel < nf ? lmx_tleap_frame_rows(in, f0 + rel) : 0;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wave_total[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kLanes / 64; ++k) {
      const int t = wave_total[k];
      before += k < wv ? t : 0;
      total += t;
    }
    if (cnt > 0) lmx_tleap_frame_map(in, f0 + rel, rel, map + 2 * (size_t)(carry + before + inc - cnt));
    carry += total;
    __syncthreads();  // wave_total is written again by the next chunk
  }
  const int T0 = carry;  // at most nf * max_det: a frame has at most max_det rows, so the map and the records stay inside the clip's share
  if (tid == 0) out.rows[c] = T0;
  __syncthreads();  // the map is complete

  for (int r = tid; r < T0; r += kLanes) lmx_tleap_record(in, f0 + map[2 * r], map[2 * r], map[2 * r + 1], rec + r);
  __syncthreads();  // the records are complete

  const int target = out.target, F = LMX_GAIT_FEATURES;
  const LmxGaitWindow win = lmx_gait_window(T0, target);
  float* series = out.series + (size_t)c * target * F;
  for (int i = tid; i < target * F; i += kLanes) {
    const int r = i / F - win.at;
    series[i] = r >= 0 && r < win.rows ? feature(rec, win.first + r, i % F) : 0.0f;
  }
  uint8_t* mask = out.mask + (size_t)c * target;
  for (int s = tid; s < target; s += kLanes) {
    const int r = s - win.at;
    uint8_t m = 1;
    if (r >= 0 && r < win.rows) {
      const lmx_tleap_record_t& q = rec[win.first + r];
      double sum = 0.0;
      for (int i = 0; i < q.n_kp; ++i) sum += q.keypoints[i][2];
      m = (float)(sum / LMX_TLEAP_KEYPOINTS * q.confidence) < 0.3f ? 1 : 0;
    }
    mask[s] = m;
  }
}

}  // namespace

extern "C" int64_t lmx_tleap_workspace_bytes(int F, int max_det) {
  if (F < 1 || max_det < 1 || (int64_t)F * max_det > (1 << 24)) return 0;
  return lmx_tleap_bounds_bytes(F) + (int64_t)F * max_det * 8;
}

extern "C" int lmx_k_tleap_series(const float* boxes, const float* scores, const int32_t* cls, const int32_t* counts, const float* kpts, int K,
                                  int ndim, int F, int max_det, int h, int w, const int32_t* clip_first_host, int n, int target, int mode,
                                  const int32_t* cow_classes_host, int n_cow, int32_t* rows, lmx_tleap_record_t* records, float* series,
                                  uint8_t* mask, void* workspace, lmx_stream_t stream) {
  LmxTleapIn in;
  LMX_TRY(lmx_tleap_check("lmx_k_tleap_series", boxes, scores, cls, counts, kpts, K, ndim, F, max_det, h, w, clip_first_host, n, target, mode,
                          cow_classes_host, n_cow, rows, records, series, mask, &in));
  LMX_REQUIRE(workspace, "lmx_k_tleap_series: null workspace");
  LMX_REQUIRE(((uintptr_t)workspace & 7) == 0, "lmx_k_tleap_series: workspace is not 8-byte aligned");
  LMX_REQUIRE((int64_t)n * target * LMX_GAIT_FEATURES <= 0x7fffffff, "lmx_k_tleap_series: n %d x target %d steps", n, target);
  hipStream_t st = (hipStream_t)stream;
  int dev;
  LMX_TRY(lmx_stream_device(st, &dev));
  LMX_HIP(hipMemcpyAsync(workspace, clip_first_host, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
  TleapOut out{(const int32_t*)workspace, (int32_t*)((char*)workspace + lmx_tleap_bounds_bytes(F)), rows, records, series, mask, target};
  hipLaunchKernelGGL(tleap_series_kernel, dim3((unsigned)n), dim3(kLanes), 0, st, in, out);
  return lmx_launch_check("tleap_series_kernel");
}
