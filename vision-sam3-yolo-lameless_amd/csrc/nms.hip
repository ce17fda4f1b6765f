// nms.hip — K8: ultralytics non_max_suppression as the predictor invokes it under
// services/yolo-pipeline/app/main.py:76 (conf filter -> best class -> sort by score -> class offset ->
// torchvision.ops.nms(iou 0.7) -> first max_det).  Integer/index work must be bit-exact, so:
//   * this file is compiled with -ffp-contract=off (no FMA contraction) and IEEE f32 division;
//   * IoU follows torchvision/csrc/ops/cpu/nms_kernel.cpp (not in tree): areas on the class-offset boxes,
//     inter / (iarea + areas[j] - inter), compared as (double)ovr > iou_threshold;
//   * the sort key is (score, anchor index): descending score, ties broken by the LOWER anchor index (torch's
//     argsort(descending=True) leaves tie order unspecified; this is the stable-sort answer).
//
// Kernels
//   nms_filter_kernel : max over the nc class scores of every anchor with coalesced loads along the rows, conf test, per-wave
//                       append of a 64-bit key (score bits << 32 | ~anchor) to the image's list.
//   nms_boxes_kernel  : torchvision.ops.nms on plain xyxy boxes and scores of any sign (lmx_k_nms_boxes): its own keys,
//                       then the same sort and greedy block suppression (bitonic_sort_desc, greedy_blocks).
//   nms_greedy_kernel : one 1024-thread workgroup per image: bitonic sort of the keys in LDS (<=16384 keys =
//                       128 KB of the 160 KB LDS), gather of the sorted class-offset boxes to the workspace, then
//                       greedy suppression in blocks of 64 sorted candidates: wave 0 resolves the block
//                       (64x64 IoU bitmask per lane, 64-step scalar scan with v_readlane), then all 16 waves
//                       suppress the later candidates against the block's kept boxes.  Stops at max_det.
#include "common.h"

namespace {

constexpr int MAX_A = 16384;

// Lanes of a wave share rows: a row is read in pieces (16 bytes where VEC, one float otherwise) by L = min(pieces, 64)
// neighbouring lanes, 64 / L rows per wave pass, so a wave's loads run along the rows (for nc = 80: 21 lanes a row, three rows
// a wave).  The row maximum — all the filter needs; nms_greedy_kernel finds the class of a candidate — is reduced over the L
// lanes with shuffles; the keys of a wave are appended with one atomicAdd per image present in it.
template <bool VEC>
__global__ __launch_bounds__(256) void nms_filter_kernel(const float* __restrict__ pred, int n, int A, int nc,
                                                         float conf, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ counts) {
  const int64_t total = (int64_t)n * A;
  const int row_len = 4 + nc;
  const int pieces = VEC ? row_len / 4 : row_len;
  const int L = pieces < 64 ? pieces : 64;
  const int rpw = 64 / L;  // rows per wave pass
  const int lane = threadIdx.x & 63;
  const int r = lane / L, q = lane - r * L;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * (blockDim.x >> 6) * rpw;
  for (int64_t base = wave * rpw; base < total; base += step) {  // wave-uniform: every lane takes part in the shuffles
    const int64_t i = base + r;
    const bool live = r < rpw && i < total;
    const int img = live ? (int)(i / A) : 0;
    float best = -__builtin_inff();
    if (live) {
      const float* row = pred + i * row_len;
      if (VEC) {
        for (int u = q > 0 ? q : L; u < pieces; u += L) {  // piece 0 is the box
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * u);
#pragma unroll
          for (int e = 0; e < 4; ++e) best = v[e] > best ? v[e] : best;
        }
      } else {
        for (int u = q; u < pieces; u += L) {
          const float v = row[u];
          best = (u >= 4 && v > best) ? v : best;
        }
      }
    }
    // after the step `off` lane q holds the maximum of lanes q .. q + 2 * off - 1 of its row
    for (int off = 1; off < L; off <<= 1) {
      const float o = __shfl_down(best, off, 64);
      best = (q + off < L && o > best) ? o : best;
    }
    const bool pass = live && q == 0 && best > conf;
    const unsigned long long key =
        ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(i - (int64_t)img * A));
    unsigned long long todo = __ballot(pass);
    while (todo) {  // one round per image among the passing rows
      const int lead = __ffsll((long long)todo) - 1;
      const int img_l = __shfl(img, lead, 64);
      const bool mine = pass && img == img_l;
      const unsigned long long m = __ballot(mine);
      int slot = 0;
      if (lane == lead) slot = atomicAdd(&counts[img_l], __popcll(m));
      slot = __shfl(slot, lead, 64) + __popcll(m & ((1ull << lane) - 1ull));
      if (mine) keys[(int64_t)img * A + slot] = key;
      todo &= ~m;
    }
  }
}

struct Box {
  float x1, y1, x2, y2, area;
};

__device__ __forceinline__ bool iou_gt(const Box& a, const Box& b, double thr) {
  const float xx1 = a.x1 > b.x1 ? a.x1 : b.x1;
  const float yy1 = a.y1 > b.y1 ? a.y1 : b.y1;
  const float xx2 = a.x2 < b.x2 ? a.x2 : b.x2;
  const float yy2 = a.y2 < b.y2 ? a.y2 : b.y2;
  float w = xx2 - xx1;
  w = w > 0.f ? w : 0.f;
  float h = yy2 - yy1;
  h = h > 0.f ? h : 0.f;
  const float inter = w * h;
  const float ovr = inter / (a.area + b.area - inter);
  return (double)ovr > thr;
}

// bitonic sort of npow2 64-bit keys in LDS, descending (1024 threads; ends with a barrier)
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* keys, int npow2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= npow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow2; i += 1024) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], b = keys[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) {
            keys[i] = b;
            keys[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// Greedy suppression over the `count` sorted boxes SB[i] = {x1, y1, x2, y2, area} (i = sorted position), in blocks of 64: wave 0
// resolves a block (64x64 IoU bitmask per lane, 64-step scalar scan with v_readlane), emit(t, i, o) is called by threads
// t < nk for the block's t-th kept candidate (sorted position i, output slot o), then all 16 waves suppress the later
// candidates against the block's kept boxes.  Stops after max_keep kept candidates.  supp [>= count] starts at 0.  Returns
// the number kept (read by every thread).
template <class Emit>
__device__ __forceinline__ int greedy_blocks(const float* __restrict__ SB, int count, double iou, int max_keep, unsigned char* supp,
                                             Box* kept, Emit emit) {
  __shared__ int s_nk;
  __shared__ int s_total;
  __shared__ int s_kept_idx[64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (tid == 0) s_total = 0;
  __syncthreads();
  const int nblk = (count + 63) / 64;
  for (int blk = 0; blk < nblk; ++blk) {
    const int base = blk * 64;
    if (tid < 64) {
      const int i = base + lane;
      const bool valid = i < count;
      Box me{0.f, 0.f, 0.f, 0.f, 0.f};
      if (valid) me = Box{SB[i * 5 + 0], SB[i * 5 + 1], SB[i * 5 + 2], SB[i * 5 + 3], SB[i * 5 + 4]};
      // lane i: mask of later in-block candidates it would suppress
      unsigned long long mask = 0ull;
      for (int j = 0; j < 64; ++j) {
        Box o;
        o.x1 = __shfl(me.x1, j, 64);
        o.y1 = __shfl(me.y1, j, 64);
        o.x2 = __shfl(me.x2, j, 64);
        o.y2 = __shfl(me.y2, j, 64);
        o.area = __shfl(me.area, j, 64);
        if (j > lane && base + j < count && iou_gt(me, o, iou)) mask |= 1ull << j;
      }
      const bool alive0 = valid && supp[i] == 0;
      unsigned long long alive = __ballot(alive0);
      unsigned long long keepm = 0ull;
      const int room = max_keep - s_total;
      int nk = 0;
      for (int j = 0; j < 64 && nk < room; ++j) {
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)(mask & 0xFFFFFFFFull), j);
        const unsigned hi = __builtin_amdgcn_readlane((unsigned)(mask >> 32), j);
        if ((alive >> j) & 1ull) {
          keepm |= 1ull << j;
          alive &= ~(((unsigned long long)hi << 32) | lo);
          ++nk;
        }
      }
      if ((keepm >> lane) & 1ull) {
        const int pos = __popcll(keepm & ((1ull << lane) - 1ull));
        kept[pos] = me;
        s_kept_idx[pos] = i;
      }
      if (lane == 0) s_nk = nk;
    }
    __syncthreads();
    const int nk = s_nk;
    const int total_before = s_total;
    if (tid < nk) emit(tid, s_kept_idx[tid], total_before + tid);
    // suppress later candidates against the kept boxes of this block
    if (nk > 0 && total_before + nk < max_keep) {
      for (int j = base + 64 + tid; j < count; j += 1024) {
        if (supp[j]) continue;
        const Box o{SB[j * 5 + 0], SB[j * 5 + 1], SB[j * 5 + 2], SB[j * 5 + 3], SB[j * 5 + 4]};
        bool s = false;
        for (int k = 0; k < nk && !s; ++k) s = iou_gt(kept[k], o, iou);
        if (s) supp[j] = 1;
      }
    }
    __syncthreads();
    if (tid == 0) s_total = total_before + nk;
    __syncthreads();
    if (total_before + nk >= max_keep) break;
  }
  return s_total;
}

__global__ __launch_bounds__(1024) void nms_greedy_kernel(const float* __restrict__ pred, int A, int nc, double iou,
                                                          int max_det, float max_wh,
                                                          const unsigned long long* __restrict__ keys_g,
                                                          const int* __restrict__ cand_counts, float* __restrict__ sbox,
                                                          float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                          int* __restrict__ out_cls, int* __restrict__ out_src,
                                                          int* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [npow2]
  const int img = blockIdx.x;
  const int tid = threadIdx.x;
  const int count = cand_counts[img];
  const int row_len = 4 + nc;
  const float* P = pred + (int64_t)img * A * row_len;

  int npow2 = 64;
  while (npow2 < count) npow2 <<= 1;
  unsigned char* supp = reinterpret_cast<unsigned char*>(smem + (size_t)npow2 * 8);  // [npow2]
  Box* kept = reinterpret_cast<Box*>(smem + (size_t)npow2 * 9);                      // [64]  (npow2*9 % 16 == 0)

  for (int i = tid; i < npow2; i += 1024) {
    keys[i] = i < count ? keys_g[(int64_t)img * A + i] : 0ull;
    supp[i] = 0;
  }
  __syncthreads();
  bitonic_sort_desc(keys, npow2);

  // ---- gather the sorted, class-offset boxes (xywh2xyxy then + cls*max_wh, all f32 as ultralytics does)
  float* SB = sbox + (int64_t)img * A * 5;
  for (int i = tid; i < count; i += 1024) {
    const unsigned a = 0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull);
    const float* row = P + (int64_t)a * row_len;
    const float cx = row[0], cy = row[1], w = row[2], h = row[3];
    const float dw = w / 2.f, dh = h / 2.f;
    float best = row[4];
    int bc = 0;
    for (int c = 1; c < nc; ++c) {
      const float v = row[4 + c];
      if (v > best) {
        best = v;
        bc = c;
      }
    }
    const float off = (float)bc * max_wh;
    const float x1 = (cx - dw) + off, y1 = (cy - dh) + off, x2 = (cx + dw) + off, y2 = (cy + dh) + off;
    SB[i * 5 + 0] = x1;
    SB[i * 5 + 1] = y1;
    SB[i * 5 + 2] = x2;
    SB[i * 5 + 3] = y2;
    SB[i * 5 + 4] = (x2 - x1) * (y2 - y1);
  }
  __syncthreads();  // SB is re-read by this workgroup only; writes are visible after the barrier (same CU)

  // write each kept detection (un-offset box, score, class, anchor)
  const int total = greedy_blocks(SB, count, iou, max_det, supp, kept, [&](int, int i, int o) {
    const unsigned long long key = keys[i];
    const unsigned a = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const float* row = P + (int64_t)a * row_len;
    const float cx = row[0], cy = row[1], w = row[2], h = row[3];
    const float dw = w / 2.f, dh = h / 2.f;
    float best = row[4];
    int bc = 0;
    for (int c = 1; c < nc; ++c) {
      const float v = row[4 + c];
      if (v > best) {
        best = v;
        bc = c;
      }
    }
    float* ob = out_boxes + ((int64_t)img * max_det + o) * 4;
    ob[0] = cx - dw;
    ob[1] = cy - dh;
    ob[2] = cx + dw;
    ob[3] = cy + dh;
    out_scores[(int64_t)img * max_det + o] = best;
    out_cls[(int64_t)img * max_det + o] = bc;
    out_src[(int64_t)img * max_det + o] = (int)a;
  });
  if (tid == 0) out_counts[img] = total;
}

// torchvision.ops.nms on plain xyxy boxes with arbitrary f32 scores (SamAutomaticMaskGenerator: batched_nms with one
// category in _process_crop and _generate_masks).  One 1024-thread workgroup: the sort and greedy_blocks of nms_greedy_kernel.
// The 64-bit key is (order-preserving map of the score) << 32 | ~index: descending score for every sign (the raw-bits key
// of lmx_k_nms orders negative scores backwards), -0 taken as +0, ties to the LOWER index — the order of a stable argsort of
// -scores (oracle.nms.torchvision_nms).  Candidates with valid[i] == 0 get key 0, below every real key, and take no part.
__device__ __forceinline__ unsigned score_order_key(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;  // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(1024) void nms_boxes_kernel(const float* __restrict__ boxes, int64_t ldb, const float* __restrict__ scores,
                                                         const uint8_t* __restrict__ valid, int n, double iou,
                                                         float* __restrict__ sbox, int32_t* __restrict__ keep_out,
                                                         int32_t* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [npow2]
  const int tid = threadIdx.x;
  int npow2 = 64;
  while (npow2 < n) npow2 <<= 1;
  unsigned char* supp = reinterpret_cast<unsigned char*>(smem + (size_t)npow2 * 8);  // [npow2]
  Box* kept = reinterpret_cast<Box*>(smem + (size_t)npow2 * 9);                      // [64]
  __shared__ int s_count;

  if (tid == 0) s_count = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < npow2; i += 1024) {
    const bool v = i < n && (valid == nullptr || valid[i] != 0);
    keys[i] = v ? (((unsigned long long)score_order_key(scores[i]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
    supp[i] = 0;
    mine += v ? 1 : 0;
    if (i < n) keep_out[i] = -1;
  }
  // candidate count: wave sum, then one LDS add per wave (an integer: the order of the adds does not matter)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
  __syncthreads();
  const int count = s_count;
  bitonic_sort_desc(keys, npow2);

  // the sorted boxes with torchvision's areas
  for (int i = tid; i < count; i += 1024) {
    const unsigned a = 0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull);
    const float* r = boxes + (int64_t)a * ldb;
    sbox[i * 5 + 0] = r[0];
    sbox[i * 5 + 1] = r[1];
    sbox[i * 5 + 2] = r[2];
    sbox[i * 5 + 3] = r[3];
    sbox[i * 5 + 4] = (r[2] - r[0]) * (r[3] - r[1]);
  }
  __syncthreads();

  const int total = greedy_blocks(sbox, count, iou, count, supp, kept, [&](int, int i, int o) {
    keep_out[o] = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull));
  });
  if (tid == 0) count_out[0] = total;
}

}  // namespace

extern "C" int64_t lmx_nms_workspace_bytes(int n, int A) {
  if (n <= 0 || A <= 0) return 0;
  // counts (padded to 256 B) + keys u64 [n][A] + sorted boxes f32 [n][A][5]
  return 256 + ((int64_t)n * 4 + 255) / 256 * 256 + (int64_t)n * A * 8 + (int64_t)n * A * 5 * 4;
}

extern "C" int lmx_k_nms(const float* pred, int n, int A, int nc, float conf, double iou, int max_det, float max_wh,
                         float* boxes, float* scores, int32_t* cls, int32_t* src, int32_t* counts, void* workspace,
                         lmx_stream_t stream) {
  LMX_REQUIRE(pred && boxes && scores && cls && src && counts && workspace, "lmx_k_nms: null pointer");
  LMX_REQUIRE(n > 0 && A > 0 && A <= MAX_A && nc > 0 && max_det > 0, "lmx_k_nms: n=%d A=%d (<=%d) nc=%d max_det=%d", n,
              A, MAX_A, nc, max_det);
  LMX_REQUIRE((((uintptr_t)workspace) & 255) == 0, "lmx_k_nms: workspace must be 256-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  int* cand_counts = reinterpret_cast<int*>(ws);
  const int64_t cnt_bytes = ((int64_t)n * 4 + 255) / 256 * 256;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + cnt_bytes);
  float* sbox = reinterpret_cast<float*>(ws + cnt_bytes + (int64_t)n * A * 8);
  LMX_HIP(hipMemsetAsync(cand_counts, 0, (size_t)n * 4, st));
  // 16-byte pieces where every row starts on a 16-byte address; one 256-thread workgroup takes 4 * (64 / L) rows a pass
  const bool vec = (4 + nc) % 4 == 0 && (((uintptr_t)pred) & 15) == 0;
  const int pieces = vec ? (4 + nc) / 4 : 4 + nc;
  const int rows_wg = 4 * (64 / (pieces < 64 ? pieces : 64));
  int64_t g = ((int64_t)n * A + rows_wg - 1) / rows_wg;
  if (g > 2048) g = 2048;
  if (vec)
    hipLaunchKernelGGL(nms_filter_kernel<true>, dim3((unsigned)g), dim3(256), 0, st, pred, n, A, nc, conf, keys, cand_counts);
  else
    hipLaunchKernelGGL(nms_filter_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, pred, n, A, nc, conf, keys, cand_counts);
  int rc = lmx_launch_check("nms_filter_kernel");
  if (rc) return rc;
  int npow2 = 64;
  while (npow2 < A) npow2 <<= 1;
  const size_t smem = (size_t)npow2 * 9 + 64 * sizeof(Box);
  int dev;
  LMX_TRY(lmx_stream_device(st, &dev));
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(&nms_greedy_kernel), (int)((size_t)MAX_A * 9 + 64 * sizeof(Box)), dev));
  hipLaunchKernelGGL(nms_greedy_kernel, dim3(n), dim3(1024), smem, st, pred, A, nc, iou, max_det, max_wh, keys, cand_counts,
                     sbox, boxes, scores, cls, src, counts);
  return lmx_launch_check("nms_greedy_kernel");
}

extern "C" int lmx_k_nms_boxes(const float* boxes, int64_t ldb, const float* scores, const uint8_t* valid, int n, double iou,
                               int32_t* keep_out, int32_t* count_out, void* workspace, lmx_stream_t stream) {
  LMX_REQUIRE(boxes && scores && keep_out && count_out && workspace, "lmx_k_nms_boxes: null pointer");
  LMX_REQUIRE(n > 0 && n <= MAX_A && ldb >= 4, "lmx_k_nms_boxes: n=%d (1..%d) ldb=%lld", n, MAX_A, (long long)ldb);
  LMX_REQUIRE((((uintptr_t)workspace) & 15) == 0, "lmx_k_nms_boxes: workspace must be 16-byte aligned");
  int npow2 = 64;
  while (npow2 < n) npow2 <<= 1;
  const size_t smem = (size_t)npow2 * 9 + 64 * sizeof(Box);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int dev;
  LMX_TRY(lmx_stream_device(st, &dev));
  LMX_TRY(lmx_allow_lds(reinterpret_cast<const void*>(&nms_boxes_kernel), (int)((size_t)MAX_A * 9 + 64 * sizeof(Box)), dev));
  hipLaunchKernelGGL(nms_boxes_kernel, dim3(1), dim3(1024), smem, st, boxes, ldb, scores, valid, n, iou, reinterpret_cast<float*>(workspace),
                     keep_out, count_out);
  return lmx_launch_check("nms_boxes_kernel");
}
