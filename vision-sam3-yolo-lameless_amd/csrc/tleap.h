// tleap.h — what the pose-series kernel (tleap.hip) and its host twin (host_tleap.cpp) share (include/lmx.h "Pose series"): the per-frame
// row count, the row map, one pose record from the detector's outputs (services/tleap-pipeline/app/main.py:173-313) and the checks of a
// call.  Plain C++ without HIP types; both files compile it with -ffp-contract=off: Python rounds after every operation, and a fused
// multiply-add in the heuristics breaks byte parity.
#pragma once
#include "gait.h"

// what a launch reads, by value: the detector's buffers, the frame and the cow classes
struct LmxTleapIn {
  const float* boxes;
  const float* scores;
  const int32_t* cls;
  const int32_t* counts;
  const float* kpts;
  int K, ndim, max_det, h, w, mode, n_cow;
  int32_t cow[LMX_TLEAP_MAX_COW_CLASSES];
};

LMX_GAIT_HD inline int lmx_tleap_count(const LmxTleapIn& in, int f) {
  const int c = in.counts[f];
  return c < 0 ? 0 : (c > in.max_det ? in.max_det : c);
}
LMX_GAIT_HD inline bool lmx_tleap_is_cow(const LmxTleapIn& in, int cls) {
  for (int i = 0; i < in.n_cow; ++i)
    if (in.cow[i] == cls) return true;
  return false;
}
// rows of frame f: every detection (trained), or the cow detections and one assumed row if there is none (heuristic)
LMX_GAIT_HD inline int lmx_tleap_frame_rows(const LmxTleapIn& in, int f) {
  const int c = lmx_tleap_count(in, f);
  if (in.mode == LMX_TLEAP_TRAINED) return c;
  int cows = 0;
  for (int j = 0; j < c; ++j) cows += lmx_tleap_is_cow(in, in.cls[(size_t)f * in.max_det + j]) ? 1 : 0;
  return cows > 0 ? cows : 1;
}
// the detection index of each row of frame f in NMS order (-1: the assumed row), with the frame's index `rel` in its clip; `map` has room
// for lmx_tleap_frame_rows(in, f) pairs
LMX_GAIT_HD inline void lmx_tleap_frame_map(const LmxTleapIn& in, int f, int rel, int32_t* map) {
  const int c = lmx_tleap_count(in, f);
  int k = 0;
  for (int j = 0; j < c; ++j)
    if (in.mode == LMX_TLEAP_TRAINED || lmx_tleap_is_cow(in, in.cls[(size_t)f * in.max_det + j])) {
      map[2 * k] = rel;
      map[2 * k + 1] = j;
      ++k;
    }
  if (k == 0 && in.mode == LMX_TLEAP_HEURISTIC) {
    map[0] = rel;
    map[1] = -1;
  }
}

// main.py:210-263 from the box: x1, y1, x2, y2 are int(c), toward zero
struct LmxTleapBox {
  double x1, y1, x2, y2, width, height;
};
LMX_GAIT_HD inline LmxTleapBox lmx_tleap_box(const double* bbox) {
  const double x1 = trunc(bbox[0]), y1 = trunc(bbox[1]), x2 = trunc(bbox[2]), y2 = trunc(bbox[3]);
  return {x1, y1, x2, y2, x2 - x1, y2 - y1};
}
#define LMX_TLEAP_KP(kp, X, Y, C) ((kp)[0] = (X), (kp)[1] = (Y), (kp)[2] = (C))
LMX_GAIT_HD inline void lmx_tleap_withers(const double* bbox, double* kp) {
  const LmxTleapBox b = lmx_tleap_box(bbox);
  LMX_TLEAP_KP(kp, b.x1 + b.width * 0.3, b.y1 + b.height * 0.15, 0.8);
}
LMX_GAIT_HD inline void lmx_tleap_heuristic(const double* bbox, double (*kp)[3]) {
  const LmxTleapBox b = lmx_tleap_box(bbox);
  const double x1 = b.x1, y1 = b.y1, y2 = b.y2, width = b.width, height = b.height;
  const double head_x = x1 + width * 0.1, head_y = y1 + height * 0.3;
  LMX_TLEAP_KP(kp[0], head_x - width * 0.02, head_y - height * 0.05, 0.7);
  LMX_TLEAP_KP(kp[1], head_x + width * 0.02, head_y - height * 0.05, 0.7);
  LMX_TLEAP_KP(kp[2], head_x, head_y + height * 0.05, 0.8);
  LMX_TLEAP_KP(kp[3], head_x - width * 0.05, head_y - height * 0.1, 0.6);
  LMX_TLEAP_KP(kp[4], head_x + width * 0.05, head_y - height * 0.1, 0.6);
  const double front_x = x1 + width * 0.25;
  LMX_TLEAP_KP(kp[5], front_x - width * 0.05, y1 + height * 0.4, 0.7);
  LMX_TLEAP_KP(kp[6], front_x + width * 0.05, y1 + height * 0.4, 0.7);
  const double back_x = x1 + width * 0.75;
  LMX_TLEAP_KP(kp[7], back_x - width * 0.05, y1 + height * 0.4, 0.7);
  LMX_TLEAP_KP(kp[8], back_x + width * 0.05, y1 + height * 0.4, 0.7);
  LMX_TLEAP_KP(kp[9], front_x - width * 0.03, y1 + height * 0.6, 0.7);
  LMX_TLEAP_KP(kp[10], front_x + width * 0.07, y1 + height * 0.6, 0.7);
  LMX_TLEAP_KP(kp[11], back_x - width * 0.07, y1 + height * 0.6, 0.7);
  LMX_TLEAP_KP(kp[12], back_x + width * 0.03, y1 + height * 0.6, 0.7);
  const double ground_y = y2 - height * 0.05;
  LMX_TLEAP_KP(kp[13], front_x - width * 0.02, ground_y, 0.7);
  LMX_TLEAP_KP(kp[14], front_x + width * 0.08, ground_y, 0.7);
  LMX_TLEAP_KP(kp[15], back_x - width * 0.08, ground_y, 0.7);
  LMX_TLEAP_KP(kp[16], back_x + width * 0.02, ground_y, 0.7);
  LMX_TLEAP_KP(kp[17], x1 + width * 0.15, y1 + height * 0.25, 0.8);
  lmx_tleap_withers(bbox, kp[18]);
  LMX_TLEAP_KP(kp[19], x1 + width * 0.9, y1 + height * 0.25, 0.7);
}

// the record of the row (frame f of the batch, `rel` in its clip, detection `det` or -1)
LMX_GAIT_HD inline void lmx_tleap_record(const LmxTleapIn& in, int f, int rel, int det, lmx_tleap_record_t* r) {
  r->frame = rel;
  r->det = det;
  r->reserved = 0;
  if (det < 0) {
    const double margin = 0.1;
    r->bbox[0] = in.w * margin;
    r->bbox[1] = in.h * margin;
    r->bbox[2] = in.w * (1 - margin);
    r->bbox[3] = in.h * (1 - margin);
    r->confidence = 0.5;
  } else {
    const size_t d = (size_t)f * in.max_det + det;
    for (int i = 0; i < 4; ++i) r->bbox[i] = (double)in.boxes[4 * d + i];
    r->confidence = (double)in.scores[d];
  }
  if (in.mode == LMX_TLEAP_HEURISTIC) {
    r->n_kp = LMX_TLEAP_KEYPOINTS;
    lmx_tleap_heuristic(r->bbox, r->keypoints);
    return;
  }
  const int n_kp = in.K < LMX_TLEAP_KEYPOINTS ? in.K : LMX_TLEAP_KEYPOINTS;
  const float* k = in.kpts + ((size_t)f * in.max_det + det) * in.K * in.ndim;
  r->n_kp = n_kp;
  for (int i = 0; i < LMX_TLEAP_KEYPOINTS; ++i) {
    const bool has = i < n_kp;
    r->keypoints[i][0] = has ? (double)k[i * in.ndim] : 0.0;
    r->keypoints[i][1] = has ? (double)k[i * in.ndim + 1] : 0.0;
    r->keypoints[i][2] = has ? (in.ndim > 2 ? (double)k[i * in.ndim + 2] : 1.0) : 0.0;
  }
  // the one name both lists share: the model's slot 2 is `withers`, the heuristic's withers is its slot 18, written into slot 2 here
  if (!(r->keypoints[2][2] > 0.3)) lmx_tleap_withers(r->bbox, r->keypoints[2]);
}

enum { LMX_TLEAP_MAX_TARGET = 65536, LMX_TLEAP_MAX_K = 4096 };

inline int64_t lmx_tleap_bounds_bytes(int F) { return ((int64_t)F + 2) / 2 * 8; }  // F + 1 clip bounds at most, in whole 8 bytes

// every refusal of include/lmx.h; the launch and the twin check the same list.  On success *in describes the call.
inline int lmx_tleap_check(const char* who, const float* boxes, const float* scores, const int32_t* cls, const int32_t* counts, const float* kpts,
                           int K, int ndim, int F, int max_det, int h, int w, const int32_t* clip_first, int n, int target, int mode,
                           const int32_t* cow, int n_cow, const int32_t* rows, const lmx_tleap_record_t* records, const float* series,
                           const uint8_t* mask, LmxTleapIn* in) {
  GAIT_REQUIRE(F >= 1 && F <= (1 << 24), "%s: F = %d frames", who, F);
  GAIT_REQUIRE(max_det >= 1 && max_det <= (1 << 16), "%s: max_det %d outside 1 .. 65536", who, max_det);
  GAIT_REQUIRE((int64_t)F * max_det <= (1 << 24), "%s: F %d x max_det %d is more than %d rows", who, F, max_det, 1 << 24);
  GAIT_REQUIRE(h >= 1 && w >= 1, "%s: a frame of h %d x w %d", who, h, w);
  GAIT_REQUIRE(n >= 1, "%s: n = %d clips", who, n);
  GAIT_REQUIRE(target >= 1 && target <= LMX_TLEAP_MAX_TARGET, "%s: target %d outside 1 .. %d", who, target, LMX_TLEAP_MAX_TARGET);
  GAIT_REQUIRE(mode == LMX_TLEAP_TRAINED || mode == LMX_TLEAP_HEURISTIC, "%s: mode %d is neither LMX_TLEAP_TRAINED nor LMX_TLEAP_HEURISTIC", who, mode);
  GAIT_REQUIRE(boxes, "%s: null boxes", who);
  GAIT_REQUIRE(scores, "%s: null scores", who);
  GAIT_REQUIRE(cls, "%s: null cls", who);
  GAIT_REQUIRE(counts, "%s: null counts", who);
  GAIT_REQUIRE(rows, "%s: null rows", who);
  GAIT_REQUIRE(records, "%s: null records", who);
  GAIT_REQUIRE(series, "%s: null series", who);
  GAIT_REQUIRE(mask, "%s: null mask", who);
  GAIT_REQUIRE(clip_first, "%s: null clip_first_host", who);
  GAIT_REQUIRE(((uintptr_t)boxes & 3) == 0, "%s: boxes is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)scores & 3) == 0, "%s: scores is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)cls & 3) == 0, "%s: cls is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)counts & 3) == 0, "%s: counts is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)kpts & 3) == 0, "%s: kpts is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)rows & 3) == 0, "%s: rows is not 4-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)records & 7) == 0, "%s: records is not 8-byte aligned", who);
  GAIT_REQUIRE(((uintptr_t)series & 3) == 0, "%s: series is not 4-byte aligned", who);
  if (mode == LMX_TLEAP_TRAINED) {
    GAIT_REQUIRE(kpts, "%s: LMX_TLEAP_TRAINED needs kpts", who);
    GAIT_REQUIRE(ndim == 2 || ndim == 3, "%s: ndim %d is neither 2 nor 3", who, ndim);
    GAIT_REQUIRE(K >= 3 && K <= LMX_TLEAP_MAX_K, "%s: K %d outside 3 .. %d (withers is the model's keypoint 2)", who, K, LMX_TLEAP_MAX_K);
  } else {
    GAIT_REQUIRE(!kpts, "%s: LMX_TLEAP_HEURISTIC takes no kpts", who);
    GAIT_REQUIRE(n_cow >= 0 && n_cow <= LMX_TLEAP_MAX_COW_CLASSES, "%s: n_cow %d outside 0 .. %d", who, n_cow, LMX_TLEAP_MAX_COW_CLASSES);
    GAIT_REQUIRE(cow || n_cow == 0, "%s: null cow_classes_host", who);
  }
  GAIT_REQUIRE(n <= F && clip_first[0] == 0 && clip_first[n] == F, "%s: clip_first_host runs from %d to %d over %d clips, not from 0 to F = %d", who,
               clip_first[0], n <= F ? clip_first[n] : -1, n, F);
  for (int c = 0; c < n; ++c)
    GAIT_REQUIRE(clip_first[c] < clip_first[c + 1], "%s: clip_first_host does not ascend at clip %d (%d then %d)", who, c, clip_first[c],
                 clip_first[c + 1]);
  *in = LmxTleapIn{boxes, scores, cls, counts, kpts, mode == LMX_TLEAP_TRAINED ? K : 0, mode == LMX_TLEAP_TRAINED ? ndim : 0, max_det, h, w, mode,
                   mode == LMX_TLEAP_HEURISTIC ? n_cow : 0, {}};
  for (int i = 0; i < in->n_cow; ++i) in->cow[i] = cow[i];
  return LMX_OK;
}
