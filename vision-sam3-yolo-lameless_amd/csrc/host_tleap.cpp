// host_tleap.cpp — the pose series on the HOST (include/lmx.h "Pose series"): lmx_h_tleap_series, the twin of lmx_k_tleap_series (csrc/tleap.hip)
// over the same tleap.h in plain C++, with lmx_h_tcn_features and lmx_h_xfm_mask for the second half so that their pin stays in one
// place, and lmx_h_tleap_locomotion, compute_locomotion_features of services/tleap-pipeline/app/main.py:338-436 with sequential sums in
// doubles.  No HIP here; the Makefile builds this file with -ffp-contract=off.  tests/tleap_check_main.cpp runs it under the sanitizers.
#include <string.h>

#include <vector>

#include "tleap.h"

extern "C" int lmx_h_tleap_series(const float* boxes, const float* scores, const int32_t* cls, const int32_t* counts, const float* kpts, int K,
                                  int ndim, int F, int max_det, int h, int w, const int32_t* clip_first, int n, int target, int mode,
                                  const int32_t* cow, int n_cow, int32_t* rows, lmx_tleap_record_t* records, float* series, uint8_t* mask) {
  LmxTleapIn in;
  if (const int rc = lmx_tleap_check("lmx_h_tleap_series", boxes, scores, cls, counts, kpts, K, ndim, F, max_det, h, w, clip_first, n, target, mode,
                                     cow, n_cow, rows, records, series, mask, &in))
    return rc;
  const int NK = LMX_TLEAP_KEYPOINTS;
  std::vector<int32_t> map;
  std::vector<double> kp, conf, bbox, det_conf;
  std::vector<int> n_kp;
  for (int c = 0; c < n; ++c) {
    const int f0 = clip_first[c], nf = clip_first[c + 1] - f0;
    lmx_tleap_record_t* rec = records + (size_t)f0 * max_det;
    map.assign((size_t)nf * max_det * 2, 0);
    int T0 = 0;
    for (int rel = 0; rel < nf; ++rel) {
      lmx_tleap_frame_map(in, f0 + rel, rel, map.data() + 2 * (size_t)T0);
      T0 += lmx_tleap_frame_rows(in, f0 + rel);
    }
    rows[c] = T0;
    float* x = series + (size_t)c * target * LMX_GAIT_FEATURES;
    uint8_t* m = mask + (size_t)c * target;
    if (T0 == 0) {  // a trained clip without a detection: a zero series, every step masked
      memset(x, 0, (size_t)target * LMX_GAIT_FEATURES * sizeof(float));
      memset(m, 1, (size_t)target);
      continue;
    }
    kp.resize((size_t)T0 * NK * 2), conf.resize((size_t)T0 * NK), bbox.resize((size_t)T0 * 4), det_conf.resize((size_t)T0), n_kp.resize((size_t)T0);
    for (int r = 0; r < T0; ++r) {
      lmx_tleap_record(in, f0 + map[2 * (size_t)r], map[2 * (size_t)r], map[2 * (size_t)r + 1], rec + r);
      for (int i = 0; i < NK; ++i) {
        kp[((size_t)r * NK + i) * 2] = rec[r].keypoints[i][0];
        kp[((size_t)r * NK + i) * 2 + 1] = rec[r].keypoints[i][1];
        conf[(size_t)r * NK + i] = rec[r].keypoints[i][2];
      }
      memcpy(&bbox[4 * (size_t)r], rec[r].bbox, 4 * sizeof(double));
      det_conf[r] = rec[r].confidence;
      n_kp[r] = rec[r].n_kp;
    }
    if (const int rc = lmx_h_tcn_features(kp.data(), n_kp.data(), bbox.data(), T0, target, x)) return rc;
    if (const int rc = lmx_h_xfm_mask(conf.data(), n_kp.data(), det_conf.data(), T0, target, m)) return rc;
  }
  return LMX_OK;
}

namespace {

double mean_of(const std::vector<double>& v) {
  double s = 0.0;
  for (double x : v) s += x;
  return s / (double)v.size();
}
double std_of(const std::vector<double>& v) {  // np.std: the population's
  const double m = mean_of(v);
  double s = 0.0;
  for (double x : v) s += (x - m) * (x - m);
  return sqrt(s / (double)v.size());
}
std::vector<double> diff_of(const std::vector<double>& v) {
  std::vector<double> d;
  for (size_t i = 1; i < v.size(); ++i) d.push_back(v[i] - v[i - 1]);
  return d;
}
double sign_of(double v) { return v > 0 ? 1.0 : (v < 0 ? -1.0 : v); }  // np.sign: 0 stays 0, NaN stays NaN

}  // namespace

extern "C" int lmx_h_tleap_locomotion(const lmx_tleap_record_t* rec, int rows, const char* const* names, lmx_tleap_locomotion_t* out) {
  GAIT_REQUIRE(rows >= 0 && rows <= (1 << 24), "lmx_h_tleap_locomotion: rows = %d", rows);
  GAIT_REQUIRE(rec || rows == 0, "lmx_h_tleap_locomotion: null records_host");
  GAIT_REQUIRE(names, "lmx_h_tleap_locomotion: null names_host");
  GAIT_REQUIRE(out, "lmx_h_tleap_locomotion: null out_host");
  const int NK = LMX_TLEAP_KEYPOINTS;
  for (int i = 0; i < NK; ++i) GAIT_REQUIRE(names[i], "lmx_h_tleap_locomotion: names_host[%d] is null", i);
  memset(out, 0, sizeof(*out));
  if (rows < 2) return LMX_OK;
  // the slot of each name the features read: the last slot that carries it, as the reference's dict keeps the last
  static const char* const kWanted[8] = {"nose", "throat", "withers", "tailbase", "left_front_paw", "right_front_paw", "left_back_paw", "right_back_paw"};
  int slot[8];
  for (int k = 0; k < 8; ++k) {
    slot[k] = -1;
    for (int i = 0; i < NK; ++i)
      if (strcmp(names[i], kWanted[k]) == 0) slot[k] = i;
  }
  std::vector<double> head, angles, hoof[4];
  for (int r = 0; r < rows; ++r) {
    if (rec[r].n_kp < NK) continue;  // main.py:360
    auto kp = [&](int k) { return slot[k] >= 0 ? rec[r].keypoints[slot[k]] : nullptr; };
    auto seen = [&](int k) { return kp(k) && kp(k)[2] > 0.3; };
    if (seen(0)) head.push_back(kp(0)[1]);
    if (seen(1) && seen(2) && seen(3)) {
      const double *t = kp(1), *w = kp(2), *b = kp(3);
      const double v1x = t[0] - w[0], v1y = t[1] - w[1], v2x = b[0] - w[0], v2y = b[1] - w[1];
      const double dot = v1x * v2x + v1y * v2y;
      const double n1 = sqrt(v1x * v1x + v1y * v1y), n2 = sqrt(v2x * v2x + v2y * v2y);
      double cosine = dot / (n1 * n2 + 1e-6);
      cosine = cosine < -1 ? -1 : (cosine > 1 ? 1 : cosine);
      angles.push_back(acos(cosine) * (180.0 / M_PI));
    }
    for (int l = 0; l < 4; ++l)
      if (seen(4 + l)) hoof[l].push_back(kp(4 + l)[0]);
  }
  double* v = &out->back_arch_mean;  // the 17 fields in order: bit i of `present` is field i
  auto set = [&](int i, double x) {
    v[i] = x;
    out->present |= 1u << i;
  };
  auto has = [&](int i) { return (out->present >> i & 1u) != 0; };
  if (!angles.empty()) {
    set(0, mean_of(angles));
    set(1, std_of(angles));
    set(2, 1.0 - mean_of(angles) / 180.0);
  }
  if (head.size() > 1) {
    set(3, std_of(head));
    const std::vector<double> d = diff_of(head);
    double turns = 0.0;
    for (size_t i = 1; i < d.size(); ++i) turns += fabs(sign_of(d[i]) - sign_of(d[i - 1]));
    set(4, turns / 2);
    set(5, v[3] / 50.0 < 1.0 ? v[3] / 50.0 : 1.0);
  }
  for (int l = 0; l < 4; ++l)
    if (hoof[l].size() > 1) {
      std::vector<double> strides = diff_of(hoof[l]), mags;
      for (double s : strides) mags.push_back(fabs(s));
      set(6 + 2 * l, mean_of(mags));
      set(7 + 2 * l, std_of(strides));
    }
  if (has(6) && has(8)) set(14, fabs(v[6] - v[8]) / (v[6] + v[8] + 1e-6));
  if (has(10) && has(12)) set(15, fabs(v[10] - v[12]) / (v[10] + v[12] + 1e-6));
  double sum = 0.0;
  int parts = 0;
  for (int i : {2, 5, 14, 15})
    if (has(i)) sum += v[i], ++parts;
  if (parts) set(16, sum / parts);
  return LMX_OK;
}
