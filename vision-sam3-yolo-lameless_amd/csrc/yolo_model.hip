// yolo_model.hip — the model-level entry points of the C-ABI for YOLOv8: a handle (model_handle.h has what every handle owns) with the
// weights of one weight image (yolo_image.h) and, per prepared (frame size, plan), the workspace of one batch; lmx_yolo_predict /
// lmx_yolo_detect are the launch sequence of lmx/yolo.py's YoloDetector (preprocess + forward_letterboxed + nms + scale_boxes
// (+ pose_gather); services/yolo-pipeline/app/main.py:76, services/tleap-pipeline/app/main.py:150) written as host C++.
// HOST code only: there is no kernel in this file.  Every launch goes through the same extern "C" lmx_k_* entry point the ctypes
// binding calls, with the descriptor filled as lmx/kernels.py fills it, so the outputs are the Python plan's bit for bit on both
// precision plans (tests/test_gpu_native_yolo.py).
// The plan is written ONCE (forward) over a Run, a run of plan_run.h: lmx_yolo_prepare walks it counting, which sizes the plan's
// arena and the one f32 region of the exact plan, and every call walks it launching over the same offsets.  lmx_k_gemm itself checks
// "smaller than 2 GB" for pooled rows (a_mode 2) only; for the dense and convolution launches this plan makes (a_mode 0 / 1) the
// run's refusal of a buffer of 2 GB or more is the only guard: it is not redundant.
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "model_handle.h"
#include "yolo_image.h"

namespace {

const float NMS_MAX_WH = 7680.f;

// one convolution's operands under one plan
struct ConvW {
  const void* w = nullptr;
  const float *b = nullptr, *s = nullptr;  // s: the exact plan's row scale
  int cout = 0, K = 0;                     // K: the columns of w
};

// an NHWC view of (a channel slice of) a workspace buffer: offset from the plan arena's base, C channels of esz bytes, pixel stride ps
struct Act {
  size_t off = 0;
  int H = 0, W = 0, C = 0, esz = 2;
  int64_t ps = 0;
};

Act slice(const Act& a, int c0, int c1) {
  Act s = a;
  s.off += (size_t)c0 * a.esz;
  s.C = c1 - c0;
  return s;
}

// what lmx_yolo_prepare builds for one (frame size, plan): geometry, tables and the workspace of max_batch frames, one allocation
struct Prepared {
  lmx_letterbox_geo_t geo;
  int A = 0;
  char* blob = nullptr;
  int32_t *xofs = nullptr, *yofs = nullptr;  // null: the frame keeps its size, lmx_k_letterbox skips the resize
  int16_t *ialpha = nullptr, *ibeta = nullptr;
  uint8_t* boxed = nullptr;  // letterboxed frames u8 [max_batch, oh, ow, 3]
  float* pred = nullptr;     // [max_batch, A, 4 + nc]
  void* nms_ws = nullptr;
  LmxArena plan, scratch;    // the plan's buffers and the f32 region of the exact plan, as the counting walk sized them
};

}  // namespace

struct lmx_yolo : LmxHandleCore {
  LmxYoloImage img;
  const float *stem_w = nullptr, *stem_b = nullptr;
  std::map<std::string, ConvW> conv[2];  // per plan (LMX_YOLO_F16, LMX_YOLO_EXACT)
  std::map<std::tuple<int, int, int>, Prepared> prepared;
};

namespace {

// the plan's view of one launch sequence: counting (at prepare: enqueue nothing) or launching n <= max_batch frames
struct Run : LmxPlanRun {
  const lmx_yolo* m;
  int precision, cm;  // cm: stored f16 channels per logical channel (1, or 3 for the exact plan's x3 triples)
  int n;
  LmxArena plan, scratch;
  hipStream_t stream() const { return lmx_run_stream(*this); }

  Run(const lmx_yolo* m_, int precision_, const char* fn_) : m(m_), precision(precision_), cm(precision_ == LMX_YOLO_EXACT ? 3 : 1), n(0) {
    fn = fn_, model = "YOLOv8", kernels = "GEMM kernels";
  }
  void* at(const Act& a) const { return plan.base + a.off; }

  // [max_batch, H, W, C] of esz-byte elements: every call finds a buffer where the count put it, whatever its n
  int alloc(int H, int W, int C, int esz, const char* what, Act* out) {
    *out = Act{plan.at, H, W, C, esz, C};
    void* p;
    return take(&plan, what, (int64_t)m->max_batch * H * W * C * esz, &p);
  }
  // the f32 output of an exact-plan convolution (parts partial sums): consumed by the lmx_k_split3 enqueued right behind it, so one
  // region serves them all in stream order
  int scratch_for(int parts, int H, int W, int C, const char* what, float** out) {
    return share(&scratch, what, (int64_t)parts * m->max_batch * H * W * C * 4, out);
  }
  int weights(const std::string& name, const ConvW** w) const {
    const auto it = m->conv[precision].find(name);
    LMX_REQUIRE(it != m->conv[precision].end(), "lmx_yolo: no convolution '%s' in the image", name.c_str());
    *w = &it->second;
    return LMX_OK;
  }
};

// K.gemm / K.conv1x1: a 1 x 1 convolution over the pixels of x
int gemm1(Run& r, const Act& x, const ConvW& w, int act, const float* scale, void* C, int64_t ldc, int out_dtype) {
  LMX_REQUIRE(w.K == x.C, "lmx_yolo: a 1 x 1 convolution with %d weight columns reads %d channels", w.K, x.C);
  if (!r.launch) return LMX_OK;
  return lmx_gemm_dense(r.at(x), x.ps, w.w, w.b, C, ldc, out_dtype, r.n * x.H * x.W, w.cout, x.C, act, scale, nullptr, 0, r.stream());
}

// K.conv3x3: 3 x 3 / pad 1 as implicit GEMM
int gemm3(Run& r, const Act& x, const ConvW& w, int act, int stride, const float* scale, const Act* res, void* C, int64_t ldc, int out_dtype,
          int split_k) {
  LMX_REQUIRE(w.K == 9 * x.C, "lmx_yolo: a 3 x 3 convolution with %d weight columns reads %d channels", w.K, x.C);
  if (!r.launch) return LMX_OK;
  return lmx_gemm_conv3(r.at(x), x.ps, r.n, x.H, x.W, x.C, w.w, w.b, scale, C, ldc, out_dtype, w.cout, act, stride, res ? r.at(*res) : nullptr,
                        res ? res->ps : 0, split_k, r.stream());
}

// P.conv3: Conv(k3) + SiLU (+ shortcut).  out_in: the consumer's slice to write into, or null for a buffer of the convolution's own
// (x by value: callers chain `conv3(r, t, ..., &t)`)
int conv3(Run& r, const Act x, const std::string& name, int stride, const Act* res, const Act* out_in, Act* out) {
  const ConvW* w;
  LMX_TRY(r.weights(name, &w));
  const int Ho = (x.H - 1) / stride + 1, Wo = (x.W - 1) / stride + 1;
  Act o;
  if (out_in)
    o = *out_in;
  else
    LMX_TRY(r.alloc(Ho, Wo, r.cm * w->cout, 2, name.c_str(), &o));
  LMX_REQUIRE(o.H == Ho && o.W == Wo && o.C == r.cm * w->cout, "lmx_yolo: '%s' writes [%d, %d, %d] into a slice of [%d, %d, %d]", name.c_str(), Ho, Wo,
              r.cm * w->cout, o.H, o.W, o.C);
  if (out) *out = o;
  if (r.precision == LMX_YOLO_F16) return gemm3(r, x, *w, LMX_ACT_SILU, stride, nullptr, res, r.launch ? r.at(o) : nullptr, o.ps, LMX_F16, 1);
  // exact: the factor depends on the layer only (pixels of ONE frame), so a frame's bits do not depend on the batch it rides in
  const int sk = lmx_h_conv_split_k((int64_t)Ho * Wo, w->cout, w->K, x.C);
  LMX_REQUIRE(sk >= 1, "lmx_yolo: split factor of '%s'", name.c_str());
  float* acc;
  LMX_TRY(r.scratch_for(sk, Ho, Wo, w->cout, name.c_str(), &acc));
  LMX_TRY(gemm3(r, x, *w, LMX_ACT_NONE, stride, w->s, nullptr, acc, w->cout, LMX_F32, sk));
  if (!r.launch) return LMX_OK;
  return lmx_k_split3(acc, w->cout, LMX_ACT_SILU, res ? r.at(*res) : nullptr, res ? res->ps : 0, r.at(o), o.ps, (int64_t)r.n * Ho * Wo,
                      w->cout, w->cout, sk, sk > 1 ? (int64_t)r.n * Ho * Wo * w->cout : 0, r.stream());
}

// P.conv1: Conv(k1) + SiLU into `out` (a slice of the consumer's buffer); g_out: the x3 group width of the output (0: all channels)
int conv1(Run& r, const Act& x, const std::string& name, const Act& out, int g_out) {
  const ConvW* w;
  LMX_TRY(r.weights(name, &w));
  LMX_REQUIRE(out.H == x.H && out.W == x.W && out.C == r.cm * w->cout, "lmx_yolo: '%s' writes [%d, %d, %d] into a slice of [%d, %d, %d]", name.c_str(),
              x.H, x.W, r.cm * w->cout, out.H, out.W, out.C);
  if (r.precision == LMX_YOLO_F16) return gemm1(r, x, *w, LMX_ACT_SILU, nullptr, r.launch ? r.at(out) : nullptr, out.ps, LMX_F16);
  float* acc;
  LMX_TRY(r.scratch_for(1, x.H, x.W, w->cout, name.c_str(), &acc));
  LMX_TRY(gemm1(r, x, *w, LMX_ACT_NONE, w->s, acc, w->cout, LMX_F32));
  if (!r.launch) return LMX_OK;
  return lmx_k_split3(acc, w->cout, LMX_ACT_SILU, nullptr, 0, r.at(out), out.ps, (int64_t)r.n * x.H * x.W, w->cout, g_out ? g_out : w->cout, 1,
                      0, r.stream());
}

// P.head: the plain Conv2d(c, n_out, 1) that ends a Detect / Pose branch: f32 out, no activation
int head(Run& r, const Act& x, const std::string& name, const Act& out) {
  const ConvW* w;
  LMX_TRY(r.weights(name, &w));
  LMX_REQUIRE(out.H == x.H && out.W == x.W && out.C == w->cout && out.esz == 4, "lmx_yolo: '%s' writes %d f32 channels into a slice of %d", name.c_str(),
              w->cout, out.C);
  return gemm1(r, x, *w, LMX_ACT_NONE, r.precision == LMX_YOLO_EXACT ? w->s : nullptr, r.launch ? r.at(out) : nullptr, out.ps, LMX_F32);
}

int pool5(Run& r, const Act& x, const Act& out) {
  if (!r.launch) return LMX_OK;
  if (r.precision == LMX_YOLO_F16) return lmx_k_maxpool5(r.at(x), x.ps, r.at(out), out.ps, r.n, x.H, x.W, x.C, r.stream());
  return lmx_k_maxpool5_x3(r.at(x), x.ps, r.at(out), out.ps, r.n, x.H, x.W, x.C / 3, r.stream());
}

int up2(Run& r, const Act& x, const Act& out) {
  LMX_REQUIRE(out.H == 2 * x.H && out.W == 2 * x.W && out.C == x.C, "lmx_yolo: upsample of [%d, %d, %d] into a slice of [%d, %d, %d]", x.H, x.W, x.C, out.H,
              out.W, out.C);
  if (!r.launch) return LMX_OK;
  return lmx_k_upsample2(r.at(x), x.ps, r.at(out), out.ps, r.n, x.H, x.W, x.C, r.stream());
}

// YoloDetector._c2f: ONE buffer [H, W, (2 + nb) c]; cv1 writes channels [0, 2c), each bottleneck reads the previous c-wide slice and
// writes the next one, cv2 is a 1 x 1 GEMM over the whole buffer
int c2f(Run& r, int i, const Act& x, const Act& out) {
  const LmxYoloModule& m = r.m->img.table[(size_t)i];
  const std::string p = "model." + std::to_string(i);
  const int c = m.c2 / 2, cm = r.cm;
  Act buf, tmp;
  LMX_TRY(r.alloc(x.H, x.W, cm * (2 + m.n) * c, 2, (p + " (C2f buffer)").c_str(), &buf));
  LMX_TRY(conv1(r, x, p + ".cv1", slice(buf, 0, cm * 2 * c), c));
  LMX_TRY(r.alloc(x.H, x.W, cm * c, 2, (p + " (bottleneck)").c_str(), &tmp));
  for (int j = 0; j < m.n; ++j) {
    const Act src = slice(buf, cm * (1 + j) * c, cm * (2 + j) * c), dst = slice(buf, cm * (2 + j) * c, cm * (3 + j) * c);
    const std::string b = p + ".m." + std::to_string(j);
    LMX_TRY(conv3(r, src, b + ".cv1", 1, nullptr, &tmp, nullptr));
    LMX_TRY(conv3(r, tmp, b + ".cv2", 1, m.shortcut ? &src : nullptr, &dst, nullptr));
  }
  return conv1(r, buf, p + ".cv2", out, 0);
}

// YoloDetector._sppf
int sppf(Run& r, int i, const Act& x, const Act& out) {
  const LmxYoloModule& m = r.m->img.table[(size_t)i];
  const std::string p = "model." + std::to_string(i);
  const int c_ = m.c1 / 2, cm = r.cm;
  Act buf;
  LMX_TRY(r.alloc(x.H, x.W, cm * 4 * c_, 2, (p + " (SPPF buffer)").c_str(), &buf));
  LMX_TRY(conv1(r, x, p + ".cv1", slice(buf, 0, cm * c_), 0));
  for (int j = 0; j < 3; ++j) LMX_TRY(pool5(r, slice(buf, cm * j * c_, cm * (j + 1) * c_), slice(buf, cm * (j + 1) * c_, cm * (j + 2) * c_)));
  return conv1(r, buf, p + ".cv2", out, 0);
}

// YoloDetector.forward_letterboxed: u8 RGB letterboxed [n, H, W, 3] -> pred f32 [n, A, 4 + nc]; kraw: the Pose branch's three levels
int forward(Run& r, const uint8_t* boxed, int H, int W, float* pred, Act kraw[3]) {
  const lmx_yolo* m = r.m;
  const LmxYoloCfg& cfg = m->img.cfg;
  const std::vector<LmxYoloModule>& T = m->img.table;
  const int cm = r.cm;
  auto buf = [&](int h, int w, int c, const char* what, Act* a) { return r.alloc(h, w, cm * c, 2, what, a); };
  const int H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
  // concat buffers (producer slices): cat11 = [up(9) | 6], cat14 = [up(12) | 4], cat17 = [16 | 12], cat20 = [19 | 9]
  const int c4 = T[4].c2, c6 = T[6].c2, c9 = T[9].c2, c12 = T[12].c2, c16 = T[16].c2, c19 = T[19].c2;
  Act cat11, cat14, cat17, cat20, x, t, b2, b8, p3, p4, p5;
  LMX_TRY(buf(H16, W16, c9 + c6, "cat11", &cat11));
  LMX_TRY(buf(H8, W8, c12 + c4, "cat14", &cat14));
  LMX_TRY(buf(H16, W16, c16 + c12, "cat17", &cat17));
  LMX_TRY(buf(H32, W32, c19 + c9, "cat20", &cat20));
  const Act x4 = slice(cat14, cm * c12, cm * (c12 + c4)), x6 = slice(cat11, cm * c9, cm * (c9 + c6)), x9 = slice(cat20, cm * c19, cm * (c19 + c9)),
            x12 = slice(cat17, cm * c16, cm * (c16 + c12));
  LMX_TRY(buf((H - 1) / 2 + 1, (W - 1) / 2 + 1, T[0].c2, "model.0", &x));                                  // 0
  if (r.launch) {
    if (r.precision == LMX_YOLO_F16)
      LMX_TRY(lmx_k_stem_conv(boxed, m->stem_w, m->stem_b, r.at(x), r.n, H, W, T[0].c2, r.stream()));
    else
      LMX_TRY(lmx_k_stem_conv_x3(boxed, m->stem_w, m->stem_b, r.at(x), r.n, H, W, T[0].c2, r.stream()));
  }
  LMX_TRY(conv3(r, x, "model.1", 2, nullptr, nullptr, &x));                                                // 1
  LMX_TRY(buf(H / 4, W / 4, T[2].c2, "model.2", &b2));
  LMX_TRY(c2f(r, 2, x, b2));                                                                                // 2
  LMX_TRY(conv3(r, b2, "model.3", 2, nullptr, nullptr, &x));                                               // 3
  LMX_TRY(c2f(r, 4, x, x4));                                                                                // 4 -> cat14
  LMX_TRY(conv3(r, x4, "model.5", 2, nullptr, nullptr, &x));                                               // 5
  LMX_TRY(c2f(r, 6, x, x6));                                                                                // 6 -> cat11
  LMX_TRY(conv3(r, x6, "model.7", 2, nullptr, nullptr, &x));                                               // 7
  LMX_TRY(buf(H32, W32, T[8].c2, "model.8", &b8));
  LMX_TRY(c2f(r, 8, x, b8));                                                                                // 8
  LMX_TRY(sppf(r, 9, b8, x9));                                                                              // 9 -> cat20
  LMX_TRY(up2(r, x9, slice(cat11, 0, cm * c9)));                                                            // 10, 11
  LMX_TRY(c2f(r, 12, cat11, x12));                                                                          // 12 -> cat17
  LMX_TRY(up2(r, x12, slice(cat14, 0, cm * c12)));                                                          // 13, 14
  LMX_TRY(buf(H8, W8, T[15].c2, "model.15", &p3));
  LMX_TRY(c2f(r, 15, cat14, p3));                                                                           // 15
  const Act s16 = slice(cat17, 0, cm * c16), s19 = slice(cat20, 0, cm * c19);
  LMX_TRY(conv3(r, p3, "model.16", 2, nullptr, &s16, nullptr));                                            // 16, 17
  LMX_TRY(buf(H16, W16, T[18].c2, "model.18", &p4));
  LMX_TRY(c2f(r, 18, cat17, p4));                                                                           // 18
  LMX_TRY(conv3(r, p4, "model.19", 2, nullptr, &s19, nullptr));                                            // 19, 20
  LMX_TRY(buf(H32, W32, T[21].c2, "model.21", &p5));
  LMX_TRY(c2f(r, 21, cat20, p5));                                                                           // 21
  // Detect
  const int A = H8 * W8 + H16 * W16 + H32 * W32, ldh = 64 + cfg.nc_pad;
  const Act* feats[3] = {&p3, &p4, &p5};
  const float strides[3] = {8.f, 16.f, 32.f};
  int a_off = 0;
  for (int l = 0; l < 3; ++l) {
    const Act& feat = *feats[l];
    const std::string p = "model.22", s = "." + std::to_string(l);
    Act hd;
    LMX_TRY(r.alloc(feat.H, feat.W, ldh, 4, "Detect head", &hd));
    LMX_TRY(conv3(r, feat, p + ".cv2" + s + ".0", 1, nullptr, nullptr, &t));
    LMX_TRY(conv3(r, t, p + ".cv2" + s + ".1", 1, nullptr, nullptr, &t));
    LMX_TRY(head(r, t, p + ".cv2" + s + ".2", slice(hd, 0, 64)));
    LMX_TRY(conv3(r, feat, p + ".cv3" + s + ".0", 1, nullptr, nullptr, &t));
    LMX_TRY(conv3(r, t, p + ".cv3" + s + ".1", 1, nullptr, nullptr, &t));
    LMX_TRY(head(r, t, p + ".cv3" + s + ".2", slice(hd, 64, ldh)));
    if (r.launch)
      LMX_TRY(lmx_k_detect_decode(static_cast<const float*>(r.at(hd)), ldh, pred, r.n, feat.H, feat.W, cfg.nc, strides[l], a_off, A, r.stream()));
    a_off += feat.H * feat.W;
    if (cfg.kpt_k) {
      LMX_TRY(conv3(r, feat, p + ".cv4" + s + ".0", 1, nullptr, nullptr, &t));
      LMX_TRY(conv3(r, t, p + ".cv4" + s + ".1", 1, nullptr, nullptr, &t));
      LMX_TRY(r.alloc(feat.H, feat.W, cfg.nk_pad, 4, "Pose head", &kraw[l]));
      LMX_TRY(head(r, t, p + ".cv4" + s + ".2", kraw[l]));
    }
  }
  return LMX_OK;
}

void destroy(lmx_yolo* m) {
  for (auto& kv : m->prepared) (void)hipFree(kv.second.blob);
  lmx_handle_free(m);
  delete m;
}

int open_into(lmx_yolo* m, const char* path) {
  LMX_TRY(lmx_yolo_image_parse(path, &m->img));
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_yolo_open_host", path, m->img.data_offset, m->img.file_bytes));
  const uint64_t base = m->img.data_offset;
  auto at = [&](const LmxTensorRef& r) -> const void* { return r.nbytes ? m->weights + (r.offset - base) : nullptr; };
  auto f32 = [&](const LmxTensorRef& r) { return static_cast<const float*>(at(r)); };
  m->stem_w = f32(m->img.stem_w);
  m->stem_b = f32(m->img.stem_b);
  for (const LmxYoloConv& c : m->img.convs) {
    const int K = c.k * c.k * c.cin;
    if (c.w.nbytes) m->conv[LMX_YOLO_F16][c.name] = ConvW{at(c.w), f32(c.b), nullptr, c.cout, K};
    if (c.xw.nbytes) m->conv[LMX_YOLO_EXACT][c.name] = ConvW{at(c.xw), f32(c.xb), f32(c.xs), c.cout, 3 * K};
  }
  return LMX_OK;
}

int check_precision(const lmx_yolo* m, const char* fn, int precision) {
  LMX_REQUIRE(precision == LMX_YOLO_F16 || precision == LMX_YOLO_EXACT, "%s: precision %d is neither LMX_YOLO_F16 (0) nor LMX_YOLO_EXACT (1)", fn, precision);
  LMX_REQUIRE(m->img.cfg.plans & (1 << precision), "%s: the image does not hold the %s plan (plans mask %d)", fn,
              precision == LMX_YOLO_F16 ? "f16" : "exact", m->img.cfg.plans);
  return LMX_OK;
}

int geometry(const lmx_yolo* m, int h, int w, lmx_letterbox_geo_t* geo, int* A) {
  LMX_TRY(lmx_h_letterbox_geometry(h, w, m->img.cfg.imgsz, 32, 1, geo));
  LMX_REQUIRE(geo->oh % 32 == 0 && geo->ow % 32 == 0, "lmx_yolo: a %d x %d frame letterboxes to %d x %d, not multiples of 32", h, w, geo->oh, geo->ow);
  *A = (geo->oh / 8) * (geo->ow / 8) + (geo->oh / 16) * (geo->ow / 16) + (geo->oh / 32) * (geo->ow / 32);
  return LMX_OK;
}

int prepare(lmx_yolo* m, int h, int w, int precision, const Prepared** out) {
  const auto key = std::make_tuple(h, w, precision);
  const auto it = m->prepared.find(key);
  if (it != m->prepared.end()) {
    if (out) *out = &it->second;
    return LMX_OK;
  }
  LMX_TRY(check_precision(m, "lmx_yolo_prepare", precision));
  Prepared P;
  LMX_TRY(geometry(m, h, w, &P.geo, &P.A));
  LMX_REQUIRE((int)m->prepared.size() < LMX_MAX_PREPARED,
              "lmx_yolo_prepare: the handle already holds %d (frame size, plan) pairs; open another for more", LMX_MAX_PREPARED);
  const lmx_letterbox_geo_t& g = P.geo;
  const bool resize = g.rh != h || g.rw != w;
  std::vector<int32_t> xofs, yofs;
  std::vector<int16_t> ialpha, ibeta;
  if (resize) {
    xofs.resize((size_t)g.rw);
    ialpha.resize((size_t)g.rw * 2);
    yofs.resize((size_t)g.rh);
    ibeta.resize((size_t)g.rh * 2);
    LMX_TRY(lmx_h_letterbox_tables(h, w, g.rh, g.rw, xofs.data(), ialpha.data(), yofs.data(), ibeta.data()));
  }
  // the plan, counted: the bytes of its buffers and of its f32 region
  Run r(m, precision, "lmx_yolo_prepare");
  Act kraw[3];
  LMX_TRY(forward(r, nullptr, g.oh, g.ow, nullptr, kraw));
  const int64_t B = m->max_batch, row = 4 + m->img.cfg.nc;
  const int64_t boxed_bytes = B * g.oh * g.ow * 3, pred_bytes = B * P.A * row * 4, nms_bytes = lmx_nms_workspace_bytes(m->max_batch, P.A);
  LMX_REQUIRE(boxed_bytes < LMX_MAX_BUFFER_BYTES && pred_bytes < LMX_MAX_BUFFER_BYTES,
              "lmx_yolo_prepare: buffer '%s' of %lld bytes for max_batch %d is beyond 2 GB", boxed_bytes < LMX_MAX_BUFFER_BYTES ? "pred" : "letterboxed frames",
              (long long)(boxed_bytes < LMX_MAX_BUFFER_BYTES ? pred_bytes : boxed_bytes), m->max_batch);
  LMX_REQUIRE(nms_bytes > 0, "lmx_yolo_prepare: lmx_nms_workspace_bytes(%d, %d) = %lld", m->max_batch, P.A, (long long)nms_bytes);
  LmxLayout lay;
  const LmxUpload up[4] = {{lay.add(xofs.size() * 4), xofs.data(), xofs.size() * 4},
                           {lay.add(ialpha.size() * 2), ialpha.data(), ialpha.size() * 2},
                           {lay.add(yofs.size() * 4), yofs.data(), yofs.size() * 4},
                           {lay.add(ibeta.size() * 2), ibeta.data(), ibeta.size() * 2}};
  const size_t o_boxed = lay.add((size_t)boxed_bytes), o_pred = lay.add((size_t)pred_bytes), o_nms = lay.add((size_t)nms_bytes),
               o_plan = lay.add(r.plan.peak), o_scratch = lay.add(r.scratch.peak);
  LMX_TRY(lmx_alloc_and_upload(lay.total, up, 4, &P.blob));
  if (resize) {
    P.xofs = reinterpret_cast<int32_t*>(P.blob + up[0].at);
    P.ialpha = reinterpret_cast<int16_t*>(P.blob + up[1].at);
    P.yofs = reinterpret_cast<int32_t*>(P.blob + up[2].at);
    P.ibeta = reinterpret_cast<int16_t*>(P.blob + up[3].at);
  }
  P.boxed = reinterpret_cast<uint8_t*>(P.blob + o_boxed);
  P.pred = reinterpret_cast<float*>(P.blob + o_pred);
  P.nms_ws = P.blob + o_nms;
  P.plan.base = P.blob + o_plan, P.plan.cap = r.plan.peak;
  P.scratch.base = P.blob + o_scratch, P.scratch.cap = r.scratch.peak;
  const auto ins = m->prepared.emplace(key, P);
  if (out) *out = &ins.first->second;
  return LMX_OK;
}

// preprocess + forward_letterboxed for nb <= max_batch frames: pred f32 [nb, A, 4 + nc]
int predict_chunk(const lmx_yolo* m, const Prepared& P, const char* fn, int precision, const uint8_t* frames, int nb, int h, int w, float* pred,
                  Act kraw[3], hipStream_t st) {
  const lmx_letterbox_geo_t& g = P.geo;
  LMX_TRY(lmx_k_letterbox(frames, P.boxed, nb, h, w, g.rh, g.rw, g.top, g.left, g.oh, g.ow, P.xofs, P.ialpha, P.yofs, P.ibeta, 1, st));
  Run r(m, precision, fn);
  r.launch = true, r.n = nb, r.st = st;
  r.plan = P.plan, r.scratch = P.scratch;
  return forward(r, P.boxed, g.oh, g.ow, pred, kraw);
}

// detect / detect_pose for nb <= max_batch frames, writing the chunk's rows of the outputs
int detect_chunk(const lmx_yolo* m, const Prepared& P, const char* fn, int precision, const uint8_t* frames, int nb, int h, int w, float conf, double iou, int max_det,
                 float* boxes, float* scores, int32_t* cls, int32_t* src, int32_t* counts, float* kpts, hipStream_t st) {
  const LmxYoloCfg& c = m->img.cfg;
  const lmx_letterbox_geo_t& g = P.geo;
  Act kraw[3];
  LMX_TRY(predict_chunk(m, P, fn, precision, frames, nb, h, w, P.pred, kraw, st));
  // K.nms's torch.zeros / torch.full(-1): lmx_k_nms leaves rows beyond counts untouched
  const size_t rows = (size_t)nb * max_det;
  LMX_HIP(hipMemsetAsync(boxes, 0, rows * 16, st));
  LMX_HIP(hipMemsetAsync(scores, 0, rows * 4, st));
  LMX_HIP(hipMemsetAsync(cls, 0, rows * 4, st));
  LMX_HIP(hipMemsetAsync(src, 0xff, rows * 4, st));
  LMX_HIP(hipMemsetAsync(counts, 0, (size_t)nb * 4, st));
  LMX_TRY(lmx_k_nms(P.pred, nb, P.A, c.nc, conf, iou, max_det, NMS_MAX_WH, boxes, scores, cls, src, counts, P.nms_ws, st));
  LMX_TRY(lmx_k_scale_boxes(boxes, (int)rows, (float)g.pad_x, (float)g.pad_y, (float)g.gain, (float)g.sw, (float)g.sh, st));
  if (!c.kpt_k) return LMX_OK;
  // ops.scale_coords subtracts the UNROUNDED padding (scale_boxes rounds it like LetterBox does)
  const double gx = g.sw * g.gain, gy = g.sh * g.gain;
  const double padx = (g.ow - gx) / 2, pady = (g.oh - gy) / 2;
  const int32_t hw[6] = {g.oh / 8, g.ow / 8, g.oh / 16, g.ow / 16, g.oh / 32, g.ow / 32};
  const float strides[3] = {8.f, 16.f, 32.f};
  auto raw = [&](int l) { return reinterpret_cast<const float*>(P.plan.base + kraw[l].off); };
  return lmx_k_pose_gather(raw(0), raw(1), raw(2), c.nk_pad, hw, strides, src, counts, nb, max_det, c.kpt_k, c.kpt_ndim, (float)padx, (float)pady,
                           (float)g.gain, (float)g.sw, (float)g.sh, kpts, st);
}

int check_frames(const lmx_yolo* m, const char* fn, const void* frames, int n, int h, int w, int precision) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0, "%s: n = %d frames", fn, n);
  LMX_REQUIRE(h > 0 && w > 0, "%s: frame size %d x %d", fn, h, w);
  LMX_REQUIRE(frames != nullptr, "%s: null pointer (frames)", fn);
  return check_precision(m, fn, precision);
}

int check_detect(const lmx_yolo* m, const char* fn, const void* frames, int n, int h, int w, int precision, int max_det, const void* boxes,
                 const void* scores, const void* cls, const void* src, const void* counts, const void* kpts) {
  LMX_TRY(check_frames(m, fn, frames, n, h, w, precision));
  LMX_REQUIRE(max_det > 0 && max_det <= (1 << 20), "%s: max_det = %d", fn, max_det);
  LMX_REQUIRE(boxes && scores && cls && src && counts, "%s: null pointer (boxes, scores, cls, src and counts are all required)", fn);
  LMX_REQUIRE((kpts != nullptr) == (m->img.cfg.kpt_k != 0), "%s: kpts must be %s", fn,
              m->img.cfg.kpt_k ? "given: the image has a Pose head" : "NULL: the image has no Pose head");
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_yolo_open_host(const char* path_host, int max_batch, lmx_yolo** out_host) {
  return lmx_handle_open("lmx_yolo_open_host", path_host, max_batch, out_host, open_into, destroy);
}

extern "C" void lmx_yolo_close(lmx_yolo* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_yolo_info(const lmx_yolo* m, lmx_yolo_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_yolo_info: null argument");
  lmx_yolo_fill_info(m->img.cfg, m->max_batch, info_host);
  return LMX_OK;
}

extern "C" const char* lmx_yolo_class_name(const lmx_yolo* m, int cls) {
  if (!m || cls < 0 || cls >= (int)m->img.names.size()) return nullptr;
  return m->img.names[(size_t)cls].c_str();
}

extern "C" int lmx_yolo_prepare(lmx_yolo* m, int h, int w, int precision) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_yolo_prepare"));
  return prepare(m, h, w, precision, nullptr);
}

extern "C" int lmx_yolo_anchors(const lmx_yolo* m, int h, int w, int* oh_host, int* ow_host, int* A_host) {
  LMX_REQUIRE(m && oh_host && ow_host && A_host, "lmx_yolo_anchors: null argument");
  lmx_letterbox_geo_t geo;
  LMX_TRY(geometry(m, h, w, &geo, A_host));
  *oh_host = geo.oh;
  *ow_host = geo.ow;
  return LMX_OK;
}

extern "C" int lmx_yolo_predict(lmx_yolo* m, const uint8_t* frames, int n, int h, int w, int precision, float* pred, lmx_stream_t stream) {
  LMX_TRY(check_frames(m, "lmx_yolo_predict", frames, n, h, w, precision));
  LMX_REQUIRE(pred != nullptr, "lmx_yolo_predict: null pointer (pred)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_yolo_predict", st));  // before prepare: a refused call allocates nothing
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));  // a pair seen before: a lookup
  const size_t frame_bytes = (size_t)h * w * 3, pred_row = (size_t)P->A * (4 + m->img.cfg.nc);
  Act kraw[3];
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    LMX_TRY(predict_chunk(m, *P, "lmx_yolo_predict", precision, frames + (size_t)done * frame_bytes, nb, h, w, pred + (size_t)done * pred_row, kraw, st));
  }
  return LMX_OK;
}

extern "C" int lmx_yolo_detect(lmx_yolo* m, const uint8_t* frames, int n, int h, int w, int precision, float conf, double iou, int max_det,
                               float* boxes, float* scores, int32_t* cls, int32_t* src, int32_t* counts, float* kpts, lmx_stream_t stream) {
  LMX_TRY(check_detect(m, "lmx_yolo_detect", frames, n, h, w, precision, max_det, boxes, scores, cls, src, counts, kpts));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_yolo_detect", st));  // before prepare: a refused call allocates nothing
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));
  const size_t frame_bytes = (size_t)h * w * 3, md = (size_t)max_det, kp = md * m->img.cfg.kpt_k * m->img.cfg.kpt_ndim;
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    const size_t d = (size_t)done;
    LMX_TRY(detect_chunk(m, *P, "lmx_yolo_detect", precision, frames + d * frame_bytes, nb, h, w, conf, iou, max_det, boxes + d * md * 4, scores + d * md, cls + d * md,
                         src + d * md, counts + d, kpts ? kpts + d * kp : nullptr, st));
  }
  return LMX_OK;
}

extern "C" int lmx_yolo_detect_host(lmx_yolo* m, const uint8_t* frames_host, int n, int h, int w, int precision, float conf, double iou, int max_det,
                                    float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* src_host, int32_t* counts_host,
                                    float* kpts_host) {
  LMX_TRY(check_detect(m, "lmx_yolo_detect_host", frames_host, n, h, w, precision, max_det, boxes_host, scores_host, cls_host, src_host, counts_host,
                       kpts_host));
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));
  // staging of one chunk: frames | boxes | scores | cls | src | counts | kpts, each on a 256-byte boundary
  const size_t B = (size_t)(n < m->max_batch ? n : m->max_batch), frame_bytes = (size_t)h * w * 3, md = (size_t)max_det;
  const size_t kp = md * m->img.cfg.kpt_k * m->img.cfg.kpt_ndim;
  LmxLayout lay;
  lay.add(B * frame_bytes);  // the frames, at the blob's start
  const size_t o_boxes = lay.add(B * md * 16), o_scores = lay.add(B * md * 4), o_cls = lay.add(B * md * 4), o_src = lay.add(B * md * 4),
               o_counts = lay.add(B * 4), o_kpts = lay.add(B * kp * 4);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  char* s = m->stage;
  float *boxes = reinterpret_cast<float*>(s + o_boxes), *scores = reinterpret_cast<float*>(s + o_scores);
  int32_t *cls = reinterpret_cast<int32_t*>(s + o_cls), *src = reinterpret_cast<int32_t*>(s + o_src), *counts = reinterpret_cast<int32_t*>(s + o_counts);
  float* kpts = kpts_host ? reinterpret_cast<float*>(s + o_kpts) : nullptr;
  for (int done = 0; done < n; done += m->max_batch) {
    const size_t nb = (size_t)(n - done < m->max_batch ? n - done : m->max_batch), d = (size_t)done;
    LMX_HIP(hipMemcpyAsync(s, frames_host + d * frame_bytes, nb * frame_bytes, hipMemcpyHostToDevice, m->own));
    LMX_TRY(detect_chunk(m, *P, "lmx_yolo_detect_host", precision, reinterpret_cast<const uint8_t*>(s), (int)nb, h, w, conf, iou, max_det, boxes, scores, cls, src, counts, kpts,
                         m->own));
    LMX_HIP(hipMemcpyAsync(boxes_host + d * md * 4, boxes, nb * md * 16, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(scores_host + d * md, scores, nb * md * 4, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(cls_host + d * md, cls, nb * md * 4, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(src_host + d * md, src, nb * md * 4, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(counts_host + d, counts, nb * 4, hipMemcpyDeviceToHost, m->own));
    if (kpts) LMX_HIP(hipMemcpyAsync(kpts_host + d * kp, kpts, nb * kp * 4, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipStreamSynchronize(m->own));
  }
  return LMX_OK;
}
