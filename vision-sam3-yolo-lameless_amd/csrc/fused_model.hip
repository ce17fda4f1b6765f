// fused_model.hip — the model-level entry points of the C-ABI for the fused per-frame path (BASELINE cfg#5): ONE handle over a YOLO, a
// SAM and a DINO weight image, raw frames in, one fixed-stride record per frame out.  lmx_fused_step is the launch sequence of
// lmx/pipeline.py's FusedExtractor._step_dense / step written as host C++ over the three model handles (yolo_model.hip, sam_model.hip
// with its workspace lanes — sam_lanes.h —, dino_model.hip) and lmx_k_pack_records: YOLO on an internal stream, DINO on another, the
// SAM passes of sam_chunk frames dealt over the rest as lmx_h_stream_plan says, each pass's decoder behind YOLO's event, the caller's
// stream behind all of them, then the record kernel.  HOST code only: there is no kernel in this file and no arithmetic of its own, so
// the records are the bytes lmx.dist.pack_records makes of FusedExtractor.step's dict (tests/test_gpu_native_fused.py).
// lmx_fused_step_yuv / _yuv_host take the frames as a decoder leaves them (NV12 / I420): lmx_k_yuv420_to_bgr (yuv.hip) into a BGR buffer of
// the handle's, on the caller's stream, then the same sequence on that buffer (tests/test_gpu_native_fused_yuv.py).
// OUT OF SCOPE: the byte masks (keep_byte_masks), pose keypoints in the record, point or mask prompts, RCCL, HIP graph capture.
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "model_handle.h"
#include "sam_lanes.h"
#include "yuv.h"

namespace {

const int MAX_DET = 300;           // YoloDetector.detect's max_det, the rows of boxes / scores / cls in a record
const double NMS_IOU = 0.7;        // ... and its iou
const int FUSED_MAX_STREAMS = 64;  // internal streams a handle may be asked for

// the step's outputs for one frame size, max_frames rows each: what FusedExtractor.step returns as a dict, in one allocation
struct Work {
  char* blob = nullptr;
  float *boxes, *scores, *emb, *iou;
  int32_t *cls, *src, *counts;
  uint8_t* mask_bits;
  int64_t *stats, *contour;
  char* gather = nullptr;  // the reference schedule's frames: [det frames | emb frames], there once a schedule is set
};

}  // namespace

struct lmx_fused : LmxHandleCore {
  int sam_chunk = 0, sam_lanes = 0, max_streams = 0;
  lmx_yolo* yolo = nullptr;
  lmx_sam* sam = nullptr;
  lmx_dino* dino = nullptr;
  lmx_yolo_info_t yi;
  lmx_sam_info_t si;
  lmx_dino_info_t di;
  std::vector<hipStream_t> pool;  // [0] YOLO, [1] DINO, [2 ..] one per SAM lane
  std::vector<hipEvent_t> done;   // one per pool stream: its part of the step is enqueued
  hipEvent_t start = nullptr, det = nullptr;
  std::map<std::pair<int, int>, Work> work;
  // the reference schedule (lmx_fused_schedule): the frames each network runs on, and on the device [map_det | map_emb | ran_det | ran_emb]
  bool scheduled = false, det_all = false, emb_all = false;  // *_all: that list was left out, the network runs on the caller's frames in place
  int sched_n = 0;
  std::vector<int32_t> det_idx, emb_idx;
  int32_t* maps = nullptr;
  // lmx_fused_step_yuv's converted frames: max_batch BGR frames of yuv_h x yuv_w, there from the first _yuv call for that size on
  uint8_t* yuv_bgr = nullptr;
  int yuv_h = 0, yuv_w = 0;
};

namespace {

void destroy(lmx_fused* m) {
  for (auto& kv : m->work) {
    (void)hipFree(kv.second.blob);
    (void)hipFree(kv.second.gather);
  }
  (void)hipFree(m->maps);
  (void)hipFree(m->yuv_bgr);
  for (hipEvent_t e : m->done) (void)hipEventDestroy(e);
  if (m->start) (void)hipEventDestroy(m->start);
  if (m->det) (void)hipEventDestroy(m->det);
  for (hipStream_t s : m->pool) (void)hipStreamDestroy(s);
  lmx_sam_close(m->sam);
  lmx_dino_close(m->dino);
  lmx_yolo_close(m->yolo);
  lmx_handle_free(m);
  delete m;
}

int open_into(lmx_fused* m, const char* yolo_image, const char* sam_image, const char* dino_image) {
  LMX_HIP(hipGetDevice(&m->device));
  LMX_TRY(lmx_yolo_open_host(yolo_image, m->max_batch, &m->yolo));
  LMX_TRY(lmx_yolo_info(m->yolo, &m->yi));
  LMX_REQUIRE(m->yi.kpt_k == 0, "lmx_fused_open_host: yolo_image has a Pose head (%d keypoints); keypoints are no part of the record", m->yi.kpt_k);
  LMX_TRY(lmx_sam_open_host(sam_image, m->sam_chunk, &m->sam));
  LMX_TRY(lmx_sam_info(m->sam, &m->si));
  LMX_TRY(lmx_dino_open_host(dino_image, m->max_batch, &m->dino));
  LMX_TRY(lmx_dino_info(m->dino, &m->di));
  // the widest plan any step takes: YOLO, DINO and one stream per lane (lmx_h_stream_plan of every chunk count stays inside it)
  const int n_pool = 2 + m->sam_lanes;
  for (int i = 0; i < n_pool; ++i) {
    hipStream_t s = nullptr;
    LMX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    m->pool.push_back(s);
    hipEvent_t e = nullptr;
    LMX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    m->done.push_back(e);
  }
  LMX_HIP(hipEventCreateWithFlags(&m->start, hipEventDisableTiming));
  LMX_HIP(hipEventCreateWithFlags(&m->det, hipEventDisableTiming));
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->maps), (size_t)m->max_batch * 4 * sizeof(int32_t)));
  return LMX_OK;
}

int check_precision(const lmx_fused* m, const char* fn, int precision) {
  LMX_REQUIRE(precision == LMX_SAM_F16 || precision == LMX_SAM_EXACT, "%s: precision %d is neither LMX_SAM_F16 (0) nor LMX_SAM_EXACT (1)", fn, precision);
  const char* plan = precision == LMX_SAM_F16 ? "f16" : "exact";
  LMX_REQUIRE(m->yi.plans & (1 << precision), "%s: yolo_image does not hold the %s plan (plans mask %d)", fn, plan, m->yi.plans);
  LMX_REQUIRE(m->si.plans & (1 << precision), "%s: sam_image does not hold the %s plan (plans mask %d)", fn, plan, m->si.plans);
  return LMX_OK;
}

int check_size(const char* fn, int h, int w) {
  LMX_REQUIRE(h > 0 && w > 0, "%s: frame size %d x %d", fn, h, w);
  LMX_REQUIRE(h > 1 && w > 1 && (int64_t)h * w <= 0x1fffff, "%s: the record's contour features are served for frames of 2 x 2 up to 2^21 - 1 pixels, not %d x %d", fn,
              h, w);
  return LMX_OK;
}

// the streams the handle's passes take: lmx_h_stream_plan under the handle's bounds (max_streams, and a stream per lane)
int plan_streams(const lmx_fused* m, int n_chunks, int* pool, std::vector<int32_t>* sam) {
  const int cap = m->max_streams < 2 + m->sam_lanes ? m->max_streams : 2 + m->sam_lanes;
  int det = 0, emb = 0;
  sam->assign((size_t)(n_chunks > 0 ? n_chunks : 1), 0);
  return lmx_h_stream_plan(n_chunks, cap, LMX_STREAMS_LANES, pool, &det, &emb, sam->data());
}

int ensure_gather(lmx_fused* m, int h, int w, Work* W) {
  if (W->gather) return LMX_OK;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&W->gather), (size_t)2 * m->max_batch * h * w * 3));
  return LMX_OK;
}

int prepare(lmx_fused* m, int h, int w, int precision, Work** out) {
  const char* fn = "lmx_fused_prepare";
  LMX_TRY(check_size(fn, h, w));
  LMX_TRY(check_precision(m, fn, precision));
  const auto key = std::make_pair(h, w);
  if (!m->work.count(key))
    LMX_REQUIRE((int)m->work.size() < LMX_MAX_PREPARED, "%s: the handle already holds %d frame sizes; open another for more", fn, LMX_MAX_PREPARED);
  LMX_TRY(lmx_yolo_prepare(m->yolo, h, w, precision));
  LMX_TRY(lmx_dino_prepare(m->dino, h, w));
  LMX_TRY(lmx_sam_lanes_prepare(m->sam, h, w, precision, m->sam_lanes));
  auto it = m->work.find(key);
  if (it == m->work.end()) {
    const size_t B = (size_t)m->max_batch, wb = ((size_t)w + 7) / 8;
    LmxLayout lay;
    const size_t o_boxes = lay.add(B * MAX_DET * 16), o_scores = lay.add(B * MAX_DET * 4), o_cls = lay.add(B * MAX_DET * 4), o_src = lay.add(B * MAX_DET * 4),
                 o_counts = lay.add(B * 4), o_emb = lay.add(B * m->di.hidden * 4), o_bits = lay.add(B * h * wb), o_stats = lay.add(B * 64),
                 o_contour = lay.add(B * 64), o_iou = lay.add(B * 4);
    Work W;
    LMX_HIP(hipMalloc(reinterpret_cast<void**>(&W.blob), lay.total));
    char* b = W.blob;
    W.boxes = reinterpret_cast<float*>(b + o_boxes);
    W.scores = reinterpret_cast<float*>(b + o_scores);
    W.cls = reinterpret_cast<int32_t*>(b + o_cls);
    W.src = reinterpret_cast<int32_t*>(b + o_src);
    W.counts = reinterpret_cast<int32_t*>(b + o_counts);
    W.emb = reinterpret_cast<float*>(b + o_emb);
    W.mask_bits = reinterpret_cast<uint8_t*>(b + o_bits);
    W.stats = reinterpret_cast<int64_t*>(b + o_stats);
    W.contour = reinterpret_cast<int64_t*>(b + o_contour);
    W.iou = reinterpret_cast<float*>(b + o_iou);
    it = m->work.emplace(key, W).first;
  }
  if (m->scheduled) LMX_TRY(ensure_gather(m, h, w, &it->second));
  LMX_HIP(hipDeviceSynchronize());
  if (out) *out = &it->second;
  return LMX_OK;
}

// the BGR frames of the _yuv entry points: one buffer per handle, of the size the last _yuv call brought.  Only these calls come here:
// a handle that steps on BGR never holds it
int ensure_yuv(lmx_fused* m, int h, int w) {
  if (m->yuv_bgr && m->yuv_h == h && m->yuv_w == w) return LMX_OK;
  LMX_HIP(hipDeviceSynchronize());  // a step on the old size has finished (the handle rule); its buffer is idle
  (void)hipFree(m->yuv_bgr);
  m->yuv_bgr = nullptr;
  m->yuv_h = m->yuv_w = 0;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->yuv_bgr), (size_t)m->max_batch * h * w * 3));
  m->yuv_h = h;
  m->yuv_w = w;
  return LMX_OK;
}

bool prepared(const lmx_fused* m, int h, int w, int precision) {
  const auto it = m->work.find(std::make_pair(h, w));
  return it != m->work.end() && (!m->scheduled || it->second.gather) && lmx_sam_lanes_ready(m->sam, h, w, precision, m->sam_lanes);
}

int check_step(const lmx_fused* m, const char* fn, const void* frames, int n, int h, int w, int precision, const void* records, int64_t n_rows) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n >= 0 && n <= m->max_batch, "%s: n = %d frames outside 0 .. max_frames = %d", fn, n, m->max_batch);
  LMX_REQUIRE(n_rows >= n, "%s: n_rows = %lld is below n = %d: every frame needs a row", fn, (long long)n_rows, n);
  LMX_TRY(check_size(fn, h, w));
  LMX_TRY(check_precision(m, fn, precision));
  LMX_REQUIRE(n == 0 || frames != nullptr, "%s: null pointer (frames)", fn);
  LMX_REQUIRE(n_rows == 0 || records != nullptr, "%s: null pointer (records)", fn);
  LMX_REQUIRE(!m->scheduled || n == m->sched_n, "%s: n = %d frames, the schedule was set for %d (lmx_fused_schedule)", fn, n, m->sched_n);
  return LMX_OK;
}

// the dense sequence on nd frames for YOLO + SAM and ne frames for DINO, then the records; everything is checked and prepared
int enqueue(lmx_fused* m, Work& W, const uint8_t* frames, int n, int h, int w, int precision, float conf, uint8_t* records, int64_t n_rows,
            hipStream_t st) {
  const size_t frame_bytes = (size_t)h * w * 3, wb = ((size_t)w + 7) / 8;
  const uint8_t *fd = frames, *fe = frames;
  int nd = n, ne = n;
  if (m->scheduled) {  // frames.index_select(0, idx): device-to-device copies on the caller's stream
    uint8_t* g = reinterpret_cast<uint8_t*>(W.gather);
    uint8_t* ge = g + (size_t)m->max_batch * frame_bytes;
    nd = (int)m->det_idx.size();
    ne = (int)m->emb_idx.size();
    if (!m->det_all) {
      for (int j = 0; j < nd; ++j)
        LMX_HIP(hipMemcpyAsync(g + (size_t)j * frame_bytes, frames + (size_t)m->det_idx[(size_t)j] * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, st));
      fd = g;
    }
    if (!m->emb_all) {
      for (int j = 0; j < ne; ++j)
        LMX_HIP(hipMemcpyAsync(ge + (size_t)j * frame_bytes, frames + (size_t)m->emb_idx[(size_t)j] * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, st));
      fe = ge;
    }
  }
  const int n_chunks = (nd + m->sam_chunk - 1) / m->sam_chunk;
  int n_pool = 0;
  std::vector<int32_t> sam_stream;
  LMX_TRY(plan_streams(m, n_chunks, &n_pool, &sam_stream));
  LMX_REQUIRE(n_pool <= (int)m->pool.size(), "lmx_fused_step: the plan asks for %d streams, the handle has %d", n_pool, (int)m->pool.size());
  if (nd > 0 || ne > 0) {
    // the frames were produced on the caller's stream
    LMX_HIP(hipEventRecord(m->start, st));
    for (int i = 0; i < n_pool; ++i) LMX_HIP(hipStreamWaitEvent(m->pool[(size_t)i], m->start, 0));
    if (nd > 0) {
      LMX_TRY(lmx_yolo_detect(m->yolo, fd, nd, h, w, precision, conf, NMS_IOU, MAX_DET, W.boxes, W.scores, W.cls, W.src, W.counts, nullptr, m->pool[0]));
      LMX_HIP(hipEventRecord(m->det, m->pool[0]));
    }
    if (ne > 0) LMX_TRY(lmx_dino_embed(m->dino, fe, ne, h, w, 0, W.emb, m->pool[1]));
    for (int j = 0; j < n_chunks; ++j) {
      const int at = j * m->sam_chunk, nb = nd - at < m->sam_chunk ? nd - at : m->sam_chunk;
      const int s = sam_stream[(size_t)j], lane = s - 2;  // a lane per stream: a later pass on the lane is ordered behind the earlier one
      hipStream_t ps = m->pool[(size_t)s];
      LMX_TRY(lmx_sam_lane_encode(m->sam, lane, fd + (size_t)at * frame_bytes, nb, h, w, precision, ps));
      LMX_HIP(hipStreamWaitEvent(ps, m->det, 0));  // the decoder needs the boxes; the encoder ran without them
      // the prompt is the frame's first (highest-confidence) detection: row 0 of its max_det boxes
      LMX_TRY(lmx_sam_lane_decode(m->sam, lane, nb, h, w, W.boxes + (size_t)at * MAX_DET * 4, (int64_t)MAX_DET * 4, precision,
                                  W.mask_bits + (size_t)at * h * wb, W.stats + (size_t)at * 8, W.contour + (size_t)at * 8, W.iou + at, ps));
    }
    for (int i = 0; i < n_pool; ++i) {
      LMX_HIP(hipEventRecord(m->done[(size_t)i], m->pool[(size_t)i]));
      LMX_HIP(hipStreamWaitEvent(st, m->done[(size_t)i], 0));
    }
  }
  // the records: lmx.dist.pack_records of the step's dict, the reference schedule's index_copy_ as the row maps
  lmx_record_layout_t lay;
  LMX_TRY(lmx_h_record_layout(h, w, m->di.hidden, MAX_DET, m->scheduled ? 1 : 0, &lay));
  lmx_record_field_t f[LMX_RECORD_MAX_FIELDS];
  const int B = m->max_batch;
  for (int i = 0; i < lay.n_fields; ++i) {
    const char* name = lay.fields[i].name;
    const void* src = nullptr;
    int map = m->scheduled ? 0 : -1, rows = nd;
    if (!strcmp(name, "boxes")) src = W.boxes;
    else if (!strcmp(name, "cls")) src = W.cls;
    else if (!strcmp(name, "counts")) src = W.counts;
    else if (!strcmp(name, "mask_bits")) src = W.mask_bits;
    else if (!strcmp(name, "mask_contour")) src = W.contour;
    else if (!strcmp(name, "mask_iou")) src = W.iou;
    else if (!strcmp(name, "mask_stats")) src = W.stats;
    else if (!strcmp(name, "scores")) src = W.scores;
    else if (!strcmp(name, "embedding")) src = W.emb, map = m->scheduled ? 1 : -1, rows = ne;
    else if (!strcmp(name, "ran_det")) src = m->maps + 2 * B, map = -1, rows = n;
    else if (!strcmp(name, "ran_emb")) src = m->maps + 3 * B, map = -1, rows = n;
    LMX_REQUIRE(src != nullptr, "lmx_fused_step: the layout names a field '%s' the step does not produce", name);
    f[i] = lmx_record_field_t{src, lay.fields[i].nbytes, lay.fields[i].offset, map, rows};
  }
  const int32_t* maps[2] = {m->maps, m->maps + B};
  return lmx_k_pack_records(f, lay.n_fields, maps, m->scheduled ? 2 : 0, n, n_rows, lay.stride, records, st);
}

}  // namespace

extern "C" int lmx_fused_open_host(const char* yolo_image, const char* sam_image, const char* dino_image, int max_frames, int sam_chunk, int sam_lanes,
                                   int max_streams, lmx_fused** out_host) {
  const char* fn = "lmx_fused_open_host";
  LMX_REQUIRE(out_host != nullptr, "%s: out_host is null", fn);
  *out_host = nullptr;
  LMX_REQUIRE(yolo_image && sam_image && dino_image, "%s: null path (%s)", fn, !yolo_image ? "yolo_image" : !sam_image ? "sam_image" : "dino_image");
  LMX_REQUIRE(max_frames > 0 && max_frames <= 65535, "%s: max_frames %d outside 1 .. 65535", fn, max_frames);
  LMX_REQUIRE(sam_chunk > 0 && sam_chunk <= 65535, "%s: sam_chunk %d outside 1 .. 65535", fn, sam_chunk);
  LMX_REQUIRE(sam_lanes > 0 && sam_lanes <= LMX_SAM_MAX_LANES, "%s: sam_lanes %d outside 1 .. %d", fn, sam_lanes, LMX_SAM_MAX_LANES);
  LMX_REQUIRE(max_streams > 0 && max_streams <= FUSED_MAX_STREAMS, "%s: max_streams %d outside 1 .. %d", fn, max_streams, FUSED_MAX_STREAMS);
  lmx_fused* m = new lmx_fused();
  m->max_batch = max_frames;
  m->sam_chunk = sam_chunk;
  m->sam_lanes = sam_lanes;
  m->max_streams = max_streams;
  int rc = open_into(m, yolo_image, sam_image, dino_image);
  if (rc == LMX_OK) rc = lmx_handle_finish_open(m);
  if (rc != LMX_OK) {
    destroy(m);
    return rc;
  }
  *out_host = m;
  return LMX_OK;
}

extern "C" void lmx_fused_close(lmx_fused* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_fused_info(const lmx_fused* m, lmx_fused_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_fused_info: null argument");
  info_host->yolo = m->yi;
  info_host->sam = m->si;
  info_host->dino = m->di;
  info_host->hidden = m->di.hidden;
  info_host->max_det = MAX_DET;
  info_host->max_frames = m->max_batch;
  info_host->sam_chunk = m->sam_chunk;
  info_host->sam_lanes = m->sam_lanes;
  info_host->max_streams = m->max_streams;
  return LMX_OK;
}

extern "C" int lmx_fused_layout(const lmx_fused* m, int h, int w, int scheduled, lmx_record_layout_t* out_host) {
  LMX_REQUIRE(m && out_host, "lmx_fused_layout: null argument");
  return lmx_h_record_layout(h, w, m->di.hidden, MAX_DET, scheduled, out_host);
}

extern "C" int lmx_fused_prepare(lmx_fused* m, int h, int w, int precision) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_fused_prepare"));
  return prepare(m, h, w, precision, nullptr);
}

extern "C" int lmx_fused_schedule(lmx_fused* m, int n, const int32_t* det_idx_host, int n_det, const int32_t* emb_idx_host, int n_emb) {
  const char* fn = "lmx_fused_schedule";
  LMX_TRY(lmx_handle_on_device(m, fn));
  if (n_det < 0 && n_emb < 0) {  // dense again (the gather buffers stay)
    m->scheduled = false;
    m->det_idx.clear();
    m->emb_idx.clear();
    return LMX_OK;
  }
  LMX_REQUIRE(n >= 0 && n <= m->max_batch, "%s: n = %d frames outside 0 .. max_frames = %d", fn, n, m->max_batch);
  // a list left out (-1) names every frame, as det_idx = None / emb_idx = None of FusedExtractor.step
  std::vector<int32_t> all((size_t)n), di, ei;
  for (int i = 0; i < n; ++i) all[(size_t)i] = i;
  LMX_REQUIRE(n_det <= 0 || det_idx_host, "%s: null pointer (det_idx_host)", fn);
  LMX_REQUIRE(n_emb <= 0 || emb_idx_host, "%s: null pointer (emb_idx_host)", fn);
  LMX_REQUIRE(n_det <= n && n_emb <= n, "%s: det_idx names %d and emb_idx %d frames of %d", fn, n_det, n_emb, n);
  if (n_det < 0)
    di = all;
  else if (n_det > 0)
    di.assign(det_idx_host, det_idx_host + n_det);
  if (n_emb < 0)
    ei = all;
  else if (n_emb > 0)
    ei.assign(emb_idx_host, emb_idx_host + n_emb);
  const size_t B = (size_t)m->max_batch;
  std::vector<int32_t> host(4 * B, 0);
  LMX_TRY(lmx_h_row_map(n, di.data(), (int)di.size(), "det_idx", host.data(), host.data() + 2 * B));
  LMX_TRY(lmx_h_row_map(n, ei.data(), (int)ei.size(), "emb_idx", host.data() + B, host.data() + 3 * B));
  for (auto& kv : m->work) LMX_TRY(ensure_gather(m, kv.first.first, kv.first.second, &kv.second));
  LMX_HIP(hipMemcpy(m->maps, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  LMX_HIP(hipDeviceSynchronize());
  m->scheduled = true;
  m->sched_n = n;
  m->det_all = n_det < 0;
  m->emb_all = n_emb < 0;
  m->det_idx = di;
  m->emb_idx = ei;
  return LMX_OK;
}

extern "C" int lmx_fused_step(lmx_fused* m, const uint8_t* frames, int n, int h, int w, int precision, float conf, uint8_t* records, int64_t n_rows,
                              lmx_stream_t stream) {
  const char* fn = "lmx_fused_step";
  LMX_TRY(check_step(m, fn, frames, n, h, w, precision, records, n_rows));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, fn, st));  // before prepare: a refused call allocates nothing
  if (!prepared(m, h, w, precision)) LMX_TRY(prepare(m, h, w, precision, nullptr));  // a size seen before: a lookup
  return enqueue(m, m->work[std::make_pair(h, w)], frames, n, h, w, precision, conf, records, n_rows, st);
}

extern "C" int lmx_fused_step_host(lmx_fused* m, const uint8_t* frames_host, int n, int h, int w, int precision, float conf, uint8_t* records_host,
                                   int64_t n_rows) {
  const char* fn = "lmx_fused_step_host";
  LMX_TRY(check_step(m, fn, frames_host, n, h, w, precision, records_host, n_rows));
  if (!prepared(m, h, w, precision)) LMX_TRY(prepare(m, h, w, precision, nullptr));
  lmx_record_layout_t lay;
  LMX_TRY(lmx_h_record_layout(h, w, m->di.hidden, MAX_DET, m->scheduled ? 1 : 0, &lay));
  // staging: frames | records, each on a 256-byte boundary
  const size_t frame_bytes = (size_t)h * w * 3, rec_bytes = (size_t)n_rows * (size_t)lay.stride;
  LmxLayout z;
  z.add((size_t)n * frame_bytes);  // the frames, at the blob's start
  const size_t o_rec = z.add(rec_bytes);
  if (z.total == 0) return LMX_OK;
  LMX_TRY(lmx_handle_grow_stage(m, z.total));
  uint8_t* s = reinterpret_cast<uint8_t*>(m->stage);
  if (n > 0) LMX_HIP(hipMemcpyAsync(s, frames_host, (size_t)n * frame_bytes, hipMemcpyHostToDevice, m->own));
  LMX_TRY(enqueue(m, m->work[std::make_pair(h, w)], s, n, h, w, precision, conf, s + o_rec, n_rows, m->own));
  if (rec_bytes) LMX_HIP(hipMemcpyAsync(records_host, s + o_rec, rec_bytes, hipMemcpyDeviceToHost, m->own));  // the records in ONE copy
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}

extern "C" int lmx_fused_step_yuv(lmx_fused* m, const lmx_yuv_frames_t* frames_host, int n, int h, int w, int precision, float conf, uint8_t* records,
                                  int64_t n_rows, lmx_stream_t stream) {
  const char* fn = "lmx_fused_step_yuv";
  LMX_TRY(check_step(m, fn, frames_host, n, h, w, precision, records, n_rows));
  LMX_TRY(lmx_yuv_check(fn, frames_host, n, h, w));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, fn, st));  // before anything is allocated
  if (!prepared(m, h, w, precision)) LMX_TRY(prepare(m, h, w, precision, nullptr));
  LMX_TRY(ensure_yuv(m, h, w));
  LMX_TRY(lmx_k_yuv420_to_bgr(frames_host, n, h, w, m->yuv_bgr, st));  // on the caller's stream: the step's start event is recorded behind it
  return enqueue(m, m->work[std::make_pair(h, w)], m->yuv_bgr, n, h, w, precision, conf, records, n_rows, st);
}

extern "C" int lmx_fused_step_yuv_roi(lmx_fused* m, const lmx_yuv_frames_t* frames_host, int n, int h, int w, const lmx_rect_t* roi_host, int precision,
                                      float conf, uint8_t* records, int64_t n_rows, lmx_stream_t stream) {
  const char* fn = "lmx_fused_step_yuv_roi";
  LMX_TRY(lmx_yuv_check(fn, frames_host, n, h, w));  // the frame's size is checked here; what the step runs at is the window's
  LMX_TRY(lmx_yuv_check_roi(fn, roi_host, h, w));
  const int rh = roi_host->h, rw = roi_host->w;
  LMX_TRY(check_step(m, fn, frames_host, n, rh, rw, precision, records, n_rows));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, fn, st));  // before anything is allocated
  if (!prepared(m, rh, rw, precision)) LMX_TRY(prepare(m, rh, rw, precision, nullptr));
  LMX_TRY(ensure_yuv(m, rh, rw));
  LMX_TRY(lmx_k_yuv420_to_bgr_roi(frames_host, n, h, w, roi_host, m->yuv_bgr, st));  // on the caller's stream, as lmx_fused_step_yuv
  return enqueue(m, m->work[std::make_pair(rh, rw)], m->yuv_bgr, n, rh, rw, precision, conf, records, n_rows, st);
}

extern "C" int lmx_fused_step_yuv_host(lmx_fused* m, const uint8_t* yuv_host, int layout, int matrix, int n, int h, int w, int precision, float conf,
                                       uint8_t* records_host, int64_t n_rows) {
  const char* fn = "lmx_fused_step_yuv_host";
  LMX_TRY(check_step(m, fn, yuv_host, n, h, w, precision, records_host, n_rows));
  LMX_TRY(lmx_yuv_check_format(fn, layout, matrix, n, h, w));
  if (!prepared(m, h, w, precision)) LMX_TRY(prepare(m, h, w, precision, nullptr));
  LMX_TRY(ensure_yuv(m, h, w));
  lmx_record_layout_t lay;
  LMX_TRY(lmx_h_record_layout(h, w, m->di.hidden, MAX_DET, m->scheduled ? 1 : 0, &lay));
  // staging: the rawvideo blob | records, each on a 256-byte boundary
  const size_t luma = (size_t)h * w, frame_bytes = luma + luma / 2, rec_bytes = (size_t)n_rows * (size_t)lay.stride;
  LmxLayout z;
  z.add((size_t)n * frame_bytes);  // the frames, at the blob's start
  const size_t o_rec = z.add(rec_bytes);
  if (z.total == 0) return LMX_OK;
  LMX_TRY(lmx_handle_grow_stage(m, z.total));
  uint8_t* s = reinterpret_cast<uint8_t*>(m->stage);
  if (n > 0) LMX_HIP(hipMemcpyAsync(s, yuv_host, (size_t)n * frame_bytes, hipMemcpyHostToDevice, m->own));  // 1.5 bytes per pixel in ONE copy
  // a rawvideo frame: h luma rows of w bytes, then (nv12) h / 2 rows of w interleaved bytes or (yuv420p) the U and the V plane of h / 2 x w / 2
  lmx_yuv_frames_t f;
  memset(&f, 0, sizeof(f));
  f.y = s;
  f.u = s + luma;
  f.v = layout == LMX_YUV_I420 ? s + luma + luma / 4 : nullptr;
  f.pitch_y = w;
  f.pitch_c = layout == LMX_YUV_I420 ? w / 2 : w;
  f.stride_y = f.stride_c = (int64_t)frame_bytes;
  f.layout = layout;
  f.matrix = matrix;
  LMX_TRY(lmx_k_yuv420_to_bgr(&f, n, h, w, m->yuv_bgr, m->own));
  LMX_TRY(enqueue(m, m->work[std::make_pair(h, w)], m->yuv_bgr, n, h, w, precision, conf, s + o_rec, n_rows, m->own));
  if (rec_bytes) LMX_HIP(hipMemcpyAsync(records_host, s + o_rec, rec_bytes, hipMemcpyDeviceToHost, m->own));  // the records in ONE copy
  LMX_HIP(hipStreamSynchronize(m->own));
  return LMX_OK;
}
