// sam_model.hip — the model-level entry points of the C-ABI for SAM v1: a handle (model_handle.h has what every handle owns) with the
// weights of one weight image (sam_image.h) and, per prepared (frame size, plan), the workspace of one batch.  lmx_sam_encode is the
// launch sequence of lmx/sam.py's SamVitEncoder.encode, lmx_sam_decode that of lmx/sam_decoder.py's MaskDecoder.predict followed by the
// lmx_k_pack_bits / lmx_k_contour_features of lmx/pipeline.py (services/sam3-pipeline/app/main.py:74-92), written as host C++.
// HOST code only: there is no kernel in this file and no arithmetic of its own beyond the resize tables (lmx_h_pil_tables).  Every
// launch goes through the same extern "C" lmx_k_* entry point the ctypes binding calls, with the descriptor filled as lmx/kernels.py
// fills it, in the Python plan's order, so the outputs are the Python plan's bit for bit on both precision plans
// (tests/test_gpu_native_sam.py).  What is torch glue in Python — torch.cat of the output tokens with the sparse prompt, the q / k / v
// slices of qkv, q3[:, k].contiguous(), iou[:, 0] — is a leading dimension or a strided copy on the call's stream here.
// An image whose encoder is Hiera runs sam_hiera_model.h's launch plan in place of the ViT's (encode_chunk branches after the resize);
// its embedding is f16 under both plans, which the decoder's first lmx_k_add_bcast takes as such.
// Memory: encode_chunk and decode_chunk are written once over a SamRun, a run of plan_run.h.  Each activation buffer is taken where the
// plan first writes it, with the size that launch uses; build() walks encode + decode counting at max_batch and every call walks them
// launching.  What the launch right behind its writer consumes (Dec::lin's x3 operand, the relative-position tables, an attention's
// projections) is ONE region each, as large as its largest request.  What outlives a call stays a named field of Prepared.
// The fused handle (fused_model.hip) keeps several passes in flight on one handle: sam_lanes.h, at the end of this file, gives it further
// workspaces (lanes) over the same weights and the two halves of a pass; the public calls keep lane 0 and their one-stream rule.
// OUT OF SCOPE: point and mask-input prompts, multimask output, SamAutomaticMaskGenerator, outputs="all" of the Hiera encoder, HIP
// graph capture.
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "model_handle.h"
#include "sam_hiera_model.h"
#include "sam_image.h"
#include "sam_lanes.h"

namespace {

const int DD = LMX_SAM_DEC_D, DH = LMX_SAM_DEC_HEADS, DT = LMX_SAM_OUT_TOKENS + 2;  // the decoder's width, heads and tokens (5 + 2 box corners)

// a Linear's operands under one plan.  K: the columns of the ACTIVATION (f16 plan: w [N][K]; encoder exact: [N][2K]; decoder exact: [N][3K])
struct Lin {
  const void* w = nullptr;
  const float *b = nullptr, *s = nullptr;
  int N = 0, K = 0;
};

struct Norm {
  const float *g = nullptr, *b = nullptr;
};

struct EncLayer {
  bool glob = false;
  const float *g1, *b1, *rh, *rw, *g2, *b2;
  const half_t* padkv;
  Lin qkv[2], proj[2], fc1[2], fc2[2];  // per plan
};

// the decoder's Linears by role, per plan
struct DecAttn {
  Lin q, k, v, o;
};
struct DecLayer {
  DecAttn sa, t2i, i2t;
  Lin lin1, lin2;
  Norm ln[4];
};
struct DecPlan {
  DecLayer L[2];
  DecAttn fin;
  Lin up1, up2, hyp[3], iou[3];
};

// the regions of a run that are ONE buffer each, sized to the largest request (LmxPlanRun::share)
enum { S_REL, S_X3, S_PQ, S_PK, S_PV, S_PA, S_T1, S_T2, S_N };

// what lmx_sam_prepare builds for one (frame size, plan): the resize tables, what outlives a call, and the arenas of max_batch frames
// as the counting walk sized them (base and cap); one allocation
struct Prepared {
  int nh = 0, nw = 0;
  char* blob = nullptr;
  int32_t *bounds_h = nullptr, *kk_h = nullptr, *bounds_v = nullptr, *kk_v = nullptr;  // of the passes that run: nh != h, nw != w
  int ksize_h = 0, ksize_v = 0;
  uint8_t *tmp_h = nullptr, *tmp_v = nullptr;
  void* emb = nullptr;      // a lane's embedding lives from lmx_sam_lane_encode to lmx_sam_lane_decode
  float* tokens = nullptr;  // [max_batch, DT, DD]: the constant rows are copied in at prepare
  float *logits = nullptr, *post = nullptr;  // where the caller passes no lowres; mask_post's intermediate
  uint8_t* mask = nullptr;                   // where the caller passes no mask
  void* contour_ws = nullptr;                // null: the frame size is outside lmx_k_contour_features' range
  LmxArena enc, dec, one[S_N];               // encode_chunk's and decode_chunk's buffers, and the shared regions
  LmxArena h_stream, h_scratch;              // encoder Hiera: the two arenas of HieraRun
  const HieraBandTable* table = nullptr;     // ... and the geometry's band table (null: no band)
};

// one walk of encode_chunk / decode_chunk
struct SamRun : HieraRun {
  LmxArena enc, dec, one[S_N];
  SamRun(const char* fn_, bool launch_, hipStream_t st_) { fn = fn_, launch = launch_, st = st_, model = "SAM"; }
  // a launching run over a prepared workspace
  SamRun(const char* fn_, const Prepared& P, hipStream_t st_) : SamRun(fn_, true, st_) {
    enc = P.enc, dec = P.dec, stream = P.h_stream, scratch = P.h_scratch;
    for (int i = 0; i < S_N; ++i) one[i] = P.one[i];
  }
};

}  // namespace

struct lmx_sam : LmxHandleCore {
  LmxSamCfg cfg;
  Lin pe[2], n1[2];
  const void *n2_w = nullptr, *n2_hi = nullptr, *n2_lo = nullptr;
  const float *pos = nullptr, *lut = nullptr;
  Norm n1_ln, n2_ln;
  std::vector<EncLayer> layers;
  const float *gauss = nullptr, *corner = nullptr, *key_pe = nullptr, *no_mask = nullptr, *out_tokens = nullptr;
  DecPlan dec[2];
  Norm ln_final, up_ln;
  std::map<std::tuple<int, int, int>, Prepared> prepared;               // lane 0: the workspace of the public lmx_sam_* calls
  std::map<std::tuple<int, int, int>, std::vector<Prepared>> more_lanes;  // lanes 1 ..: further workspaces over the same weights (sam_lanes.h)
  HieraW hiera;                                                // encoder Hiera
  std::map<std::pair<int, int>, HieraBandTable> band_tables;  // ... per resized geometry (nh, nw), shared by both plans
  bool is_hiera() const { return cfg.encoder == LMX_SAM_ENC_HIERA; }
};

namespace {

void destroy(lmx_sam* m) {
  for (auto& kv : m->prepared) (void)hipFree(kv.second.blob);
  for (auto& kv : m->more_lanes)
    for (Prepared& P : kv.second) (void)hipFree(P.blob);
  for (auto& kv : m->band_tables) (void)hipFree(kv.second.blob);
  lmx_handle_free(m);
  delete m;
}

int open_into(lmx_sam* m, const char* path) {
  LmxSamImage img;
  LMX_TRY(lmx_sam_image_parse(path, &img));
  m->cfg = img.cfg;
  const LmxSamCfg& c = m->cfg;
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_sam_open_host", path, img.data_offset, img.file_bytes));
  const uint64_t base = img.data_offset;
  auto at = [&](const LmxTensorRef& r) -> const void* { return r.nbytes ? m->weights + (r.offset - base) : nullptr; };
  auto f32 = [&](const LmxTensorRef& r) { return static_cast<const float*>(at(r)); };
  auto norm = [&](const LmxSamNorm& n) { return Norm{f32(n.g), f32(n.b)}; };
  const int D = c.hidden, I = c.mlp, Kp = c.patch * c.patch * 3, C = c.out_ch;
  m->lut = f32(img.lut);
  if (m->is_hiera()) {
    HieraW& W = m->hiera;
    W.cfg = c.hiera;
    W.n_blocks = (int)img.hiera_blocks.size();
    W.pe_w = at(img.pe_w);
    W.pe_b = f32(img.pe_b);
    W.pos = f32(img.pos);
    auto f16 = [&](const LmxTensorRef& r) { return static_cast<const half_t*>(at(r)); };
    for (int i = 0; i < W.n_blocks; ++i) {
      const LmxHieraBlockRefs& r = img.hiera_blocks[(size_t)i];
      HieraBlockW B;
      B.shape = r.shape;
      B.fused = r.fused;
      if (r.shape.win == 0 && W.first_global < 0) W.first_global = i;
      B.g1 = f32(r.g1), B.b1 = f32(r.b1), B.bqkv = f32(r.bqkv), B.bo = f32(r.bo), B.g2 = f32(r.g2), B.b2 = f32(r.b2), B.bb1 = f32(r.bb1), B.bb2 = f32(r.bb2);
      B.bp = f32(r.bp);
      B.wqkv = f16(r.wqkv), B.padkv = f16(r.padkv), B.wo = f16(r.wo), B.w1 = f16(r.w1), B.w2 = f16(r.w2), B.wp = f16(r.wp);
      for (int j = 0; j < 4; ++j) B.attn[j] = at(r.attn[j]);
      for (int j = 0; j < 2; ++j) B.mlp_img[j] = at(r.mlp_img[j]);
      W.blocks.push_back(B);
    }
    for (int s = 0; s < LMX_HIERA_MAX_STAGES; ++s) W.neck_w[s] = at(img.neck_w[s]), W.neck_b[s] = f32(img.neck_b[s]);
  }
  m->pe[LMX_SAM_F16] = Lin{at(img.pe_w), f32(img.pe_b), nullptr, D, Kp};
  m->pe[LMX_SAM_EXACT] = Lin{at(img.x_pe), f32(img.pe_b), nullptr, D, Kp};
  m->n1[LMX_SAM_F16] = Lin{at(img.n1_w), nullptr, nullptr, C, D};
  m->n1[LMX_SAM_EXACT] = Lin{at(img.x_n1), nullptr, nullptr, C, D};
  m->n2_w = at(img.n2_w);
  m->n2_hi = at(img.x_n2_hi);
  m->n2_lo = at(img.x_n2_lo);
  m->pos = f32(img.pos);
  m->lut = f32(img.lut);
  m->n1_ln = Norm{f32(img.n1_g), f32(img.n1_b)};
  m->n2_ln = Norm{f32(img.n2_g), f32(img.n2_b)};
  for (int i = 0; i < (m->is_hiera() ? 0 : c.layers); ++i) {
    const LmxSamLayerRefs& r = img.layers[(size_t)i];
    EncLayer L;
    L.glob = c.is_global(i);
    L.g1 = f32(r.g1);
    L.b1 = f32(r.b1);
    L.rh = f32(r.rh);
    L.rw = f32(r.rw);
    L.g2 = f32(r.g2);
    L.b2 = f32(r.b2);
    L.padkv = static_cast<const half_t*>(at(r.padkv));
    L.qkv[LMX_SAM_F16] = Lin{at(r.wqkv), f32(r.bqkv), nullptr, 3 * D, D};
    L.qkv[LMX_SAM_EXACT] = Lin{at(r.xqkv), f32(r.bqkv), nullptr, 3 * D, D};
    L.proj[LMX_SAM_F16] = Lin{at(r.wo), f32(r.bo), nullptr, D, D};
    L.proj[LMX_SAM_EXACT] = Lin{at(r.xproj), f32(r.bo), nullptr, D, D};
    L.fc1[LMX_SAM_F16] = Lin{at(r.w1), f32(r.bb1), nullptr, I, D};
    L.fc1[LMX_SAM_EXACT] = Lin{at(r.xfc1), f32(r.bb1), nullptr, I, D};
    L.fc2[LMX_SAM_F16] = Lin{at(r.w2), f32(r.bb2), nullptr, D, I};
    L.fc2[LMX_SAM_EXACT] = Lin{at(r.xfc2), f32(r.bb2), nullptr, D, I};
    m->layers.push_back(L);
  }
  m->gauss = f32(img.gauss);
  m->corner = f32(img.corner);
  m->key_pe = f32(img.key_pe);
  m->no_mask = f32(img.no_mask);
  m->out_tokens = f32(img.out_tokens);
  m->ln_final = norm(img.ln_final);
  m->up_ln = norm(img.up_ln);
  // the decoder's Linears: lmx_sam_linears()'s order, walked once per plan
  for (int plan = 0; plan < 2; ++plan) {
    size_t at_lin = 0;
    auto next = [&]() {
      const LmxSamLinear& l = img.linears[at_lin++];
      return plan == LMX_SAM_F16 ? Lin{at(l.w), f32(l.b), nullptr, l.N, l.K} : Lin{at(l.xw), f32(l.xb), f32(l.xs), l.N, l.K};
    };
    auto attn = [&](DecAttn* a) {
      a->q = next();
      a->k = next();
      a->v = next();
      a->o = next();
    };
    DecPlan& P = m->dec[plan];
    for (int i = 0; i < 2; ++i) {
      attn(&P.L[i].sa);
      attn(&P.L[i].t2i);
      P.L[i].lin1 = next();
      P.L[i].lin2 = next();
      attn(&P.L[i].i2t);
      for (int j = 0; j < 4; ++j) P.L[i].ln[j] = norm(img.dec_ln[i][j]);
    }
    attn(&P.fin);
    P.up1 = next();
    P.up2 = next();
    for (int j = 0; j < 3; ++j) P.hyp[j] = next();
    for (int j = 0; j < 3; ++j) P.iou[j] = next();
    LMX_REQUIRE(at_lin == img.linears.size(), "lmx_sam_open_host: the decoder's plan reads %d Linears, the image lists %d", (int)at_lin,
                (int)img.linears.size());
  }
  return LMX_OK;
}

int check_precision(const lmx_sam* m, const char* fn, int precision) {
  LMX_REQUIRE(precision == LMX_SAM_F16 || precision == LMX_SAM_EXACT, "%s: precision %d is neither LMX_SAM_F16 (0) nor LMX_SAM_EXACT (1)", fn, precision);
  LMX_REQUIRE(m->cfg.plans & (1 << precision), "%s: the image does not hold the %s plan (plans mask %d)", fn, precision == LMX_SAM_F16 ? "f16" : "exact",
              m->cfg.plans);
  return LMX_OK;
}

// one axis of ResizeLongestSide's PIL bilinear resize (lmx/sam.py _tables: resample.coeff_tables); nothing where the size is kept
int pil_axis(int in_size, int out_size, std::vector<int32_t>* bounds, std::vector<int32_t>* kk, int* ksize) {
  if (in_size == out_size) return LMX_OK;
  LMX_TRY(lmx_h_pil_tables(in_size, out_size, LMX_FILT_BILINEAR, nullptr, nullptr, 0, ksize));
  bounds->resize((size_t)out_size * 2);
  kk->resize((size_t)out_size * *ksize);
  return lmx_h_pil_tables(in_size, out_size, LMX_FILT_BILINEAR, bounds->data(), kk->data(), (int64_t)kk->size(), ksize);
}

// ---- encoder Hiera ---------------------------------------------------------------------------------------------------------------
// the plan of a chunk of n frames resized to nh x nw, as HieraEncoder(band="blocks").encode(outputs="embedding") computes it
int hiera_plan_of(const lmx_sam* m, const char* fn, int n, int nh, int nw, std::vector<lmx_hiera_block_t>* plan, std::vector<int>* rows) {
  const HieraW& W = m->hiera;
  plan->assign((size_t)W.n_blocks, lmx_hiera_block_t());
  rows->assign((size_t)W.n_blocks, 0);
  LMX_TRY(lmx_h_hiera_plan(&W.cfg, n, nh, nw, 2, plan->data(), rows->data()));
  for (int i = 0; i < W.n_blocks; ++i)
    LMX_REQUIRE(!(*plan)[(size_t)i].join_out, "%s: block %d ends a kept stage inside the band (the first global block lies behind the embedding's stage): not served",
                fn, i);
  return LMX_OK;
}

// one counting pass: the arenas' peaks for a plan
int hiera_count(const lmx_sam* m, const char* fn, const lmx_hiera_block_t* plan, int n, const HieraBandTable* table, int stop_at, const int* have,
                const int* need, size_t* stream, size_t* scratch) {
  HieraRun R;
  R.fn = fn;
  LMX_TRY(hiera_trunk(R, m->hiera, plan, nullptr, n, table, nullptr, stop_at, have, need, nullptr));
  if (R.stream.peak > *stream) *stream = R.stream.peak;
  if (R.scratch.peak > *scratch) *scratch = R.scratch.peak;
  return LMX_OK;
}

// HieraEncoder._band_table for the rows `rows` of a geometry: ONE whole-grid pass of one frame up to the last block with a join in
// front, keeping rows [have, need) of the stream entering each such block.  The rows it keeps do not depend on the frame's content
// (no pixel reaches them), so the frame is all zeros.  The pass has buffers of its own, freed when it is done.  SYNCHRONOUS.
int hiera_build_table(lmx_sam* m, int nh, int nw, const std::vector<lmx_hiera_block_t>& band, const std::vector<int>& rows, HieraBandTable* T) {
  const HieraW& W = m->hiera;
  const int nb = W.n_blocks, g = W.cfg.image / 4;
  std::vector<int> whole_rows((size_t)nb), have((size_t)nb, 0), need((size_t)nb, 0);
  std::vector<lmx_hiera_block_t> whole((size_t)nb);
  for (int i = 0, r = g; i < nb; ++i) {
    whole_rows[(size_t)i] = r;
    if (W.blocks[(size_t)i].shape.qs) r /= 2;
  }
  LMX_TRY(lmx_h_hiera_plan_rows(&W.cfg, 1, whole_rows.data(), 2, whole.data()));
  int stop_at = -1;
  LmxLayout lay;
  std::vector<size_t> offs((size_t)nb, 0);
  for (int i = 0; i < nb; ++i)
    if (band[(size_t)i].join) {
      have[(size_t)i] = band[(size_t)i].join;
      need[(size_t)i] = band[(size_t)i].H;
      offs[(size_t)i] = lay.add((size_t)(need[(size_t)i] - have[(size_t)i]) * band[(size_t)i].W * W.blocks[(size_t)i].shape.dim * 4);
      stop_at = i;
    }
  LMX_REQUIRE(stop_at >= 0, "lmx_sam_prepare: a band without a join");
  size_t stream = 0, scratch = 0;
  LMX_TRY(hiera_count(m, "lmx_sam_prepare", whole.data(), 1, nullptr, stop_at, have.data(), need.data(), &stream, &scratch));
  const int64_t patch_bytes = (int64_t)g * g * HIERA_KPAD_COLS * 2;
  LMX_REQUIRE(patch_bytes < LMX_MAX_BUFFER_BYTES, "lmx_sam_prepare: buffer 'patches of the table pass' has %lld bytes, the kernels index below 2 GB",
              (long long)patch_bytes);
  LmxLayout tmp;
  const size_t o_frame = tmp.add((size_t)nh * nw * 3), o_patches = tmp.add((size_t)patch_bytes), o_stream = tmp.add(stream), o_scratch = tmp.add(scratch);
  char *work = nullptr, *blob = nullptr;
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&blob), lay.total));
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&work), tmp.total);
  int rc = LMX_OK;
  if (e == hipSuccess) e = hipMemset(work + o_frame, 0, (size_t)nh * nw * 3);
  if (e == hipSuccess) {
    std::vector<float*> taps((size_t)nb, nullptr);
    for (int i = 0; i < nb; ++i)
      if (need[(size_t)i]) taps[(size_t)i] = reinterpret_cast<float*>(blob + offs[(size_t)i]);
    HieraRun R;
    R.launch = true;
    R.fn = "lmx_sam_prepare";
    R.stream.base = work + o_stream, R.stream.cap = stream;
    R.scratch.base = work + o_scratch, R.scratch.cap = scratch;
    rc = lmx_k_im2col_u8(reinterpret_cast<const uint8_t*>(work + o_frame), m->lut, work + o_patches, 1, nh, nw, W.cfg.image, W.cfg.image, 7, 7, 4, 3,
                         HIERA_KPAD_COLS, nullptr);
    if (rc == LMX_OK) rc = hiera_trunk(R, W, whole.data(), work + o_patches, 1, nullptr, nullptr, stop_at, have.data(), need.data(), taps.data());
    e = hipDeviceSynchronize();
  }
  (void)hipFree(work);
  if (e != hipSuccess || rc != LMX_OK) {
    (void)hipFree(blob);
    if (rc != LMX_OK) return rc;
    LMX_HIP(e);
  }
  T->blob = blob;
  T->rows = rows;
  T->x.assign((size_t)nb, nullptr);
  for (int i = 0; i < nb; ++i)
    if (need[(size_t)i]) T->x[(size_t)i] = reinterpret_cast<const float*>(blob + offs[(size_t)i]);
  return LMX_OK;
}

// what lmx_sam_prepare adds for a Hiera handle: P->table (the arenas are sized by build()'s walk of encode_chunk)
int hiera_prepare(lmx_sam* m, int nh, int nw, Prepared* P) {
  const HieraW& W = m->hiera;
  const int g = W.cfg.image / 4;
  std::vector<lmx_hiera_block_t> plan;
  std::vector<int> rows;
  LMX_TRY(hiera_plan_of(m, "lmx_sam_prepare", m->max_batch, nh, nw, &plan, &rows));
  if (m->max_batch > 1) {  // the last chunk of a call may be any size; the pooled GEMM's rule sees it
    std::vector<int> rows1;
    LMX_TRY(hiera_plan_of(m, "lmx_sam_prepare", 1, nh, nw, &plan, &rows1));
    LMX_REQUIRE(rows1 == rows, "lmx_sam_prepare: the band's rows depend on the batch size for a %d x %d frame: not served", nh, nw);
  }
  P->table = nullptr;
  if (rows[0] < g) {
    const auto key = std::make_pair(nh, nw);
    auto it = m->band_tables.find(key);
    if (it == m->band_tables.end()) {  // (a geometry seen under the other plan: a lookup)
      HieraBandTable T;
      LMX_TRY(hiera_build_table(m, nh, nw, plan, rows, &T));
      it = m->band_tables.emplace(key, T).first;
    }
    P->table = &it->second;
  }
  return LMX_OK;
}

// the bytes of an element of the image embedding: f32 from the exact plan's ViT, f16 otherwise (Hiera's is f16 under both plans)
int64_t emb_elt(const lmx_sam* m, int precision) { return precision == LMX_SAM_EXACT && !m->is_hiera() ? 4 : 2; }

// SamVitEncoder.embed's `lin`: one launch either way — f16 weights, or a_rep = 2 over [whi | wlo]
int enc_lin(int precision, const void* a, const Lin& l, void* C, int out_dtype, int M, int act, const void* res, int res_rows, hipStream_t st) {
  const int rep = precision == LMX_SAM_EXACT ? 2 : 1;
  return lmx_gemm_dense_rep(a, l.K, l.w, l.b, C, l.N, out_dtype, M, l.N, rep * l.K, act, nullptr, res, l.N, res_rows, rep, st);
}

// K.conv3x3 of the neck: [n, g, g, C] -> [n, g, g, C], no bias, no activation
int neck_conv(const void* x, const void* w, void* out, int out_dtype, const void* res, int n, int g, int C, hipStream_t st) {
  return lmx_gemm_conv3(x, C, n, g, g, C, w, nullptr, nullptr, out, C, out_dtype, C, LMX_ACT_NONE, 1, res, C, 1, st);
}

// HieraEncoder(band="blocks").encode(frames, outputs="embedding")["fpn"][2] for n <= max_batch frames: emb f16 [n, 64, 64, fpn_dim]
int hiera_encode_chunk(SamRun& R, const lmx_sam* m, const Prepared& P, const uint8_t* img, int n, void* emb) {
  const HieraW& W = m->hiera;
  const int S = W.cfg.image, g = S / 4;
  R.model = "the Hiera encoder";  // whose buffer a refusal names, until decode_chunk
  std::vector<lmx_hiera_block_t> plan;
  std::vector<int> rows;
  LMX_TRY(hiera_plan_of(m, R.fn, n, P.nh, P.nw, &plan, &rows));
  const bool band = rows[0] < g;
  LMX_REQUIRE(!R.launch || !band || (P.table && P.table->rows == rows), "%s: the band's rows for %d frames are not those the table was prepared for", R.fn, n);
  void* patches;  // of the band's top rows
  LMX_TRY(R.take(&R.enc, "patches", (int64_t)n * rows[0] * g * HIERA_KPAD_COLS * 2, &patches));
  LMX_LAUNCH(R, lmx_k_im2col_u8(img, m->lut, patches, n, P.nh, P.nw, band ? 4 * rows[0] : S, S, 7, 7, 4, 3, HIERA_KPAD_COLS, lmx_run_stream(R)));
  R.rewind_to(&R.stream, 0);
  return hiera_trunk(R, W, plan.data(), patches, n, band ? P.table : nullptr, emb, -1, nullptr, nullptr, nullptr);
}

// SamVitEncoder.preprocess + embed for n <= max_batch frames: emb f16 (f16 plan) / f32 (exact plan) [n, g, g, out_ch]
int encode_chunk(SamRun& R, const lmx_sam* m, const Prepared& P, int precision, const uint8_t* frames, int n, int h, int w, void* emb) {
  const LmxSamCfg& c = m->cfg;
  const int D = c.hidden, I = c.mlp, H = c.heads, hd = D / H, g = c.grid(), gg = g * g, rows = n * gg, Kp = c.patch * c.patch * 3, C = c.out_ch, ws = c.window;
  const int64_t r64 = rows;
  const float eps = (float)c.eps, scale = (float)pow((double)hd, -0.5);
  hipStream_t st = lmx_run_stream(R);
  R.rewind_to(&R.enc, 0);
  const uint8_t* img = frames;
  if (P.nw != w) {
    LMX_LAUNCH(R, lmx_k_pil_resize_h(img, P.tmp_h, n, h, w, P.nw, P.bounds_h, P.kk_h, P.ksize_h, 0, st));
    img = P.tmp_h;
  }
  if (P.nh != h) {
    LMX_LAUNCH(R, lmx_k_pil_resize_v(img, P.tmp_v, n, h, P.nh, P.nw, P.bounds_v, P.kk_v, P.ksize_v, st));
    img = P.tmp_v;
  }
  if (m->is_hiera()) return hiera_encode_chunk(R, m, P, img, n, emb);
  void* patches;
  float* x;
  LMX_TRY(R.take(&R.enc, "patches", r64 * Kp * 2, &patches));
  LMX_LAUNCH(R, lmx_k_im2col_u8(img, m->lut, patches, n, P.nh, P.nw, c.image, c.image, c.patch, c.patch, c.patch, 0, Kp, st));
  LMX_TRY(R.take(&R.enc, "residual stream", r64 * D * 4, &x));
  LMX_LAUNCH(R, enc_lin(precision, patches, m->pe[precision], x, LMX_F32, rows, LMX_ACT_NONE, m->pos, gg, st));
  // what every layer writes anew: LayerNorm rows, qkv, attention output, MLP hidden
  half_t *hn, *qkv, *a, *u;
  LMX_TRY(R.take(&R.enc, "LayerNorm rows", r64 * D * 2, &hn));
  LMX_TRY(R.take(&R.enc, "qkv", r64 * 3 * D * 2, &qkv));
  LMX_TRY(R.take(&R.enc, "attention output", r64 * D * 2, &a));
  LMX_TRY(R.take(&R.enc, "MLP hidden", r64 * I * 2, &u));
  const half_t *k = qkv ? qkv + D : nullptr, *v = qkv ? qkv + 2 * D : nullptr;
  for (const EncLayer& L : m->layers) {
    LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, L.g1, L.b1, hn, LMX_F16, D, rows, D, eps, LMX_ACT_NONE, st));
    LMX_LAUNCH(R, enc_lin(precision, hn, L.qkv[precision], qkv, LMX_F16, rows, LMX_ACT_NONE, nullptr, 0, st));
    lmx_attn_desc ad = L.glob ? lmx_attn_flat(qkv, 3 * D, k, v, 3 * D, a, D, n, H, gg, gg, hd, scale)
                              : lmx_attn_windowed(qkv, 3 * D, k, v, 3 * D, a, D, n, H, hd, scale, g, g, ws, false, L.padkv + D, L.padkv + 2 * D);
    const int S = L.glob ? g : ws;
    void* rel;  // f16 [B * H * Tq][2 S], consumed by the attention right behind it
    LMX_TRY(R.share(&R.one[S_REL], "relative-position tables", (int64_t)ad.B * H * ad.Tq * 2 * S * 2, &rel));
    LMX_LAUNCH(R, lmx_k_relpos_tables(&ad, L.rh, L.rw, S, rel, st));
    ad.rel = rel;
    ad.rel_S = S;
    LMX_LAUNCH(R, lmx_k_attention(&ad, st));
    LMX_LAUNCH(R, enc_lin(precision, a, L.proj[precision], x, LMX_F32, rows, LMX_ACT_NONE, x, 0, st));
    LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, L.g2, L.b2, hn, LMX_F16, D, rows, D, eps, LMX_ACT_NONE, st));
    LMX_LAUNCH(R, enc_lin(precision, hn, L.fc1[precision], u, LMX_F16, rows, LMX_ACT_GELU, nullptr, 0, st));
    LMX_LAUNCH(R, enc_lin(precision, u, L.fc2[precision], x, LMX_F32, rows, LMX_ACT_NONE, x, 0, st));
  }
  // neck: 1x1 (no bias) -> LayerNorm2d -> 3x3 (no bias) -> LayerNorm2d
  const bool exact = precision == LMX_SAM_EXACT;
  float* y32;
  void *y16, *acc;
  LMX_LAUNCH(R, lmx_k_cast_f32_f16(x, D, hn, D, rows, D, st));
  LMX_TRY(R.take(&R.enc, "neck 1x1 output", r64 * C * 4, &y32));
  LMX_LAUNCH(R, enc_lin(precision, hn, m->n1[precision], y32, LMX_F32, rows, LMX_ACT_NONE, nullptr, 0, st));
  LMX_TRY(R.take(&R.enc, "neck LayerNorm rows", r64 * C * 2, &y16));
  LMX_LAUNCH(R, lmx_k_layernorm(y32, LMX_F32, C, m->n1_ln.g, m->n1_ln.b, y16, LMX_F16, C, rows, C, 1e-6f, LMX_ACT_NONE, st));
  LMX_TRY(R.take(&R.enc, "neck 3x3 output", r64 * C * (exact ? 4 : 2), &acc));
  if (exact) {  // two accumulating launches of the implicit GEMM (whi, then + wlo), f32 output, f32 embedding
    LMX_LAUNCH(R, neck_conv(y16, m->n2_hi, acc, LMX_F32, nullptr, n, g, C, st));
    LMX_LAUNCH(R, neck_conv(y16, m->n2_lo, acc, LMX_F32, acc, n, g, C, st));
    LMX_LAUNCH(R, lmx_k_layernorm(acc, LMX_F32, C, m->n2_ln.g, m->n2_ln.b, emb, LMX_F32, C, rows, C, 1e-6f, LMX_ACT_NONE, st));
    return LMX_OK;
  }
  LMX_LAUNCH(R, neck_conv(y16, m->n2_w, acc, LMX_F16, nullptr, n, g, C, st));
  LMX_LAUNCH(R, lmx_k_layernorm(acc, LMX_F16, C, m->n2_ln.g, m->n2_ln.b, emb, LMX_F16, C, rows, C, 1e-6f, LMX_ACT_NONE, st));
  return LMX_OK;
}

// ---- the mask decoder: MaskDecoder.lowres, ONE walk.  The precision plan enters in operand / lin / attention / upscale -------------
struct Dec {
  const lmx_sam* m;
  const Prepared& P;
  SamRun& R;
  int n;
  bool exact;

  // an activation as a Linear reads it: f16 rows (f16 plan) or f32 rows (exact plan), ld in elements
  struct Opd {
    const void* p;
    int64_t ld;
  };
  int mid() const { return exact ? LMX_F32 : LMX_F16; }  // what travels between two Linears ...
  int64_t mid_bytes() const { return exact ? 4 : 2; }    // ... and the bytes of one element of it
  hipStream_t st() const { return lmx_run_stream(R); }
  // [rows][cols] of esz-byte elements from the decoder's arena
  template <class T>
  int buf(const char* what, int64_t rows, int64_t cols, int64_t esz, T** out) const {
    return R.take(&R.dec, what, rows * cols * esz, out);
  }

  int ln(const float* x, const Norm& g, float eps, void* y, int out_dtype, int64_t rows, int D, int act) const {
    LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, g.g, g.b, y, out_dtype, D, (int)rows, D, eps, act, st()));
    return LMX_OK;
  }
  int add(const void* a, int a_dtype, const float* b, int64_t b_rows, void* out, int out_dtype, int64_t rows) const {
    LMX_LAUNCH(R, lmx_k_add_bcast(a, a_dtype, DD, b, DD, (int)b_rows, out, out_dtype, DD, rows, DD, st()));
    return LMX_OK;
  }
  // the plans' operand(x, pe): x + pe in `buf`; without pe a cast into `buf` (f16 plan) or x where it lies (exact plan: no launch)
  int operand(const float* x, int64_t ldx, const float* pe, int64_t pe_rows, void* buf, int64_t rows, Opd* out) const {
    *out = pe || !exact ? Opd{buf, DD} : Opd{x, ldx};
    if (pe) return add(x, LMX_F32, pe, pe_rows, buf, mid(), rows);
    if (!exact) LMX_LAUNCH(R, lmx_k_cast_f32_f16(x, ldx, buf, DD, rows, DD, st()));
    return LMX_OK;
  }
  // the plans' linear: K.gemm on (w f16, b), or the x3 rows of act_in(a), then ONE GEMM over 3 K with the row scale and f32 output.
  // The x3 operand [rows][3 K] f16 is consumed by the GEMM right behind the split: one region serves every Linear
  int lin(Opd a, int64_t rows, const Lin& l, void* out, int out_dtype, int act = LMX_ACT_NONE, const float* res = nullptr, int act_in = LMX_ACT_NONE) const {
    if (!exact) {
      LMX_LAUNCH(R, lmx_gemm_dense(a.p, l.K, l.w, l.b, out, l.N, out_dtype, (int)rows, l.N, l.K, act, nullptr, res, l.N, st()));
      return LMX_OK;
    }
    void* x3;
    LMX_TRY(R.share(&R.one[S_X3], "x3 operand", rows * 3 * l.K * 2, &x3));
    LMX_LAUNCH(R, lmx_k_split3(static_cast<const float*>(a.p), a.ld, act_in, nullptr, 0, x3, 3 * l.K, rows, l.K, l.K, 1, 0, st()));
    LMX_LAUNCH(R, lmx_gemm_dense(x3, 3 * l.K, l.w, l.b, out, l.N, LMX_F32, (int)rows, l.N, 3 * l.K, act, l.s, res, l.N, st()));
    return LMX_OK;
  }
  // MaskDecoder._attn: q / k / v projections, attention over 8 heads, out projection (+ res) in f32.  The projections and the
  // attention's output die with the call: one region each serves every attention
  int attn(const DecAttn& W, Opd q, Opd k, Opd v, int tq, int tk, const float* res, float* out) const {
    const int inner = W.q.N, hd = inner / DH;
    const int64_t rq = (int64_t)n * tq, rk = (int64_t)n * tk, e = mid_bytes();
    const float scale = (float)pow((double)hd, -0.5);
    void *pq, *pk, *pv, *pa;
    LMX_TRY(R.share(&R.one[S_PQ], "q projection", rq * inner * e, &pq));
    LMX_TRY(lin(q, rq, W.q, pq, mid()));
    LMX_TRY(R.share(&R.one[S_PK], "k projection", rk * inner * e, &pk));
    LMX_TRY(lin(k, rk, W.k, pk, mid()));
    LMX_TRY(R.share(&R.one[S_PV], "v projection", rk * inner * e, &pv));
    LMX_TRY(lin(v, rk, W.v, pv, mid()));
    LMX_TRY(R.share(&R.one[S_PA], "decoder attention output", rq * inner * e, &pa));
    if (exact) {
      auto f = [](void* p) { return static_cast<float*>(p); };
      LMX_LAUNCH(R, lmx_k_attention_f32(f(pq), inner, f(pk), inner, f(pv), inner, f(pa), inner, n, DH, tq, tk, hd, scale, st()));
    } else {
      const lmx_attn_desc ad = lmx_attn_flat(pq, inner, pk, pv, inner, pa, inner, n, DH, tq, tk, hd, scale);
      LMX_LAUNCH(R, lmx_k_attention(&ad, st()));
    }
    return lin(Opd{pa, inner}, rq, W.o, out, LMX_F32, LMX_ACT_NONE, res);
  }
  // MaskDecoder._ffn: three Linears on n rows
  int ffn(const Lin* l, Opd x, float* out) const {
    void *t1, *t2;
    LMX_TRY(R.share(&R.one[S_T1], "hyper MLP", (int64_t)n * l[0].N * mid_bytes(), &t1));
    LMX_TRY(lin(x, n, l[0], t1, mid(), LMX_ACT_RELU));
    LMX_TRY(R.share(&R.one[S_T2], "hyper MLP", (int64_t)n * l[1].N * mid_bytes(), &t2));
    LMX_TRY(lin(Opd{t1, l[0].N}, n, l[1], t2, mid(), LMX_ACT_RELU));
    return lin(Opd{t2, l[1].N}, n, l[2], out, LMX_F32);
  }
  // the upscaler of the plans' upscale_and_mask: per-pixel GEMMs, LayerNorm2d row-wise on the [.., quadrant, 64] view, pixel shuffle
  // deferred.  The two GELUs sit in the epilogues of the LayerNorm and of the second GEMM (f16 plan), or, exact, in the next split and
  // in the final dot product.  *u2: [nP * 4][W.up2.N] of mid()
  int upscale(const DecPlan& W, Opd x, int64_t nP, void** u2) const {
    const float eps = 1e-6f;
    float* u1;
    void* u1n;
    LMX_TRY(buf("upscaler 1", nP, W.up1.N, 4, &u1));
    LMX_TRY(lin(x, nP, W.up1, u1, LMX_F32));
    LMX_TRY(buf("upscaler LayerNorm rows", nP * 4, 64, mid_bytes(), &u1n));
    LMX_TRY(buf("upscaler 2", nP * 4, W.up2.N, mid_bytes(), u2));
    if (exact) {
      LMX_TRY(ln(u1, m->up_ln, eps, u1n, LMX_F32, nP * 4, 64, LMX_ACT_NONE));
      return lin(Opd{u1n, 64}, nP * 4, W.up2, *u2, LMX_F32, LMX_ACT_NONE, nullptr, LMX_ACT_GELU);
    }
    LMX_TRY(ln(u1, m->up_ln, eps, u1n, LMX_F16, nP * 4, 64, LMX_ACT_GELU));
    return lin(Opd{u1n, 64}, nP * 4, W.up2, *u2, LMX_F16, LMX_ACT_GELU);
  }

  // MaskDecoder.lowres: emb f16 (f16 plan, Hiera) / f32 [n * G * G, 256] -> logits f32 [n, 4G, 4G], *iou4 f32 [n, 4]
  int lowres(const void* emb, float* logits, float** iou4) const {
    const DecPlan& W = m->dec[exact ? LMX_SAM_EXACT : LMX_SAM_F16];
    const int G = m->cfg.grid(), Pn = G * G, T = DT;
    const int64_t nT = (int64_t)n * T, nP = (int64_t)n * Pn, e = mid_bytes();
    const float eps = 1e-6f;
    // the f32 queries and keys, each with the spare a LayerNorm or a residual Linear writes: x = LayerNorm(y) / x = y, and the
    // ping-pong buffers flip behind every launch that writes one
    float *queries, *spare, *keys, *kspare;
    LMX_TRY(buf("queries", nT, DD, 4, &queries));
    LMX_TRY(buf("queries", nT, DD, 4, &spare));
    LMX_TRY(buf("keys", nP, DD, 4, &keys));
    LMX_TRY(buf("keys", nP, DD, 4, &kspare));
    auto flip = [](float*& a, float*& b) {
      float* t = a;
      a = b;
      b = t;
    };
    auto norm = [&](float*& x, float*& other, const Norm& g, float e, int64_t rows) {
      LMX_TRY(ln(x, g, e, other, LMX_F32, rows, DD, LMX_ACT_NONE));
      flip(x, other);
      return (int)LMX_OK;
    };
    // queries + qpe, keys + key_pe and the bare queries / keys, each in its own buffer (kk is read twice, kc16 by the upscaler); the
    // exact plan reads the bare ones where they lie
    void *qq, *kk, *qc16 = nullptr, *kc16 = nullptr, *tok16 = nullptr, *hh;
    LMX_TRY(buf("queries + position", nT, DD, e, &qq));
    LMX_TRY(buf("keys + position", nP, DD, e, &kk));
    if (!exact) {
      LMX_TRY(buf("queries f16", nT, DD, 2, &qc16));
      LMX_TRY(buf("keys f16", nP, DD, 2, &kc16));
      LMX_TRY(buf("token f16", n, DD, 2, &tok16));
    }
    LMX_TRY(buf("decoder MLP hidden", nT, LMX_SAM_DEC_MLP, e, &hh));  // written anew by both layers
    auto q_pe = [&](Opd* o) { return operand(queries, DD, P.tokens, nT, qq, nT, o); };
    auto k_pe = [&](Opd* o) { return operand(keys, DD, m->key_pe, Pn, kk, nP, o); };
    auto q_in = [&](Opd* o) { return operand(queries, DD, nullptr, 0, qc16, nT, o); };
    auto k_in = [&](Opd* o) { return operand(keys, DD, nullptr, 0, kc16, nP, o); };
    Opd q, k, v;
    LMX_TRY(add(emb, emb_elt(m, exact ? LMX_SAM_EXACT : LMX_SAM_F16) == 4 ? LMX_F32 : LMX_F16, m->no_mask, 1, keys, LMX_F32, nP));
    for (int i = 0; i < 2; ++i) {
      const DecLayer& L = W.L[i];
      if (i == 0) {
        LMX_TRY(operand(P.tokens, DD, nullptr, 0, qq, nT, &q));
        LMX_TRY(attn(L.sa, q, q, q, T, T, nullptr, queries));
      } else {
        LMX_TRY(q_pe(&q));
        LMX_TRY(q_in(&v));
        LMX_TRY(attn(L.sa, q, q, v, T, T, queries, spare));
        flip(queries, spare);
      }
      LMX_TRY(norm(queries, spare, L.ln[0], eps, nT));
      LMX_TRY(q_pe(&q));
      LMX_TRY(k_pe(&k));
      LMX_TRY(k_in(&v));
      LMX_TRY(attn(L.t2i, q, k, v, T, Pn, queries, spare));
      flip(queries, spare);
      LMX_TRY(norm(queries, spare, L.ln[1], eps, nT));
      LMX_TRY(q_in(&v));
      LMX_TRY(lin(v, nT, L.lin1, hh, mid(), LMX_ACT_RELU));
      LMX_TRY(lin(Opd{hh, LMX_SAM_DEC_MLP}, nT, L.lin2, spare, LMX_F32, LMX_ACT_NONE, queries));
      flip(queries, spare);
      LMX_TRY(norm(queries, spare, L.ln[2], eps, nT));
      LMX_TRY(q_pe(&q));
      // (keys have not changed since the token-to-image attention above: k is still keys + key_pe)
      LMX_TRY(q_in(&v));
      LMX_TRY(attn(L.i2t, k, q, v, Pn, T, keys, kspare));
      flip(keys, kspare);
      LMX_TRY(norm(keys, kspare, L.ln[3], eps, nP));
    }
    LMX_TRY(q_pe(&q));
    LMX_TRY(k_pe(&k));
    LMX_TRY(k_in(&v));  // the final attention's values and the upscaler's input
    LMX_TRY(attn(W.fin, q, k, v, T, Pn, queries, spare));
    flip(queries, spare);
    LMX_TRY(norm(queries, spare, m->ln_final, 1e-5f, nT));
    Opd iou_tok, mask_tok;
    void* u2;
    float* hyper;
    LMX_TRY(operand(queries, (int64_t)T * DD, nullptr, 0, tok16, n, &iou_tok));  // q3[:, 0]: the iou token, ahead of the upscaler
    LMX_TRY(upscale(W, v, nP, &u2));
    LMX_TRY(operand(queries ? queries + DD : nullptr, (int64_t)T * DD, nullptr, 0, qc16, n, &mask_tok));  // q3[:, 1]: mask token 0, behind it
    LMX_TRY(buf("hyper", n, W.hyp[2].N, 4, &hyper));
    LMX_TRY(ffn(W.hyp, mask_tok, hyper));
    if (exact)
      LMX_LAUNCH(R, lmx_k_hyper_mask_multi_f32(static_cast<const float*>(u2), hyper, logits, n, 1, G, 32, LMX_ACT_GELU, st()));
    else
      LMX_LAUNCH(R, lmx_k_hyper_mask_multi(u2, hyper, logits, n, 1, G, 32, st()));
    LMX_TRY(buf("iou head", n, W.iou[2].N, 4, iou4));
    return ffn(W.iou, iou_tok, *iou4);
  }
};

// MaskDecoder.predict (+ pack_bits, contour_features) for n <= max_batch frames, writing the chunk's rows of the outputs
int decode_chunk(SamRun& R, const lmx_sam* m, const Prepared& P, int precision, const void* emb, int n, int h, int w, const float* boxes, int64_t ldb,
                 uint8_t* mask, uint8_t* mask_bits, int64_t* stats, int64_t* contour, float* iou, float* lowres) {
  const LmxSamCfg& c = m->cfg;
  const int L = 4 * c.grid();
  hipStream_t st = lmx_run_stream(R);
  uint8_t* mk = mask ? mask : P.mask;
  float *logits = lowres ? lowres : P.logits, *sparse, *iou4;
  R.rewind_to(&R.dec, 0);
  R.model = "SAM";
  LMX_TRY(R.take(&R.dec, "sparse prompt", (int64_t)n * 2 * DD * 4, &sparse));
  LMX_LAUNCH(R, lmx_k_prompt_box(boxes, ldb, sparse, n, (double)P.nw / (double)w, (double)P.nh / (double)h, (float)c.image, m->gauss, m->corner, DD / 2, st));
  // torch.cat([out_tokens, sparse], 1): the output-token rows are in place since prepare
  if (R.launch)
    LMX_HIP(hipMemcpy2DAsync(P.tokens + LMX_SAM_OUT_TOKENS * DD, (size_t)DT * DD * 4, sparse, (size_t)2 * DD * 4, (size_t)2 * DD * 4, (size_t)n,
                             hipMemcpyDeviceToDevice, st));
  LMX_TRY((Dec{m, P, R, n, precision == LMX_SAM_EXACT}.lowres(emb, logits, &iou4)));
  LMX_LAUNCH(R, lmx_k_mask_post(logits, n, L, c.image, P.nh, P.nw, h, w, mk, stats, P.post, st));
  if (R.launch) LMX_HIP(hipMemcpy2DAsync(iou, 4, iou4, 16, 4, (size_t)n, hipMemcpyDeviceToDevice, st));  // iou[:, 0]
  if (mask_bits) LMX_LAUNCH(R, lmx_k_pack_bits(mk, (int64_t)n * h, w, mask_bits, st));
  if (contour) LMX_LAUNCH(R, lmx_k_contour_features(mk, n, h, w, contour, P.contour_ws, st));
  return LMX_OK;
}

// one workspace of max_batch frames for (h, w, precision): what lmx_sam_prepare keeps as lane 0 and lmx_sam_lanes_prepare as every further lane
int build(lmx_sam* m, int h, int w, int precision, Prepared* built) {
  const LmxSamCfg& c = m->cfg;
  Prepared P;
  lmx_sam_resized_hw(c.image, h, w, &P.nh, &P.nw);
  LMX_REQUIRE(P.nh >= 1 && P.nw >= 1 && P.nh <= c.image && P.nw <= c.image, "lmx_sam_prepare: a %d x %d frame resizes to %d x %d", h, w, P.nh, P.nw);
  const int nh = P.nh, nw = P.nw;
  std::vector<int32_t> bh, kh, bv, kv;
  LMX_TRY(pil_axis(w, nw, &bh, &kh, &P.ksize_h));
  LMX_TRY(pil_axis(h, nh, &bv, &kv, &P.ksize_v));
  // the arenas: ONE counting walk of encode + decode at max_batch; a Hiera plan can depend on n (the last chunk of a call may be any
  // size; the pooled GEMM's rule sees it), so its encoder is also walked for a single frame
  const int B = m->max_batch;
  SamRun R("lmx_sam_prepare", false, nullptr);
  LMX_TRY(encode_chunk(R, m, P, precision, nullptr, B, h, w, nullptr));
  if (m->is_hiera() && B > 1) LMX_TRY(encode_chunk(R, m, P, precision, nullptr, 1, h, w, nullptr));
  LMX_TRY(decode_chunk(R, m, P, precision, nullptr, B, h, w, nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  // The blob, in the order of the plan: a field — what outlives a call or is written at prepare, refused by name from 2 GB on like the
  // walk's buffers — or an arena as the walk counted it (an arena holds many buffers, each checked where it is taken)
  const int64_t gg = (int64_t)c.grid() * c.grid(), L = 4 * c.grid();
  int64_t contour = 0;
  if (h > 1 && w > 1 && (int64_t)h * w <= 0x1fffff && (int64_t)B * h < 0x7fffffffll && B <= 65535) contour = lmx_contour_workspace_bytes(B, h, w);
  auto vp = [](auto** p) { return reinterpret_cast<void**>(p); };
  struct Part {
    void** ptr;  // a field ...
    const char* what;
    int64_t bytes;
    const void* src;          // host data to copy in, or null
    const LmxArena* counted;  // ... or an arena of the counting run and the prepared entry's copy of it
    LmxArena* kept;
  };
  auto arena = [](const LmxArena& counted, LmxArena* kept) { return Part{nullptr, nullptr, 0, nullptr, &counted, kept}; };
  auto one = [&](int i) { return arena(R.one[i], &P.one[i]); };
  const Part parts[] = {
      {vp(&P.bounds_h), "resize table", (int64_t)bh.size() * 4, bh.data()},
      {vp(&P.kk_h), "resize table", (int64_t)kh.size() * 4, kh.data()},
      {vp(&P.bounds_v), "resize table", (int64_t)bv.size() * 4, bv.data()},
      {vp(&P.kk_v), "resize table", (int64_t)kv.size() * 4, kv.data()},
      {vp(&P.tmp_h), "frame after the horizontal resize", nw != w ? (int64_t)B * h * nw * 3 : 0},
      {vp(&P.tmp_v), "resized frame", nh != h ? (int64_t)B * nh * nw * 3 : 0},
      arena(R.enc, &P.enc),
      one(S_REL),
      {vp(&P.emb), "image embedding", B * gg * c.out_ch * emb_elt(m, precision)},
      {vp(&P.tokens), "tokens", (int64_t)B * DT * DD * 4},
      arena(R.dec, &P.dec),
      one(S_PQ), one(S_PK), one(S_PV), one(S_PA), one(S_T1), one(S_T2), one(S_X3),
      {vp(&P.logits), "low-resolution logits", B * L * L * 4},
      {vp(&P.post), "mask_post intermediate", (int64_t)B * nh * nw * 4},
      {vp(&P.mask), "mask", (int64_t)B * h * w},
      {vp(&P.contour_ws), "contour workspace", contour},
      arena(R.stream, &P.h_stream),
      arena(R.scratch, &P.h_scratch),
  };
  const int np = (int)(sizeof(parts) / sizeof(parts[0]));
  LmxLayout lay;
  size_t offs[np], bytes[np];
  LmxUpload up[np];
  for (int i = 0; i < np; ++i) {
    const Part& p = parts[i];
    LmxArena check;
    void* none;
    if (!p.kept && p.bytes) LMX_TRY(R.take(&check, p.what, p.bytes, &none));
    bytes[i] = p.kept ? p.counted->peak : (size_t)p.bytes;
    offs[i] = lay.add(bytes[i]);
    up[i] = LmxUpload{offs[i], p.src, p.src ? bytes[i] : 0};
  }
  // encoder Hiera: the band table of this geometry (built once, shared by both plans).  Last: a workspace refused above costs no pass
  // on the device
  if (m->is_hiera()) LMX_TRY(hiera_prepare(m, nh, nw, &P));
  LMX_TRY(lmx_alloc_and_upload(lay.total, up, np, &P.blob));
  for (int i = 0; i < np; ++i) {
    char* at = bytes[i] ? P.blob + offs[i] : nullptr;
    if (parts[i].kept) *parts[i].kept = LmxArena{at, 0, bytes[i], bytes[i]};
    if (parts[i].ptr) *parts[i].ptr = at;
  }
  // the constant rows of the token buffer: [iou token | 4 mask tokens] in front of every frame's two box corners
  hipError_t err = hipSuccess;
  for (int64_t b = 0; b < B && err == hipSuccess; ++b)
    err = hipMemcpy(P.tokens + b * DT * DD, m->out_tokens, (size_t)LMX_SAM_OUT_TOKENS * DD * 4, hipMemcpyDeviceToDevice);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    (void)hipFree(P.blob);
    LMX_HIP(err);
  }
  *built = P;
  return LMX_OK;
}

int prepare(lmx_sam* m, int h, int w, int precision, const Prepared** out) {
  const auto key = std::make_tuple(h, w, precision);
  const auto it = m->prepared.find(key);
  if (it != m->prepared.end()) {
    if (out) *out = &it->second;
    return LMX_OK;
  }
  LMX_TRY(check_precision(m, "lmx_sam_prepare", precision));
  LMX_REQUIRE((int)m->prepared.size() < LMX_MAX_PREPARED, "lmx_sam_prepare: the handle already holds %d (frame size, plan) pairs; open another for more",
              LMX_MAX_PREPARED);
  Prepared P;
  LMX_TRY(build(m, h, w, precision, &P));
  const auto ins = m->prepared.emplace(key, P);
  if (out) *out = &ins.first->second;
  return LMX_OK;
}

int check_call(const lmx_sam* m, const char* fn, int n, int h, int w, int precision) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0, "%s: n = %d frames", fn, n);
  LMX_REQUIRE(h > 0 && w > 0, "%s: frame size %d x %d", fn, h, w);
  return check_precision(m, fn, precision);
}

int check_decode(const lmx_sam* m, const char* fn, const void* in, const char* in_name, int n, int h, int w, const void* boxes, int precision,
                 const void* stats, const void* contour, const void* iou) {
  LMX_TRY(check_call(m, fn, n, h, w, precision));
  LMX_REQUIRE(in != nullptr, "%s: null pointer (%s)", fn, in_name);
  LMX_REQUIRE(boxes != nullptr, "%s: null pointer (boxes)", fn);
  LMX_REQUIRE(stats != nullptr, "%s: null pointer (stats: mask, mask_bits, contour and lowres may be NULL, stats and iou may not)", fn);
  LMX_REQUIRE(iou != nullptr, "%s: null pointer (iou: mask, mask_bits, contour and lowres may be NULL, stats and iou may not)", fn);
  LMX_REQUIRE(!contour || (h > 1 && w > 1 && (int64_t)h * w <= 0x1fffff),
              "%s: contour features are served for frames of 2 x 2 up to 2^21 - 1 pixels, not %d x %d (pass contour = NULL)", fn, h, w);
  return LMX_OK;
}

// the workspace of `lane` for a prepared (size, plan): a lookup, never an allocation
int lane_of(const lmx_sam* m, const char* fn, int lane, int h, int w, int precision, const Prepared** out) {
  const auto key = std::make_tuple(h, w, precision);
  if (lane == 0) {
    const auto it = m->prepared.find(key);
    LMX_REQUIRE(it != m->prepared.end(), "%s: lane 0 of a %d x %d frame under precision %d is not prepared", fn, h, w, precision);
    *out = &it->second;
    return LMX_OK;
  }
  const auto it = m->more_lanes.find(key);
  LMX_REQUIRE(it != m->more_lanes.end() && lane >= 1 && lane <= (int)it->second.size(), "%s: lane %d of a %d x %d frame under precision %d is not prepared", fn,
              lane, h, w, precision);
  *out = &it->second[(size_t)lane - 1];
  return LMX_OK;
}

}  // namespace

// ---- sam_lanes.h: several passes in flight over one weight upload ------------------------------------------------------------------
int lmx_sam_lanes_ready(const lmx_sam* m, int h, int w, int precision, int lanes) {
  const auto key = std::make_tuple(h, w, precision);
  if (!m->prepared.count(key)) return 0;
  if (lanes <= 1) return 1;
  const auto it = m->more_lanes.find(key);
  return it != m->more_lanes.end() && (int)it->second.size() >= lanes - 1;
}

int lmx_sam_lanes_prepare(lmx_sam* m, int h, int w, int precision, int lanes) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_sam_lanes_prepare"));
  LMX_REQUIRE(h > 0 && w > 0, "lmx_sam_lanes_prepare: frame size %d x %d", h, w);
  LMX_REQUIRE(lanes >= 1 && lanes <= LMX_SAM_MAX_LANES, "lmx_sam_lanes_prepare: %d lanes outside 1 .. %d", lanes, LMX_SAM_MAX_LANES);
  LMX_TRY(prepare(m, h, w, precision, nullptr));  // lane 0, with every check of lmx_sam_prepare
  std::vector<Prepared>& more = m->more_lanes[std::make_tuple(h, w, precision)];
  while ((int)more.size() < lanes - 1) {
    Prepared P;
    LMX_TRY(build(m, h, w, precision, &P));
    more.push_back(P);
  }
  return LMX_OK;
}

int lmx_sam_lane_encode(lmx_sam* m, int lane, const uint8_t* frames, int n, int h, int w, int precision, hipStream_t st) {
  const Prepared* P = nullptr;
  LMX_TRY(lane_of(m, "lmx_sam_lane_encode", lane, h, w, precision, &P));
  LMX_REQUIRE(frames != nullptr && n > 0 && n <= m->max_batch, "lmx_sam_lane_encode: %d frames at %p for a lane of %d", n, (const void*)frames, m->max_batch);
  SamRun R("lmx_sam_lane_encode", *P, st);
  return encode_chunk(R, m, *P, precision, frames, n, h, w, P->emb);
}

int lmx_sam_lane_decode(lmx_sam* m, int lane, int n, int h, int w, const float* boxes, int64_t ldb, int precision, uint8_t* mask_bits, int64_t* stats,
                        int64_t* contour, float* iou, hipStream_t st) {
  const Prepared* P = nullptr;
  LMX_TRY(lane_of(m, "lmx_sam_lane_decode", lane, h, w, precision, &P));
  LMX_REQUIRE(n > 0 && n <= m->max_batch, "lmx_sam_lane_decode: %d frames for a lane of %d", n, m->max_batch);
  LMX_REQUIRE(boxes && ldb >= 4 && stats && iou, "lmx_sam_lane_decode: null pointer, or a box row stride of %lld floats", (long long)ldb);
  LMX_REQUIRE(!contour || P->contour_ws, "lmx_sam_lane_decode: contour features are served for frames of 2 x 2 up to 2^21 - 1 pixels, not %d x %d", h, w);
  SamRun R("lmx_sam_lane_decode", *P, st);
  return decode_chunk(R, m, *P, precision, P->emb, n, h, w, boxes, ldb, nullptr, mask_bits, stats, contour, iou, nullptr);
}

extern "C" int lmx_sam_open_host(const char* path_host, int max_batch, lmx_sam** out_host) {
  return lmx_handle_open("lmx_sam_open_host", path_host, max_batch, out_host, open_into, destroy);
}

extern "C" void lmx_sam_close(lmx_sam* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_sam_info(const lmx_sam* m, lmx_sam_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_sam_info: null argument");
  lmx_sam_fill_info(m->cfg, m->max_batch, info_host);
  return LMX_OK;
}

extern "C" int lmx_sam_resized(const lmx_sam* m, int h, int w, int* nh_host, int* nw_host) {
  LMX_REQUIRE(m && nh_host && nw_host, "lmx_sam_resized: null argument");
  LMX_REQUIRE(h > 0 && w > 0, "lmx_sam_resized: frame size %d x %d", h, w);
  lmx_sam_resized_hw(m->cfg.image, h, w, nh_host, nw_host);
  return LMX_OK;
}

extern "C" int lmx_sam_prepare(lmx_sam* m, int h, int w, int precision) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_sam_prepare"));
  LMX_REQUIRE(h > 0 && w > 0, "lmx_sam_prepare: frame size %d x %d", h, w);
  return prepare(m, h, w, precision, nullptr);
}

extern "C" int lmx_sam_encode(lmx_sam* m, const uint8_t* frames, int n, int h, int w, int precision, void* emb, lmx_stream_t stream) {
  LMX_TRY(check_call(m, "lmx_sam_encode", n, h, w, precision));
  LMX_REQUIRE(frames != nullptr, "lmx_sam_encode: null pointer (frames)");
  LMX_REQUIRE(emb != nullptr, "lmx_sam_encode: null pointer (emb)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_sam_encode", st));  // before prepare: a refused call allocates nothing
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));  // a pair seen before: a lookup
  const size_t frame_bytes = (size_t)h * w * 3, g = (size_t)m->cfg.grid();
  const size_t emb_bytes = g * g * m->cfg.out_ch * (size_t)emb_elt(m, precision);
  SamRun R("lmx_sam_encode", *P, st);
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    LMX_TRY(encode_chunk(R, m, *P, precision, frames + (size_t)done * frame_bytes, nb, h, w, static_cast<char*>(emb) + (size_t)done * emb_bytes));
  }
  return LMX_OK;
}

// the chunk loop of lmx_sam_decode (frames == nullptr: emb_or_null holds the embeddings) and lmx_sam_segment (encode into the workspace first)
static int run(lmx_sam* m, const char* fn, const Prepared& P, const uint8_t* frames, const void* emb, int n, int h, int w, const float* boxes, int precision,
               uint8_t* mask, uint8_t* mask_bits, int64_t* stats, int64_t* contour, float* iou, float* lowres, hipStream_t st) {
  const size_t frame_bytes = (size_t)h * w * 3, g = (size_t)m->cfg.grid(), px = (size_t)h * w, wb = (size_t)(w + 7) / 8, LL = 16 * g * g;
  const size_t emb_bytes = g * g * m->cfg.out_ch * (size_t)emb_elt(m, precision);
  SamRun R(fn, P, st);
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    const size_t d = (size_t)done;
    const void* e = emb ? static_cast<const char*>(emb) + d * emb_bytes : P.emb;
    if (frames) LMX_TRY(encode_chunk(R, m, P, precision, frames + d * frame_bytes, nb, h, w, P.emb));
    LMX_TRY(decode_chunk(R, m, P, precision, e, nb, h, w, boxes + d * 4, 4, mask ? mask + d * px : nullptr, mask_bits ? mask_bits + d * h * wb : nullptr,
                         stats + d * 8, contour ? contour + d * 8 : nullptr, iou + d, lowres ? lowres + d * LL : nullptr));
  }
  return LMX_OK;
}

extern "C" int lmx_sam_decode(lmx_sam* m, const void* emb, int n, int h, int w, const float* boxes, int precision, uint8_t* mask, uint8_t* mask_bits,
                              int64_t* stats, int64_t* contour, float* iou, float* lowres, lmx_stream_t stream) {
  LMX_TRY(check_decode(m, "lmx_sam_decode", emb, "emb", n, h, w, boxes, precision, stats, contour, iou));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_sam_decode", st));
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));
  return run(m, "lmx_sam_decode", *P, nullptr, emb, n, h, w, boxes, precision, mask, mask_bits, stats, contour, iou, lowres, st);
}

extern "C" int lmx_sam_segment(lmx_sam* m, const uint8_t* frames, int n, int h, int w, const float* boxes, int precision, uint8_t* mask,
                               uint8_t* mask_bits, int64_t* stats, int64_t* contour, float* iou, float* lowres, lmx_stream_t stream) {
  LMX_TRY(check_decode(m, "lmx_sam_segment", frames, "frames", n, h, w, boxes, precision, stats, contour, iou));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_sam_segment", st));  // before prepare: a refused call allocates nothing
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));
  return run(m, "lmx_sam_segment", *P, frames, nullptr, n, h, w, boxes, precision, mask, mask_bits, stats, contour, iou, lowres, st);
}

extern "C" int lmx_sam_segment_host(lmx_sam* m, const uint8_t* frames_host, int n, int h, int w, const float* boxes_host, int precision,
                                    uint8_t* mask_host, uint8_t* mask_bits_host, int64_t* stats_host, int64_t* contour_host, float* iou_host,
                                    float* lowres_host) {
  LMX_TRY(check_decode(m, "lmx_sam_segment_host", frames_host, "frames", n, h, w, boxes_host, precision, stats_host, contour_host, iou_host));
  const Prepared* P = nullptr;
  LMX_TRY(prepare(m, h, w, precision, &P));
  // staging of one chunk: frames | boxes | mask | mask_bits | stats | contour | iou | lowres, each on a 256-byte boundary
  const size_t B = (size_t)(n < m->max_batch ? n : m->max_batch), frame_bytes = (size_t)h * w * 3, px = (size_t)h * w, wb = (size_t)(w + 7) / 8;
  const size_t g = (size_t)m->cfg.grid(), LL = 16 * g * g;
  LmxLayout lay;
  lay.add(B * frame_bytes);  // the frames, at the blob's start
  const size_t o_boxes = lay.add(B * 16), o_mask = lay.add(mask_host ? B * px : 0), o_bits = lay.add(mask_bits_host ? B * h * wb : 0),
               o_stats = lay.add(B * 64), o_contour = lay.add(contour_host ? B * 64 : 0), o_iou = lay.add(B * 4),
               o_lowres = lay.add(lowres_host ? B * LL * 4 : 0);
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  char* s = m->stage;
  float* boxes = reinterpret_cast<float*>(s + o_boxes);
  uint8_t *mask = mask_host ? reinterpret_cast<uint8_t*>(s + o_mask) : nullptr, *bits = mask_bits_host ? reinterpret_cast<uint8_t*>(s + o_bits) : nullptr;
  int64_t *stats = reinterpret_cast<int64_t*>(s + o_stats), *contour = contour_host ? reinterpret_cast<int64_t*>(s + o_contour) : nullptr;
  float *iou = reinterpret_cast<float*>(s + o_iou), *lowres = lowres_host ? reinterpret_cast<float*>(s + o_lowres) : nullptr;
  for (int done = 0; done < n; done += m->max_batch) {
    const size_t nb = (size_t)(n - done < m->max_batch ? n - done : m->max_batch), d = (size_t)done;
    LMX_HIP(hipMemcpyAsync(s, frames_host + d * frame_bytes, nb * frame_bytes, hipMemcpyHostToDevice, m->own));
    LMX_HIP(hipMemcpyAsync(boxes, boxes_host + d * 4, nb * 16, hipMemcpyHostToDevice, m->own));
    LMX_TRY(run(m, "lmx_sam_segment_host", *P, reinterpret_cast<const uint8_t*>(s), nullptr, (int)nb, h, w, boxes, precision, mask, bits, stats, contour, iou, lowres, m->own));
    if (mask) LMX_HIP(hipMemcpyAsync(mask_host + d * px, mask, nb * px, hipMemcpyDeviceToHost, m->own));
    if (bits) LMX_HIP(hipMemcpyAsync(mask_bits_host + d * h * wb, bits, nb * h * wb, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(stats_host + d * 8, stats, nb * 64, hipMemcpyDeviceToHost, m->own));
    if (contour) LMX_HIP(hipMemcpyAsync(contour_host + d * 8, contour, nb * 64, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipMemcpyAsync(iou_host + d, iou, nb * 4, hipMemcpyDeviceToHost, m->own));
    if (lowres) LMX_HIP(hipMemcpyAsync(lowres_host + d * LL, lowres, nb * LL * 4, hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipStreamSynchronize(m->own));
  }
  return LMX_OK;
}
