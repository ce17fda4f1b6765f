// sam_hiera_model.h — the Hiera encoder's launch plan for the SAM handle (included by sam_model.hip, which owns the handle, the resize,
// the decoder and the entry points).  It is the launch sequence of lmx/sam.py's HieraEncoder(band="blocks").encode(frames,
// outputs="embedding")["fpn"][2]: preprocess' im2col, trunk() record by record over the plan lmx_h_hiera_plan computes for the chunk
// (host_hiera_plan.cpp), _attention_half's forms, and fpn(lowest=2).  HOST code only: every launch goes through the extern "C"
// lmx_k_* entry point the ctypes binding calls, with the descriptor lmx/kernels.py fills, in Python's order.
// Memory follows Python's tensors: what a chain updates in place there is updated in place here; where Python allocates a fresh
// tensor this takes a distinct buffer — from the `stream` arena where it outlives its block (the residual stream's new tensors, the
// next block's layer_norm1 rows, the f16 copies, the neck), from the `scratch` arena, rewound at every block, where it does not.
// The trunk is written once over HieraRun, a run of plan_run.h: a counting run (prepare) sizes the two arenas, each buffer refused by
// name from 2 GB on, and a launching run walks the same code over the same offsets.
#pragma once
#include <math.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "model_handle.h"
#include "sam_image.h"

namespace {

const int HIERA_KPAD_COLS = 152;  // the patch matrix' columns: 7 * 7 * 3 padded to a multiple of 8

struct HieraBlockW {
  LmxHieraBlock shape;
  int fused = 0;
  const float *g1, *b1, *bqkv, *bo, *g2, *b2, *bb1, *bb2, *bp;
  const half_t *wqkv, *padkv, *wo, *w1, *w2, *wp;
  const void* attn[4];
  const void* mlp_img[2];
};

struct HieraW {
  lmx_hiera_config_t cfg;
  int n_blocks = 0, first_global = -1;
  const void* pe_w = nullptr;
  const float *pe_b = nullptr, *pos = nullptr;
  std::vector<HieraBlockW> blocks;
  const void* neck_w[LMX_HIERA_MAX_STAGES];
  const float* neck_b[LMX_HIERA_MAX_STAGES];
};

// the rows below the band of the f32 stream entering each block with a join in front, for one frame geometry: what
// HieraEncoder._band_table keeps in tab["x"].  One allocation; x[i] is null where block i has no join.
struct HieraBandTable {
  char* blob = nullptr;
  std::vector<int> rows;         // the rows per block the table was built for
  std::vector<const float*> x;   // per block: rows [join, H) of the stream entering it, [(H - join) * W][dim]
};

// one pass over the trunk: counting (launch false: no kernel runs, no pointer is followed) or launching
struct HieraRun : LmxPlanRun {
  LmxArena stream, scratch;
  HieraRun() { model = "the Hiera encoder"; }
  template <class T>
  int keep(const char* what, int64_t bytes, T** out) {  // outlives its block
    return take(&stream, what, bytes, out);
  }
  template <class T>
  int tmp(const char* what, int64_t bytes, T** out) {  // dies with its block
    return take(&scratch, what, bytes, out);
  }
};

#define HR_LAUNCH(call) LMX_LAUNCH(R, call)

// K.gemm: out [M or M / 4][N] = act(a [M][K] w^T + bias) (+ res), with the pooled-row mode (pool_h > 0: the rows of a are an
// [n, pool_h, pool_w] grid, the result its 2 x 2 max-pool) and the ln_out rows of the projection
inline int hiera_gemm(const void* a, int K, const void* w, const float* bias, void* out, int out_dtype, int M, int N, int act, const void* res, int res_rows,
                      int pool_h, int pool_w, void* ln_out, const float* ln_g, const float* ln_b, float ln_eps, hipStream_t st) {
  return lmx_gemm_dense_rep(a, K, w, bias, out, N, out_dtype, M, N, K, act, nullptr, res, N, res_rows, 1, st, pool_h, pool_w, ln_out, ln_g, ln_b, ln_eps);
}

// HieraEncoder._attention_half: [shortcut GEMM ->] qkv GEMM -> [Q-pool] -> attention -> proj GEMM + residual as separate launches, in
// the forms P names.  *x: the stream, replaced where the block has a shortcut; *h2: layer_norm2's rows where the projection wrote them
inline int hiera_attention_half(HieraRun& R, const lmx_hiera_block_t& P, const HieraBlockW& B, const half_t* h, float** x, half_t** h2, int n, float eps) {
  const int Din = B.shape.dim, D = B.shape.D, heads = B.shape.heads, win = P.window, qs = B.shape.qs, hd = D / heads;
  const int H = P.H, W = P.W, Hq = P.Ho, Wq = P.Wo;
  const int64_t rows_in = (int64_t)n * H * W, rows_out = (int64_t)n * Hq * Wq;
  const float scale = (float)pow((double)hd, -0.5);
  hipStream_t st = lmx_run_stream(R);
  const float* res = *x;
  const bool fresh = P.shortcut != LMX_HIERA_SHORTCUT_NONE;  // the residual is a tensor of its own: so is the block's output
  if (P.shortcut == LMX_HIERA_SHORTCUT_POOLED_GEMM) {  // the shortcut's projection and its 2 x 2 max-pool in one launch
    float* r;
    LMX_TRY(R.tmp("pooled shortcut", rows_out * D * 4, &r));
    HR_LAUNCH(hiera_gemm(h, Din, B.wp, B.bp, r, LMX_F32, (int)rows_in, D, LMX_ACT_NONE, nullptr, 0, H, W, nullptr, nullptr, nullptr, 0.f, st));
    res = r;
  } else if (P.shortcut != LMX_HIERA_SHORTCUT_NONE) {
    float* r;
    LMX_TRY(R.tmp("shortcut", rows_in * D * 4, &r));
    HR_LAUNCH(hiera_gemm(h, Din, B.wp, B.bp, r, LMX_F32, (int)rows_in, D, LMX_ACT_NONE, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
    res = r;
    if (P.shortcut == LMX_HIERA_SHORTCUT_GEMM_MAXPOOL) {
      float* pooled;
      LMX_TRY(R.tmp("pooled shortcut", rows_out * D * 4, &pooled));
      HR_LAUNCH(lmx_k_maxpool2(r, D, pooled, D, LMX_F32, n, H, W, D, st));
      res = pooled;
    }
  }
  const half_t *q, *k, *v;
  int64_t ldq, ldkv;
  if (P.query == LMX_HIERA_QUERY_POOLED_Q_KV) {
    // pooled queries: the q third of the projection writes its 2 x 2 max-pool directly, k and v come from a second launch on the same rows
    half_t *qp, *kv;
    LMX_TRY(R.tmp("pooled q", rows_out * D * 2, &qp));
    HR_LAUNCH(hiera_gemm(h, Din, B.wqkv, B.bqkv, qp, LMX_F16, (int)rows_in, D, LMX_ACT_NONE, nullptr, 0, H, W, nullptr, nullptr, nullptr, 0.f, st));
    LMX_TRY(R.tmp("kv", rows_in * 2 * D * 2, &kv));
    HR_LAUNCH(hiera_gemm(h, Din, B.wqkv + (int64_t)D * Din, B.bqkv + D, kv, LMX_F16, (int)rows_in, 2 * D, LMX_ACT_NONE, nullptr, 0, 0, 0, nullptr, nullptr,
                         nullptr, 0.f, st));
    q = qp, k = kv, v = kv ? kv + D : nullptr, ldq = D, ldkv = 2 * D;
  } else {
    half_t* qkv;
    LMX_TRY(R.tmp("qkv", rows_in * 3 * D * 2, &qkv));
    HR_LAUNCH(hiera_gemm(h, Din, B.wqkv, B.bqkv, qkv, LMX_F16, (int)rows_in, 3 * D, LMX_ACT_NONE, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
    q = qkv, k = qkv ? qkv + D : nullptr, v = qkv ? qkv + 2 * D : nullptr, ldq = ldkv = 3 * D;
    if (P.query == LMX_HIERA_QUERY_QKV_MAXPOOL) {
      half_t* qp;
      LMX_TRY(R.tmp("pooled q", rows_out * D * 2, &qp));
      HR_LAUNCH(lmx_k_maxpool2(qkv, 3 * D, qp, D, LMX_F16, n, H, W, D, st));
      q = qp, ldq = D;
    }
  }
  half_t* a;
  LMX_TRY(R.tmp("attention output", rows_out * D * 2, &a));
  if (R.launch) {
    const lmx_attn_desc ad = win > 0 ? lmx_attn_windowed(q, ldq, k, v, ldkv, a, D, n, heads, hd, scale, H, W, win, qs != 0, B.padkv + D, B.padkv + 2 * D)
                                     : lmx_attn_flat(q, ldq, k, v, ldkv, a, D, n, heads, Hq * Wq, H * W, hd, scale);
    LMX_TRY(lmx_k_attention(&ad, st));
  }
  float* xo = *x;
  if (fresh) LMX_TRY(R.keep("residual stream", rows_out * D * 4, &xo));
  *h2 = nullptr;
  if (P.ln_out) LMX_TRY(R.tmp("layer_norm2 rows", rows_out * D * 2, h2));
  HR_LAUNCH(hiera_gemm(a, D, B.wo, B.bo, xo, LMX_F32, (int)rows_out, D, LMX_ACT_NONE, res, 0, 0, 0, *h2, B.g2, B.b2, eps, st));
  *x = xo;
  return LMX_OK;
}

// HieraEncoder.trunk() + fpn(lowest = 2) for n frames whose patches hold the top plan[0].H token rows: the embedding, f16
// [n][64][64][fpn_dim], goes to `emb`.  stop_at >= 0 (the table pass: one frame, the whole grid): taps[i] (device, caller-sized)
// receives rows [tap_have[i], tap_need[i]) of the stream entering block i where tap_need[i] > 0, and the trunk stops in front of
// block stop_at.
inline int hiera_trunk(HieraRun& R, const HieraW& Wt, const lmx_hiera_block_t* plan, const void* patches, int n, const HieraBandTable* table, void* emb,
                       int stop_at, const int* tap_have, const int* tap_need, float* const* taps) {
  const lmx_hiera_config_t& c = Wt.cfg;
  const int g = c.image / 4, nb = Wt.n_blocks;
  const float eps = (float)c.eps;
  hipStream_t st = lmx_run_stream(R);
  const int H0 = plan[0].join ? plan[0].join : plan[0].H;
  float* x;
  LMX_TRY(R.keep("residual stream", (int64_t)n * H0 * g * c.hidden * 4, &x));
  HR_LAUNCH(hiera_gemm(patches, HIERA_KPAD_COLS, Wt.pe_w, Wt.pe_b, x, LMX_F32, n * H0 * g, c.hidden, LMX_ACT_NONE, Wt.pos, H0 * g, 0, 0, nullptr, nullptr,
                       nullptr, 0.f, st));
  const float* stage_x[LMX_HIERA_MAX_STAGES] = {nullptr};
  const half_t* stage_x16[LMX_HIERA_MAX_STAGES] = {nullptr};
  int stage_h[LMX_HIERA_MAX_STAGES] = {0}, stage_w[LMX_HIERA_MAX_STAGES] = {0}, stage = 0;
  half_t* h_next = nullptr;
  for (int i = 0; i < nb; ++i) {
    const lmx_hiera_block_t& P = plan[i];
    const HieraBlockW& B = Wt.blocks[(size_t)i];
    const int Din = B.shape.dim, D = B.shape.D, heads = B.shape.heads;
    R.rewind_to(&R.scratch, 0);  // what the last block took from the scratch arena is dead
    if (stop_at >= 0) {
      if (tap_need[i] > 0 && R.launch)
        LMX_HIP(hipMemcpyAsync(taps[i], x + (int64_t)tap_have[i] * P.W * Din, (size_t)(tap_need[i] - tap_have[i]) * P.W * Din * 4, hipMemcpyDeviceToDevice, st));
      if (i == stop_at) return LMX_OK;
    }
    const int64_t rows_in = (int64_t)n * P.H * P.W, rows_out = (int64_t)n * P.Ho * P.Wo;
    if (P.join) {
      LMX_REQUIRE(!R.launch || (table && table->x[(size_t)i]), "%s: the band table holds no rows for the join in front of block %d", R.fn, i);
      float* joined;
      LMX_TRY(R.keep("joined stream", rows_in * Din * 4, &joined));
      HR_LAUNCH(lmx_k_band_join(x, table->x[(size_t)i], joined, LMX_F32, n, P.H, P.join, P.W, Din, st));
      x = joined;
    }
    const half_t* h = nullptr;
    if (P.ln1 == LMX_HIERA_LN1_PREV) {
      LMX_REQUIRE(h_next || !R.launch, "%s: block %d takes layer_norm1's rows from a block that wrote none", R.fn, i);
      h = h_next;
    } else if (P.ln1 == LMX_HIERA_LN1_LAUNCH) {
      half_t* hl;
      LMX_TRY(R.tmp("layer_norm1 rows", rows_in * Din * 2, &hl));
      HR_LAUNCH(lmx_k_layernorm(x, LMX_F32, Din, B.g1, B.b1, hl, LMX_F16, Din, (int)rows_in, Din, eps, LMX_ACT_NONE, st));
      h = hl;
    }
    const float scale = (float)pow((double)(D / heads), -0.5);
    half_t* h2 = nullptr;
    // the attention half in one launch (csrc/hiera.hip) ...
    if (P.attn == LMX_HIERA_ATTN8_LN) {
      HR_LAUNCH(lmx_k_hiera_attn8(nullptr, x, D, B.g1, B.b1, eps, B.attn[0], static_cast<const float*>(B.attn[1]), B.attn[2], static_cast<const float*>(B.attn[3]),
                                  n, P.H, P.W, D, heads, scale, st));
    } else if (P.attn == LMX_HIERA_ATTN8) {
      HR_LAUNCH(lmx_k_hiera_attn8(h, x, D, nullptr, nullptr, 0.f, B.attn[0], static_cast<const float*>(B.attn[1]), B.attn[2], static_cast<const float*>(B.attn[3]),
                                  n, P.H, P.W, D, heads, scale, st));
    } else if (P.attn == LMX_HIERA_ATTN_POOL) {  // the stage-opening block: pooled q + shortcut
      float* out;
      LMX_TRY(R.keep("residual stream", rows_out * D * 4, &out));
      HR_LAUNCH(lmx_k_hiera_attn_pool(h, out, B.attn[0], static_cast<const float*>(B.attn[1]), n, P.H, P.W, Din, D, heads, scale, st));
      x = out;
    } else if (P.attn == LMX_HIERA_ATTN4) {
      HR_LAUNCH(lmx_k_hiera_attn4(h, x, D, B.attn[0], static_cast<const float*>(B.attn[1]), n, P.H, P.W, D, heads, scale, st));
    } else {  // ... or as separate launches
      LMX_TRY(hiera_attention_half(R, P, B, h, &x, &h2, n, eps));
    }
    // the FPN's lateral convolution reads a stage output as f16: written by the MLP kernel, not cast later
    half_t *x16 = nullptr, *hn = nullptr;
    if (P.x16) LMX_TRY(R.keep("f16 stage output", rows_out * D * 2, &x16));
    if (P.emit_ln1) LMX_TRY(R.keep("next block's layer_norm1 rows", rows_out * D * 2, &hn));
    h_next = hn;
    if (P.mlp == LMX_HIERA_MLP_IMG) {
      HR_LAUNCH(lmx_k_ln_mlp_img(x, D, B.mlp_img[0], static_cast<const float*>(B.mlp_img[1]), rows_out, D, eps, x16, hn, st));
    } else {
      LMX_REQUIRE(P.mlp == LMX_HIERA_MLP_LAUNCHES, "%s: block %d: MLP form %d is not the default plan's", R.fn, i, P.mlp);
      if (!h2) {  // (else: written by the attention projection, ln_out)
        LMX_TRY(R.tmp("layer_norm2 rows", rows_out * D * 2, &h2));
        HR_LAUNCH(lmx_k_layernorm(x, LMX_F32, D, B.g2, B.b2, h2, LMX_F16, D, (int)rows_out, D, eps, LMX_ACT_NONE, st));
      }
      half_t* u;
      LMX_TRY(R.tmp("MLP hidden", rows_out * 4 * D * 2, &u));
      HR_LAUNCH(hiera_gemm(h2, D, B.w1, B.bb1, u, LMX_F16, (int)rows_out, 4 * D, LMX_ACT_GELU, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
      HR_LAUNCH(hiera_gemm(u, 4 * D, B.w2, B.bb2, x, LMX_F32, (int)rows_out, D, LMX_ACT_NONE, x, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
    }
    if (!P.stage_end) continue;
    if (P.keep) {
      // (a kept stage output inside the band would be joined with the table's rows: lmx_sam_prepare refuses such a plan)
      LMX_REQUIRE(!P.join_out, "%s: block %d ends a kept stage inside the band", R.fn, i);
      stage_x[stage] = x, stage_x16[stage] = x16, stage_h[stage] = P.Ho, stage_w[stage] = P.Wo;
      if (P.clone) {  // the stream goes on in a copy: a same-width next block would update the kept output in place
        float* copy;
        LMX_TRY(R.keep("residual stream", rows_out * D * 4, &copy));
        if (R.launch) LMX_HIP(hipMemcpyAsync(copy, x, (size_t)rows_out * D * 4, hipMemcpyDeviceToDevice, st));
        x = copy;
      }
    }
    ++stage;
  }
  if (stop_at >= 0) return LMX_OK;
  // HieraEncoder.fpn(stages, stages16, lowest = 2): the lateral convolutions from the last level down to the embedding's
  const int nlev = c.n_stages - 1, C = c.fpn_dim;
  const half_t* prev = nullptr;
  int prev_h = 0, prev_w = 0;
  for (int s = nlev; s >= 2; --s) {
    LMX_REQUIRE(stage_x[s] || !R.launch, "%s: stage %d was not kept", R.fn, s);
    const int64_t rows = (int64_t)n * stage_h[s] * stage_w[s];
    const half_t* a = stage_x16[s];
    if (!a) {
      half_t* cast;
      LMX_TRY(R.keep("f16 stage output", rows * c.dims[s] * 2, &cast));
      HR_LAUNCH(lmx_k_cast_f32_f16(stage_x[s], c.dims[s], cast, c.dims[s], rows, c.dims[s], st));
      a = cast;
    }
    half_t* out = static_cast<half_t*>(emb);
    if (s != 2) LMX_TRY(R.keep("FPN level", rows * C * 2, &out));
    bool top_down = false;
    for (int k = 0; k < c.n_top_down; ++k) top_down |= c.fpn_top_down[k] == s;
    if (!top_down || s == nlev) {
      HR_LAUNCH(hiera_gemm(a, c.dims[s], Wt.neck_w[s], Wt.neck_b[s], out, LMX_F16, (int)rows, C, LMX_ACT_NONE, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
    } else {
      LMX_REQUIRE(stage_h[s] == 2 * prev_h && stage_w[s] == 2 * prev_w, "%s: FPN level %d is %d x %d, the level above %d x %d", R.fn, s, stage_h[s], stage_w[s],
                  prev_h, prev_w);
      half_t* up;
      LMX_TRY(R.keep("upsampled FPN level", rows * C * 2, &up));
      HR_LAUNCH(lmx_k_upsample2(prev, C, up, C, n, prev_h, prev_w, C, st));
      HR_LAUNCH(hiera_gemm(a, c.dims[s], Wt.neck_w[s], Wt.neck_b[s], out, LMX_F16, (int)rows, C, LMX_ACT_NONE, up, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, st));
    }
    prev = out, prev_h = stage_h[s], prev_w = stage_w[s];
  }
  return LMX_OK;
}

}  // namespace
