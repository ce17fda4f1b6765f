// dino_model.hip — the model-level entry points of the C-ABI for DINO: a handle (model_handle.h has what every handle owns) with the
// weights of one weight image (dino_image.h) and the workspace of one batch, and lmx_dino_embed, the launch sequence of lmx/dino.py's DinoEmbedder
// (preprocess + hidden_states + token_mean; services/dinov3-pipeline/app/main.py:98-113) written as host C++.
// HOST code only: there is no kernel in this file.  Every launch goes through the same extern "C" lmx_k_* entry point the ctypes
// binding calls, with the descriptor filled as lmx/kernels.py fills it, so the embedding is the Python plan's bit for bit
// (tests/test_gpu_native_dino.py).
// The transformer's buffers come from a run of plan_run.h: lmx_dino_open_host walks embed_chunk counting at max_batch (they do not
// depend on the frame size), every call walks it launching.  The run refuses a buffer of 2 GB or more by name.  That also keeps every
// element index the kernels form below 2^31: the widest rows are qkv's 3 hidden and the MLP GEMM's 2 mlp columns (gated), and a row
// index times either stays below the BYTES of the f16 qkv and MLP buffers, which the run bounds: no separate check on elements.
#include <math.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "dino_image.h"
#include "model_handle.h"

namespace {

// what lmx_dino_prepare builds for one frame size: the resize tables and the resized-frame workspace, one device allocation
struct FrameSize {
  int nh = 0, nw = 0;
  char* blob = nullptr;
  // pil: tab_h always (identity if the width is kept), tab_v only if the height changes; float: both, already cut to the crop
  int32_t *bounds_h = nullptr, *bounds_v = nullptr;
  void *kk_h = nullptr, *kk_v = nullptr;  // i32 (pil) / f32 (float)
  int ksize_h = 0, ksize_v = 0, seg_cols = 0;
  uint8_t *tmp_h = nullptr, *tmp_v = nullptr;  // pil: [max_batch, h, nw, 3] after the horizontal pass, [max_batch, nh, nw, 3] after the vertical
};

struct Layer {
  const float *g1, *b1, *bqkv, *bo, *ls1, *g2, *b2, *bb1, *bb2, *ls2;
  const void *wqkv, *wo, *w1, *w2;
};

}  // namespace

struct lmx_dino : LmxHandleCore {
  LmxDinoCfg cfg;
  char* work = nullptr;  // the workspace of max_batch frames: the patch matrix, then the arena of embed_chunk's buffers
  LmxArena arena;        // ... as open counted it (base and cap); a call walks a copy
  // weights
  const void* pe_w = nullptr;
  const float *pe_b = nullptr, *prefix = nullptr, *pos = nullptr, *rope_cos = nullptr, *rope_sin = nullptr, *gf = nullptr, *bf = nullptr,
              *lut = nullptr;
  std::vector<Layer> layers;
  void* patches = nullptr;  // the patch matrix [max_batch, grid^2, k_pad], a field: its padding columns are zeroed once, at open
  float mean_std[6];
  std::map<std::pair<int, int>, FrameSize> sizes;
};

namespace {

void destroy(lmx_dino* m) {
  for (auto& kv : m->sizes) (void)hipFree(kv.second.blob);
  (void)hipFree(m->work);
  lmx_handle_free(m);
  delete m;
}

// one axis of the float recipe: ATen's table, cut to the rows the centre crop keeps (TorchvisionBackend.center_crop: int((size - crop) / 2))
int aa_axis(int in_size, int out_size, int filt, int S, std::vector<int32_t>* bounds, std::vector<float>* kk, int* ksize) {
  LMX_TRY(lmx_h_aa_tables(in_size, out_size, filt, nullptr, nullptr, 0, ksize));
  std::vector<int32_t> b((size_t)out_size * 2);
  std::vector<float> k((size_t)out_size * *ksize);
  LMX_TRY(lmx_h_aa_tables(in_size, out_size, filt, b.data(), k.data(), (int64_t)k.size(), ksize));
  const int o = (int)((out_size - S) / 2.0);
  bounds->assign(b.begin() + 2 * (size_t)o, b.begin() + 2 * (size_t)(o + S));
  kk->assign(k.begin() + (size_t)o * *ksize, k.begin() + (size_t)(o + S) * *ksize);
  return LMX_OK;
}

int prepare(lmx_dino* m, int h, int w, const FrameSize** out) {
  const LmxDinoCfg& c = m->cfg;
  const auto it = m->sizes.find({h, w});
  if (it != m->sizes.end()) {
    if (out) *out = &it->second;
    return LMX_OK;
  }
  FrameSize fs;
  LMX_TRY(lmx_dino_resized(c, h, w, &fs.nh, &fs.nw));
  LMX_REQUIRE((int)m->sizes.size() < LMX_MAX_PREPARED, "lmx_dino_prepare: the handle already holds %d frame sizes; open another for more", LMX_MAX_PREPARED);
  const int nh = fs.nh, nw = fs.nw;
  std::vector<int32_t> bh, bv;
  std::vector<char> kh, kv;  // i32 or f32 bytes
  size_t tmp_h = 0, tmp_v = 0;
  if (c.recipe_kind == LMX_RECIPE_PIL) {
    // the horizontal pass always runs: it also does the BGR->RGB swap (identity table if the width is kept)
    bh.resize((size_t)nw * 2);
    if (nw != w) {
      LMX_TRY(lmx_h_pil_tables(w, nw, c.filt, nullptr, nullptr, 0, &fs.ksize_h));
      kh.resize((size_t)nw * fs.ksize_h * 4);
      LMX_TRY(lmx_h_pil_tables(w, nw, c.filt, bh.data(), reinterpret_cast<int32_t*>(kh.data()), (int64_t)nw * fs.ksize_h, &fs.ksize_h));
    } else {
      fs.ksize_h = 1;
      kh.resize((size_t)nw * 4);
      LMX_TRY(lmx_h_identity_table(nw, bh.data(), reinterpret_cast<int32_t*>(kh.data())));
    }
    tmp_h = (size_t)m->max_batch * h * nw * 3;
    if (nh != h) {
      LMX_TRY(lmx_h_pil_tables(h, nh, c.filt, nullptr, nullptr, 0, &fs.ksize_v));
      bv.resize((size_t)nh * 2);
      kv.resize((size_t)nh * fs.ksize_v * 4);
      LMX_TRY(lmx_h_pil_tables(h, nh, c.filt, bv.data(), reinterpret_cast<int32_t*>(kv.data()), (int64_t)nh * fs.ksize_v, &fs.ksize_v));
      tmp_v = (size_t)m->max_batch * nh * nw * 3;
    }
  } else {
    std::vector<float> fh, fv;
    LMX_TRY(aa_axis(w, nw, c.filt, c.image, &bh, &fh, &fs.ksize_h));
    LMX_TRY(aa_axis(h, nh, c.filt, c.image, &bv, &fv, &fs.ksize_v));
    kh.assign(reinterpret_cast<char*>(fh.data()), reinterpret_cast<char*>(fh.data() + fh.size()));
    kv.assign(reinterpret_cast<char*>(fv.data()), reinterpret_cast<char*>(fv.data() + fv.size()));
    fs.seg_cols = lmx_h_segment_cols(bh.data(), c.image, 256);
    LMX_REQUIRE(fs.seg_cols > 0, "lmx_dino_prepare: empty horizontal table for %d -> %d", w, nw);
  }
  LmxLayout lay;
  const LmxUpload up[4] = {{lay.add(bh.size() * 4), bh.data(), bh.size() * 4},
                           {lay.add(kh.size()), kh.data(), kh.size()},
                           {lay.add(bv.size() * 4), bv.data(), bv.size() * 4},
                           {lay.add(kv.size()), kv.data(), kv.size()}};
  const size_t o_tmp_h = lay.add(tmp_h), o_tmp_v = lay.add(tmp_v);
  LMX_TRY(lmx_alloc_and_upload(lay.total, up, 4, &fs.blob));
  fs.bounds_h = reinterpret_cast<int32_t*>(fs.blob + up[0].at);
  fs.kk_h = fs.blob + up[1].at;
  fs.bounds_v = up[2].bytes ? reinterpret_cast<int32_t*>(fs.blob + up[2].at) : nullptr;
  fs.kk_v = up[3].bytes ? fs.blob + up[3].at : nullptr;
  fs.tmp_h = tmp_h ? reinterpret_cast<uint8_t*>(fs.blob + o_tmp_h) : nullptr;
  fs.tmp_v = tmp_v ? reinterpret_cast<uint8_t*>(fs.blob + o_tmp_v) : nullptr;
  const auto ins = m->sizes.emplace(std::make_pair(h, w), fs);
  if (out) *out = &ins.first->second;
  return LMX_OK;
}

// one walk of embed_chunk: counting at open (m null), or launching over a copy of the handle's arena
struct DinoRun : LmxPlanRun {
  LmxArena arena;
  DinoRun(const char* fn_, const lmx_dino* m, hipStream_t st_) {
    fn = fn_, model = "DINO", st = st_, launch = m != nullptr;
    if (m) arena = m->arena;
  }
};

// DinoEmbedder.preprocess + hidden_states + token_mean for n <= max_batch frames
int embed_chunk(DinoRun& R, const lmx_dino* m, const FrameSize& fs, const uint8_t* frames, int n, int h, int w, int rgb, float* emb) {
  const LmxDinoCfg& c = m->cfg;
  const int D = c.hidden, H = c.heads, hd = D / H, T = c.tokens, I = c.mlp, np = c.grid * c.grid, rows = n * T;
  hipStream_t st = lmx_run_stream(R);
  LmxArena* A = &R.arena;
  R.rewind_to(A, 0);
  if (c.recipe_kind == LMX_RECIPE_FLOAT) {
    LMX_LAUNCH(R, lmx_k_float_resize_patchify(frames, m->patches, n, h, w, c.grid, c.grid, c.patch, c.k_pad, fs.bounds_h,
                                              static_cast<const float*>(fs.kk_h), fs.ksize_h, fs.bounds_v, static_cast<const float*>(fs.kk_v), fs.ksize_v,
                                              fs.seg_cols, (float)c.rescale, m->mean_std, rgb ? 0 : 1, st));
  } else {
    LMX_LAUNCH(R, lmx_k_pil_resize_h(frames, fs.tmp_h, n, h, w, fs.nw, fs.bounds_h, static_cast<const int32_t*>(fs.kk_h), fs.ksize_h, rgb ? 0 : 1, st));
    const uint8_t* img = fs.tmp_h;
    if (fs.tmp_v) {
      LMX_LAUNCH(R, lmx_k_pil_resize_v(fs.tmp_h, fs.tmp_v, n, h, fs.nh, fs.nw, fs.bounds_v, static_cast<const int32_t*>(fs.kk_v), fs.ksize_v, st));
      img = fs.tmp_v;
    }
    LMX_LAUNCH(R, lmx_k_patchify_norm(img, m->patches, n, fs.nh, fs.nw, (fs.nh - c.image) / 2, (fs.nw - c.image) / 2, c.grid, c.grid, c.patch, c.k_pad,
                                      m->lut, st));
  }
  const int64_t e16 = 2, e32 = 4, prows = (int64_t)n * np, trows = rows;  // bytes per element; patch and token rows
  half_t *xp, *hn, *qkv, *a, *u;
  float *x, *y;
  LMX_TRY(R.take(A, "patch embedding", prows * D * e16, &xp));
  LMX_LAUNCH(R, lmx_gemm_dense(m->patches, c.k_pad, m->pe_w, m->pe_b, xp, D, LMX_F16, n * np, D, c.k_pad, LMX_ACT_NONE, nullptr, nullptr, 0, st));
  LMX_TRY(R.take(A, "residual stream", trows * D * e32, &x));
  LMX_LAUNCH(R, lmx_k_assemble_tokens(xp, m->prefix, m->pos, x, n, np, c.n_prefix, D, st));
  const float scale = (float)pow((double)hd, -0.5), eps = (float)c.eps;
  const int act1 = c.gated ? LMX_ACT_SWIGLU : LMX_ACT_GELU, N1 = c.gated ? 2 * I : I;
  // what every layer writes anew: LayerNorm rows, qkv, attention output, MLP intermediate
  LMX_TRY(R.take(A, "LayerNorm rows", trows * D * e16, &hn));
  LMX_TRY(R.take(A, "qkv", trows * 3 * D * e16, &qkv));
  LMX_TRY(R.take(A, "attention output", trows * D * e16, &a));
  LMX_TRY(R.take(A, "MLP intermediate", trows * I * e16, &u));
  for (const Layer& L : m->layers) {
    LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, L.g1, L.b1, hn, LMX_F16, D, rows, D, eps, LMX_ACT_NONE, st));
    LMX_LAUNCH(R, lmx_gemm_dense(hn, D, L.wqkv, L.bqkv, qkv, 3 * D, LMX_F16, rows, 3 * D, D, LMX_ACT_NONE, nullptr, nullptr, 0, st));
    if (m->rope_cos) {
      LMX_LAUNCH(R, lmx_k_rope(qkv, 3 * D, n, T, H, hd, c.n_prefix, m->rope_cos, m->rope_sin, st));
      LMX_LAUNCH(R, lmx_k_rope(qkv + D, 3 * D, n, T, H, hd, c.n_prefix, m->rope_cos, m->rope_sin, st));
    }
    if (R.launch) {
      const lmx_attn_desc ad = lmx_attn_flat(qkv, 3 * D, qkv + D, qkv + 2 * D, 3 * D, a, D, n, H, T, T, hd, scale);
      LMX_TRY(lmx_k_attention(&ad, st));
    }
    LMX_LAUNCH(R, lmx_gemm_dense(a, D, L.wo, L.bo, x, D, LMX_F32, rows, D, D, LMX_ACT_NONE, L.ls1, x, D, st));
    LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, L.g2, L.b2, hn, LMX_F16, D, rows, D, eps, LMX_ACT_NONE, st));
    LMX_LAUNCH(R, lmx_gemm_dense(hn, D, L.w1, L.bb1, u, I, LMX_F16, rows, N1, D, act1, nullptr, nullptr, 0, st));
    LMX_LAUNCH(R, lmx_gemm_dense(u, I, L.w2, L.bb2, x, D, LMX_F32, rows, D, I, LMX_ACT_NONE, L.ls2, x, D, st));
  }
  LMX_TRY(R.take(A, "final LayerNorm rows", trows * D * e32, &y));
  LMX_LAUNCH(R, lmx_k_layernorm(x, LMX_F32, D, m->gf, m->bf, y, LMX_F32, D, rows, D, eps, LMX_ACT_NONE, st));
  LMX_LAUNCH(R, lmx_k_token_mean(y, LMX_F32, emb, n, T, D, st));
  return LMX_OK;
}

int open_into(lmx_dino* m, const char* path) {
  const int max_batch = m->max_batch;
  LmxDinoImage img;
  LMX_TRY(lmx_dino_image_parse(path, &img));
  const LmxDinoCfg& c = img.cfg;
  m->cfg = c;
  for (int i = 0; i < 3; ++i) {
    m->mean_std[i] = (float)c.mean[i];
    m->mean_std[3 + i] = (float)c.std[i];
  }
  LMX_TRY(lmx_handle_upload_weights(m, "lmx_dino_open_host", path, img.data_offset, img.file_bytes));
  const uint64_t base = img.data_offset;
  auto at = [&](const LmxTensorRef& r) -> const void* { return r.nbytes ? m->weights + (r.offset - base) : nullptr; };
  auto f32 = [&](const LmxTensorRef& r) { return static_cast<const float*>(at(r)); };
  m->pe_w = at(img.pe_w);
  m->pe_b = f32(img.pe_b);
  m->prefix = f32(img.prefix);
  m->pos = f32(img.pos);
  m->rope_cos = f32(img.rope_cos);
  m->rope_sin = f32(img.rope_sin);
  m->gf = f32(img.gf);
  m->bf = f32(img.bf);
  m->lut = f32(img.lut);
  for (const LmxDinoLayerRefs& r : img.layers)
    m->layers.push_back(Layer{f32(r.g1), f32(r.b1), f32(r.bqkv), f32(r.bo), f32(r.ls1), f32(r.g2), f32(r.b2), f32(r.bb1), f32(r.bb2), f32(r.ls2),
                              at(r.wqkv), at(r.wo), at(r.w1), at(r.w2)});

  // the workspace of max_batch frames: the patch matrix and what embed_chunk's plan asks for, one allocation
  DinoRun R("lmx_dino_open_host", nullptr, nullptr);
  LMX_TRY(embed_chunk(R, m, FrameSize(), nullptr, max_batch, 0, 0, 0, nullptr));
  LmxArena whole;  // (the patch matrix is refused like every buffer)
  LMX_TRY(R.take(&whole, "patch matrix", (int64_t)max_batch * c.grid * c.grid * c.k_pad * 2, &m->patches));
  LMX_HIP(hipMalloc(reinterpret_cast<void**>(&m->work), whole.peak + R.arena.peak));
  // the patch matrix's columns beyond 3 * patch^2 (k_pad) are never written by a kernel: zero once, as kernels.patchify_norm's torch.zeros
  LMX_HIP(hipMemset(m->work, 0, whole.peak));
  m->patches = m->work;
  m->arena.base = m->work + whole.peak, m->arena.cap = m->arena.peak = R.arena.peak;
  return LMX_OK;
}

int check_frames(const lmx_dino* m, const char* fn, const void* frames, int n, int h, int w, const void* emb) {
  LMX_TRY(lmx_handle_on_device(m, fn));
  LMX_REQUIRE(n > 0, "%s: n = %d frames", fn, n);
  LMX_REQUIRE(h > 0 && w > 0, "%s: frame size %d x %d", fn, h, w);
  LMX_REQUIRE(frames && emb, "%s: null pointer", fn);
  return LMX_OK;
}

}  // namespace

extern "C" int lmx_dino_open_host(const char* path_host, int max_batch, lmx_dino** out_host) {
  return lmx_handle_open("lmx_dino_open_host", path_host, max_batch, out_host, open_into, destroy);
}

extern "C" void lmx_dino_close(lmx_dino* m) { lmx_handle_close(m, destroy); }

extern "C" int lmx_dino_info(const lmx_dino* m, lmx_dino_info_t* info_host) {
  LMX_REQUIRE(m && info_host, "lmx_dino_info: null argument");
  lmx_dino_fill_info(m->cfg, m->max_batch, info_host);
  return LMX_OK;
}

extern "C" int lmx_dino_prepare(lmx_dino* m, int h, int w) {
  LMX_TRY(lmx_handle_on_device(m, "lmx_dino_prepare"));
  return prepare(m, h, w, nullptr);
}

extern "C" int lmx_dino_embed(lmx_dino* m, const uint8_t* frames, int n, int h, int w, int rgb, float* emb, lmx_stream_t stream) {
  LMX_TRY(check_frames(m, "lmx_dino_embed", frames, n, h, w, emb));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LMX_TRY(lmx_handle_stream_on_device(m, "lmx_dino_embed", st));  // before prepare: a refused call allocates nothing
  const FrameSize* fs = nullptr;
  LMX_TRY(prepare(m, h, w, &fs));  // a size seen before: a lookup
  const size_t frame_bytes = (size_t)h * w * 3;
  DinoRun R("lmx_dino_embed", m, st);
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    LMX_TRY(embed_chunk(R, m, *fs, frames + (size_t)done * frame_bytes, nb, h, w, rgb, emb + (size_t)done * m->cfg.hidden));
  }
  return LMX_OK;
}

extern "C" int lmx_dino_embed_host(lmx_dino* m, const uint8_t* frames_host, int n, int h, int w, int rgb, float* emb_host) {
  LMX_TRY(check_frames(m, "lmx_dino_embed_host", frames_host, n, h, w, emb_host));
  const FrameSize* fs = nullptr;
  LMX_TRY(prepare(m, h, w, &fs));
  const size_t frame_bytes = (size_t)h * w * 3, D = (size_t)m->cfg.hidden;
  // staging of one chunk: frames | embeddings, each on a 256-byte boundary
  const size_t B = (size_t)(n < m->max_batch ? n : m->max_batch);
  LmxLayout lay;
  const size_t o_frames = lay.add(B * frame_bytes), o_emb = lay.add(B * D * sizeof(float));
  LMX_TRY(lmx_handle_grow_stage(m, lay.total));
  uint8_t* frames = reinterpret_cast<uint8_t*>(m->stage + o_frames);
  float* emb = reinterpret_cast<float*>(m->stage + o_emb);
  DinoRun R("lmx_dino_embed_host", m, m->own);
  for (int done = 0; done < n; done += m->max_batch) {
    const int nb = n - done < m->max_batch ? n - done : m->max_batch;
    LMX_HIP(hipMemcpyAsync(frames, frames_host + (size_t)done * frame_bytes, nb * frame_bytes, hipMemcpyHostToDevice, m->own));
    LMX_TRY(embed_chunk(R, m, *fs, frames, nb, h, w, rgb, emb));
    LMX_HIP(hipMemcpyAsync(emb_host + (size_t)done * D, emb, nb * D * sizeof(float), hipMemcpyDeviceToHost, m->own));
    LMX_HIP(hipStreamSynchronize(m->own));
  }
  return LMX_OK;
}
