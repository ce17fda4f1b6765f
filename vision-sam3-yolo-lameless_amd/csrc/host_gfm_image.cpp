// host_gfm_image.cpp — reader of the graph transformer's weight image (gfm_image.h has the config block and the tensors; image.h the
// container; lmx/native.py write_gfm_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header
// and the directory against the file's real size, this file checks the config block (the list of include/lmx.h, through gfm.h's
// lmx_gfm_check_config) and asks for every tensor the configuration calls for.  A malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "gfm_image.h"

namespace {

// the pointers of lmx_gfm_weights_t are one run of `const float*`: 14 in front, 17 arrays of LMX_GFM_MAX_LAYERS, 26 behind
static_assert(offsetof(lmx_gfm_weights_t, ln1_g) == offsetof(lmx_gfm_weights_t, in_w) + LMX_GFM_HEAD_TENSORS * sizeof(float*), "the front tensors");
static_assert(offsetof(lmx_gfm_weights_t, vu1_w) ==
                  offsetof(lmx_gfm_weights_t, ln1_g) + LMX_GFM_LAYER_TENSORS * LMX_GFM_MAX_LAYERS * sizeof(float*),
              "the per-layer tensors");
static_assert(sizeof(lmx_gfm_weights_t) == offsetof(lmx_gfm_weights_t, vu1_w) + LMX_GFM_TAIL_TENSORS * sizeof(float*), "the tensors behind");

struct Want {
  const char* name;
  const char* field;
  int rank, shape[4];
};

}  // namespace

int lmx_gfm_image_parse(const char* path, LmxGfmImage* img) {
  IMG_REQUIRE(img, "gfm image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("gfm image", path, LMX_IMAGE_GFM, "GFM", &file)) return rc;
  IMG_REQUIRE(file.config.size() == LMX_GFM_CONFIG_BYTES, "gfm image: config_bytes %u, a GFM config block has %d", (unsigned)file.config.size(),
              (int)LMX_GFM_CONFIG_BYTES);
  const unsigned char* raw = file.config.data();
  lmx_gfm_weights_t& c = img->cfg;
  memset(&c, 0, sizeof(c));
  c.input_dim = rd<int32_t>(raw);
  c.d_model = rd<int32_t>(raw + 4);
  c.n_heads = rd<int32_t>(raw + 8);
  c.n_layers = rd<int32_t>(raw + 12);
  c.ff = rd<int32_t>(raw + 16);
  c.edge_dim = rd<int32_t>(raw + 20);
  c.max_degree = rd<int32_t>(raw + 24);
  c.max_spd = rd<int32_t>(raw + 28);
  img->p = rd<double>(raw + 32);
  if (const int rc = lmx_gfm_check_config("gfm image", &c, false)) return rc;
  IMG_REQUIRE(isfinite(img->p) && img->p >= 0.0 && img->p < 1.0, "gfm image: p %g outside [0, 1)", img->p);

  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, Q = D / 16, PD = lmx_gfm_pool_dim(D), NI = c.max_spd + 2,
            ND = c.max_degree + 1;
  auto take = [&](const std::string& prefix, const Want& t, LmxTensorRef* ref) {
    const LmxImageWant w = {t.field, LMX_IMG_F32, (uint32_t)t.rank, {t.shape[0], t.shape[1], t.shape[2], t.shape[3]}};
    return lmx_image_take(file, prefix + t.name, w, ref);
  };
  const Want head[LMX_GFM_HEAD_TENSORS] = {
      {"in_w", "input_dim, d_model", 4, {lmx_gait_groups(F), Q, 64, 4}}, {"in_b", "d_model", 1, {D}}, {"in_g", "d_model", 1, {D}},
      {"in_beta", "d_model", 1, {D}}, {"deg_in", "max_degree, d_model", 2, {ND, D}}, {"deg_out", "max_degree, d_model", 2, {ND, D}},
      {"time_w", "d_model", 4, {Q, Q, 64, 4}}, {"time_b", "d_model", 1, {D}}, {"div_term", "d_model", 1, {D / 2}},
      {"spd", "max_spd, n_heads", 2, {NI, H}}, {"e1_w", "n_heads, edge_dim", 2, {2 * H, 3}}, {"e1_b", "n_heads", 1, {2 * H}},
      {"e2_w", "n_heads", 2, {H, 2 * H}}, {"e2_b", "n_heads", 1, {H}}};
  const Want layer[LMX_GFM_LAYER_TENSORS] = {
      {"ln1_g", "d_model", 1, {D}}, {"ln1_b", "d_model", 1, {D}}, {"qkv_w", "n_heads, d_model", 4, {H * Q, 3 * dh / 16, 64, 4}},
      {"qkv_b", "n_heads, d_model", 2, {H, 3 * dh}}, {"out_w", "d_model", 4, {Q, Q, 64, 4}}, {"out_b", "d_model", 1, {D}},
      {"ln2_g", "d_model", 1, {D}}, {"ln2_b", "d_model", 1, {D}}, {"ff1_w", "d_model, ff", 4, {Q, FF / 16, 64, 4}}, {"ff1_b", "ff", 1, {FF}},
      {"ff2_w", "ff, d_model", 4, {FF / 16, Q, 64, 4}}, {"ff2_b", "d_model", 1, {D}}, {"vn", "d_model", 1, {D}},
      {"vqkv_w", "n_heads, d_model", 4, {H * Q, 3 * dh / 16, 64, 4}}, {"vqkv_b", "n_heads, d_model", 2, {H, 3 * dh}},
      {"vout_w", "d_model", 4, {Q, Q, 64, 4}}, {"vout_b", "d_model", 1, {D}}};
  const Want tail[LMX_GFM_TAIL_TENSORS] = {
      {"vu1_w", "d_model", 2, {D, 2 * D}}, {"vu1_b", "d_model", 1, {2 * D}}, {"vu2_w", "d_model", 2, {2 * D, D}}, {"vu2_b", "d_model", 1, {D}},
      {"vu_g", "d_model", 1, {D}}, {"vu_beta", "d_model", 1, {D}}, {"lnf_g", "d_model", 1, {D}}, {"lnf_b", "d_model", 1, {D}},
      {"pool1_w", "d_model", 4, {Q, PD / 16, 64, 4}}, {"pool1_b", "d_model", 1, {PD}}, {"pool2_w", "d_model", 1, {PD}},
      {"pool2_b", "one score", 1, {1}}, {"comb_w", "d_model", 2, {3 * D, D}}, {"comb_b", "d_model", 1, {D}}, {"comb_g", "d_model", 1, {D}},
      {"comb_beta", "d_model", 1, {D}}, {"ph1_w", "d_model", 2, {D, D / 2}}, {"ph1_b", "d_model", 1, {D / 2}},
      {"ph2_w", "d_model", 2, {D / 2, D / 4}}, {"ph2_b", "d_model", 1, {D / 4}}, {"ph3_w", "d_model", 1, {D / 4}}, {"ph3_b", "one class", 1, {1}},
      {"nh1_w", "d_model", 4, {Q, PD / 16, 64, 4}}, {"nh1_b", "d_model", 1, {PD}}, {"nh2_w", "d_model", 1, {PD}}, {"nh2_b", "one score", 1, {1}}};
  for (int i = 0; i < LMX_GFM_HEAD_TENSORS; ++i)
    if (const int rc = take("", head[i], &img->head[i])) return rc;
  for (int l = 0; l < c.n_layers; ++l)
    for (int i = 0; i < LMX_GFM_LAYER_TENSORS; ++i)
      if (const int rc = take("layer." + std::to_string(l) + ".", layer[i], &img->layer[l][i])) return rc;
  for (int i = 0; i < LMX_GFM_TAIL_TENSORS; ++i)
    if (const int rc = take("", tail[i], &img->tail[i])) return rc;
  return LMX_OK;
}

void lmx_gfm_bind(const LmxGfmImage& img, const char* data, lmx_gfm_weights_t* w) {
  auto at = [&](const LmxTensorRef& r) { return r.nbytes ? reinterpret_cast<const float*>(data + (r.offset - img.data_offset)) : nullptr; };
  *w = img.cfg;
  const float** front = &w->in_w;
  const float** layers = &w->ln1_g[0];
  const float** behind = &w->vu1_w;
  for (int i = 0; i < LMX_GFM_HEAD_TENSORS; ++i) front[i] = at(img.head[i]);
  for (int l = 0; l < img.cfg.n_layers; ++l)
    for (int i = 0; i < LMX_GFM_LAYER_TENSORS; ++i) layers[i * LMX_GFM_MAX_LAYERS + l] = at(img.layer[l][i]);
  for (int i = 0; i < LMX_GFM_TAIL_TENSORS; ++i) behind[i] = at(img.tail[i]);
}

void lmx_gfm_fill_info(const LmxGfmImage& img, int max_graphs, int max_nodes_total, int max_samples, lmx_gfm_info_t* info) {
  const lmx_gfm_weights_t& c = img.cfg;
  info->input_dim = c.input_dim, info->d_model = c.d_model, info->n_heads = c.n_heads, info->n_layers = c.n_layers, info->ff = c.ff;
  info->edge_dim = c.edge_dim, info->max_degree = c.max_degree, info->max_spd = c.max_spd, info->max_nodes = LMX_GFM_MAX_NODES;
  info->max_graphs = max_graphs, info->max_nodes_total = max_nodes_total, info->max_samples = max_samples;
  info->p = img.p;
}

extern "C" int lmx_gfm_image_check_host(const char* path_host, lmx_gfm_info_t* info_host) {
  LmxGfmImage img;
  if (const int rc = lmx_gfm_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_gfm_fill_info(img, 0, 0, 0, info_host);
  return LMX_OK;
}
