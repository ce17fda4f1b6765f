// host_gnn_image.cpp — reader of GraphGPS' weight image (gnn_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_gnn_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block (the list of include/lmx.h, through gnn.h's
// lmx_gnn_check_config) and asks for every tensor the configuration calls for.  A malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "gnn_image.h"

namespace {

// the pointers of lmx_gnn_weights_t are one run of `const float*`: 20 in front, 32 arrays of LMX_GNN_MAX_LAYERS, 16 behind
static_assert(offsetof(lmx_gnn_weights_t, ln1_g) == offsetof(lmx_gnn_weights_t, in_w) + LMX_GNN_HEAD_TENSORS * sizeof(float*), "the front tensors");
static_assert(offsetof(lmx_gnn_weights_t, lnf_g) ==
                  offsetof(lmx_gnn_weights_t, ln1_g) + LMX_GNN_LAYER_TENSORS * LMX_GNN_MAX_LAYERS * sizeof(float*),
              "the per-layer tensors");
static_assert(sizeof(lmx_gnn_weights_t) == offsetof(lmx_gnn_weights_t, lnf_g) + LMX_GNN_TAIL_TENSORS * sizeof(float*), "the tensors behind");
static_assert(offsetof(lmx_gnn_weights_t, eu1_w) == offsetof(lmx_gnn_weights_t, ln1_g) + LMX_GNN_EDGE_FIRST * LMX_GNN_MAX_LAYERS * sizeof(float*) &&
                  offsetof(lmx_gnn_weights_t, bnn_g) ==
                      offsetof(lmx_gnn_weights_t, eu1_w) + LMX_GNN_EDGE_TENSORS * LMX_GNN_MAX_LAYERS * sizeof(float*),
              "the edge update's tensors");

struct Want {
  const char* name;
  const char* field;
  int rank, shape[4];
};

}  // namespace

int lmx_gnn_image_parse(const char* path, LmxGnnImage* img) {
  IMG_REQUIRE(img, "gnn image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("gnn image", path, LMX_IMAGE_GNN, "GNN", &file)) return rc;
  IMG_REQUIRE(file.config.size() == LMX_GNN_CONFIG_BYTES, "gnn image: config_bytes %u, a GNN config block has %d", (unsigned)file.config.size(),
              (int)LMX_GNN_CONFIG_BYTES);
  const unsigned char* raw = file.config.data();
  lmx_gnn_weights_t& c = img->cfg;
  memset(&c, 0, sizeof(c));
  c.input_dim = rd<int32_t>(raw);
  c.d_model = rd<int32_t>(raw + 4);
  c.n_heads = rd<int32_t>(raw + 8);
  c.n_layers = rd<int32_t>(raw + 12);
  c.pe_dim = rd<int32_t>(raw + 16);
  c.ff = rd<int32_t>(raw + 20);
  c.edge_dim = rd<int32_t>(raw + 24);
  IMG_REQUIRE(rd<int32_t>(raw + 28) == 0, "gnn image: the reserved word of the config block is %d, not 0", (int)rd<int32_t>(raw + 28));
  img->p = rd<double>(raw + 32);
  if (const int rc = lmx_gnn_check_config("gnn image", &c, false)) return rc;
  IMG_REQUIRE(isfinite(img->p) && img->p >= 0.0 && img->p < 1.0, "gnn image: p %g outside [0, 1)", img->p);

  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, Q = D / 16, P = c.pe_dim, D2 = D / 2;
  auto take = [&](const std::string& prefix, const Want& t, LmxTensorRef* ref) {
    const LmxImageWant w = {t.field, LMX_IMG_F32, (uint32_t)t.rank, {t.shape[0], t.shape[1], t.shape[2], t.shape[3]}};
    return lmx_image_take(file, prefix + t.name, w, ref);
  };
  const Want head[LMX_GNN_HEAD_TENSORS] = {
      {"in_w", "input_dim, d_model, pe_dim", 4, {lmx_gait_groups(F), (D - 2 * P) / 16, 64, 4}}, {"in_b", "d_model, pe_dim", 1, {D - 2 * P}},
      {"lap1_w", "pe_dim", 2, {2 * P, LMX_GNN_LAP_K}}, {"lap1_b", "pe_dim", 1, {2 * P}}, {"lap2_w", "pe_dim", 2, {P, 2 * P}},
      {"lap2_b", "pe_dim", 1, {P}}, {"lap_g", "pe_dim", 1, {P}}, {"lap_beta", "pe_dim", 1, {P}},
      {"rw1_w", "pe_dim", 2, {2 * P, LMX_GNN_RW_K}}, {"rw1_b", "pe_dim", 1, {2 * P}}, {"rw2_w", "pe_dim", 2, {P, 2 * P}},
      {"rw2_b", "pe_dim", 1, {P}}, {"rw_g", "pe_dim", 1, {P}}, {"rw_beta", "pe_dim", 1, {P}},
      {"ee1_w", "d_model, edge_dim", 2, {D2, 3}}, {"ee1_b", "d_model", 1, {D2}}, {"ee2_w", "d_model", 4, {D2 / 16, Q, 64, 4}},
      {"ee2_b", "d_model", 1, {D}}, {"ee_g", "d_model", 1, {D}}, {"ee_beta", "d_model", 1, {D}}};
  const Want layer[LMX_GNN_LAYER_TENSORS] = {
      {"ln1_g", "d_model", 1, {D}}, {"ln1_b", "d_model", 1, {D}}, {"abde_w", "d_model", 4, {Q, 4 * Q, 64, 4}}, {"abde_b", "d_model", 1, {4 * D}},
      {"c_w", "d_model", 4, {Q, Q, 64, 4}}, {"c_b", "d_model", 1, {D}},
      {"eu1_w", "d_model", 4, {3 * Q, Q, 64, 4}}, {"eu1_b", "d_model", 1, {D}}, {"eu2_w", "d_model", 4, {Q, Q, 64, 4}}, {"eu2_b", "d_model", 1, {D}},
      {"bne_g", "d_model", 1, {D}}, {"bne_b", "d_model", 1, {D}}, {"bne_mean", "d_model", 1, {D}}, {"bne_var", "d_model", 1, {D}},
      {"bnn_g", "d_model", 1, {D}}, {"bnn_b", "d_model", 1, {D}}, {"bnn_mean", "d_model", 1, {D}}, {"bnn_var", "d_model", 1, {D}},
      {"ln2_g", "d_model", 1, {D}}, {"ln2_b", "d_model", 1, {D}}, {"qkv_w", "n_heads, d_model", 4, {H * Q, 3 * dh / 16, 64, 4}},
      {"qkv_b", "n_heads, d_model", 2, {H, 3 * dh}}, {"out_w", "d_model", 4, {Q, Q, 64, 4}}, {"out_b", "d_model", 1, {D}},
      {"lna_g", "d_model", 1, {D}}, {"lna_b", "d_model", 1, {D}}, {"ln3_g", "d_model", 1, {D}}, {"ln3_b", "d_model", 1, {D}},
      {"ff1_w", "d_model, ff", 4, {Q, FF / 16, 64, 4}}, {"ff1_b", "ff", 1, {FF}}, {"ff2_w", "ff, d_model", 4, {FF / 16, Q, 64, 4}},
      {"ff2_b", "d_model", 1, {D}}};
  const Want tail[LMX_GNN_TAIL_TENSORS] = {
      {"lnf_g", "d_model", 1, {D}}, {"lnf_b", "d_model", 1, {D}}, {"nh1_w", "d_model", 4, {Q, D2 / 16, 64, 4}}, {"nh1_b", "d_model", 1, {D2}},
      {"nh2_w", "d_model", 1, {D2}}, {"nh2_b", "one score", 1, {1}}, {"na1_w", "d_model", 4, {Q, D2 / 16, 64, 4}}, {"na1_b", "d_model", 1, {D2}},
      {"na2_w", "d_model", 1, {D2}}, {"na2_b", "one score", 1, {1}}, {"cl1_w", "d_model", 2, {2 * D, D}}, {"cl1_b", "d_model", 1, {D}},
      {"cl2_w", "d_model", 2, {D, D2}}, {"cl2_b", "d_model", 1, {D2}}, {"cl3_w", "d_model", 1, {D2}}, {"cl3_b", "one class", 1, {1}}};
  for (int i = 0; i < LMX_GNN_HEAD_TENSORS; ++i)
    if (const int rc = take("", head[i], &img->head[i])) return rc;
  for (int l = 0; l < c.n_layers; ++l)
    for (int i = 0; i < LMX_GNN_LAYER_TENSORS; ++i) {
      const bool edge = i >= LMX_GNN_EDGE_FIRST && i < LMX_GNN_EDGE_FIRST + LMX_GNN_EDGE_TENSORS;
      if (edge && l == c.n_layers - 1) {  // the last live layer's edge update reaches no output and is not in the image
        img->layer[l][i] = LmxTensorRef();
        continue;
      }
      if (const int rc = take("layer." + std::to_string(l) + ".", layer[i], &img->layer[l][i])) return rc;
    }
  for (int i = 0; i < LMX_GNN_TAIL_TENSORS; ++i)
    if (const int rc = take("", tail[i], &img->tail[i])) return rc;
  return LMX_OK;
}

void lmx_gnn_bind(const LmxGnnImage& img, const char* data, lmx_gnn_weights_t* w) {
  auto at = [&](const LmxTensorRef& r) { return r.nbytes ? reinterpret_cast<const float*>(data + (r.offset - img.data_offset)) : nullptr; };
  *w = img.cfg;
  const float** front = &w->in_w;
  const float** layers = &w->ln1_g[0];
  const float** behind = &w->lnf_g;
  for (int i = 0; i < LMX_GNN_HEAD_TENSORS; ++i) front[i] = at(img.head[i]);
  for (int l = 0; l < img.cfg.n_layers; ++l)
    for (int i = 0; i < LMX_GNN_LAYER_TENSORS; ++i) layers[i * LMX_GNN_MAX_LAYERS + l] = at(img.layer[l][i]);
  for (int i = 0; i < LMX_GNN_TAIL_TENSORS; ++i) behind[i] = at(img.tail[i]);
}

void lmx_gnn_fill_info(const LmxGnnImage& img, int max_graphs, int max_nodes_total, int max_edges_total, int max_samples, lmx_gnn_info_t* info) {
  const lmx_gnn_weights_t& c = img.cfg;
  info->input_dim = c.input_dim, info->d_model = c.d_model, info->n_heads = c.n_heads, info->n_layers = c.n_layers, info->pe_dim = c.pe_dim;
  info->ff = c.ff, info->edge_dim = c.edge_dim, info->max_nodes = LMX_GNN_MAX_NODES, info->max_edges = LMX_GNN_MAX_EDGES;
  info->max_graphs = max_graphs, info->max_nodes_total = max_nodes_total, info->max_edges_total = max_edges_total, info->max_samples = max_samples;
  info->reserved = 0;
  info->p = img.p;
}

extern "C" int lmx_gnn_image_check_host(const char* path_host, lmx_gnn_info_t* info_host) {
  LmxGnnImage img;
  if (const int rc = lmx_gnn_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_gnn_fill_info(img, 0, 0, 0, 0, info_host);
  return LMX_OK;
}
