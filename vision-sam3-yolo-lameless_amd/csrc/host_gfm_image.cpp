// host_gfm_image.cpp — reader of the graph transformer's weight image (gfm_image.h has the config block and the tensors; image.h the
// container; lmx/native.py write_gfm_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header
// and the directory against the file's real size, this file checks the config block (the list of include/lmx.h, through gfm.h's
// lmx_gfm_check_config) and weights_table.h asks for every tensor of the configuration's table (lmx_gfm_tensor_rows, host_gfm.cpp).  A
// malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <string.h>

#include "gfm_image.h"

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
  return lmx_table_take(file, lmx_gfm_tensor_rows, img);
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
