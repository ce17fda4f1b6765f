// host_gnn_image.cpp — reader of GraphGPS' weight image (gnn_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_gnn_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block (the list of include/lmx.h, through gnn.h's
// lmx_gnn_check_config) and weights_table.h asks for every tensor of the configuration's table (lmx_gnn_tensor_rows, host_gnn.cpp).  A
// malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <string.h>

#include "gnn_image.h"

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
  return lmx_table_take(file, lmx_gnn_tensor_rows, img);
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
