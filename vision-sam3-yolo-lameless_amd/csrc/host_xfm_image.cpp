// host_xfm_image.cpp — reader of the gait transformer's weight image (xfm_image.h has the config block and the tensors; image.h the
// container; lmx/native.py write_xfm_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header
// and the directory against the file's real size, this file checks the config block (the list of include/lmx.h, through xfm.h's
// lmx_xfm_check_config) and weights_table.h asks for every tensor of the configuration's table (lmx_xfm_tensor_rows, host_xfm.cpp).  A
// malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <string.h>

#include "xfm_image.h"

int lmx_xfm_image_parse(const char* path, LmxXfmImage* img) {
  IMG_REQUIRE(img, "xfm image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("xfm image", path, LMX_IMAGE_XFM, "XFM", &file)) return rc;
  IMG_REQUIRE(file.config.size() == LMX_XFM_CONFIG_BYTES, "xfm image: config_bytes %u, an XFM config block has %d", (unsigned)file.config.size(),
              (int)LMX_XFM_CONFIG_BYTES);
  const unsigned char* raw = file.config.data();
  lmx_xfm_weights_t& c = img->cfg;
  memset(&c, 0, sizeof(c));
  c.input_dim = rd<int32_t>(raw);
  c.d_model = rd<int32_t>(raw + 4);
  c.n_heads = rd<int32_t>(raw + 8);
  c.n_layers = rd<int32_t>(raw + 12);
  c.ff = rd<int32_t>(raw + 16);
  c.head = rd<int32_t>(raw + 20);
  c.max_len = rd<int32_t>(raw + 24);
  c.reserved = rd<int32_t>(raw + 28);
  img->p = rd<double>(raw + 32);
  if (const int rc = lmx_xfm_check_config("xfm image", &c, false)) return rc;
  IMG_REQUIRE(c.reserved == 0, "xfm image: reserved config word is %d", c.reserved);
  IMG_REQUIRE(isfinite(img->p) && img->p >= 0.0 && img->p < 1.0, "xfm image: p %g outside [0, 1)", img->p);
  return lmx_table_take(file, lmx_xfm_tensor_rows, img);
}

void lmx_xfm_fill_info(const LmxXfmImage& img, int max_clips, int max_samples, lmx_xfm_info_t* info) {
  const lmx_xfm_weights_t& c = img.cfg;
  info->input_dim = c.input_dim;
  info->d_model = c.d_model;
  info->n_heads = c.n_heads;
  info->n_layers = c.n_layers;
  info->ff = c.ff;
  info->head = c.head;
  info->max_len = c.max_len;
  info->max_clips = max_clips;
  info->max_samples = max_samples;
  info->reserved = 0;
  info->p = img.p;
}

extern "C" int lmx_xfm_image_check_host(const char* path_host, lmx_xfm_info_t* info_host) {
  LmxXfmImage img;
  if (const int rc = lmx_xfm_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_xfm_fill_info(img, 0, 0, info_host);
  return LMX_OK;
}
