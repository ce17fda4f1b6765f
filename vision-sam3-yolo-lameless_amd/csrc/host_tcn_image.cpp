// host_tcn_image.cpp — reader of the TCN weight image (tcn_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_tcn_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block (the list of include/lmx.h, through tcn.h's
// lmx_tcn_check_config) and weights_table.h asks for every tensor of the configuration's table (lmx_tcn_tensor_rows, host_tcn.cpp).  A
// malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <string.h>

#include "tcn_image.h"

int lmx_tcn_image_parse(const char* path, LmxTcnImage* img) {
  IMG_REQUIRE(img, "tcn image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("tcn image", path, LMX_IMAGE_TCN, "TCN", &file)) return rc;
  IMG_REQUIRE(file.config.size() == LMX_TCN_CONFIG_BYTES, "tcn image: config_bytes %u, a TCN config block has %d", (unsigned)file.config.size(),
              (int)LMX_TCN_CONFIG_BYTES);
  const unsigned char* raw = file.config.data();
  lmx_tcn_weights_t& c = img->cfg;
  memset(&c, 0, sizeof(c));
  c.input_dim = rd<int32_t>(raw);
  c.n_blocks = rd<int32_t>(raw + 4);
  c.k = rd<int32_t>(raw + 8);
  c.head = rd<int32_t>(raw + 12);
  for (int i = 0; i < LMX_TCN_MAX_BLOCKS; ++i) c.channels[i] = rd<int32_t>(raw + 16 + 4 * i);
  img->p = rd<double>(raw + 48);
  if (const int rc = lmx_tcn_check_config("tcn image", &c, false)) return rc;
  for (int i = c.n_blocks; i < LMX_TCN_MAX_BLOCKS; ++i)
    IMG_REQUIRE(c.channels[i] == 0, "tcn image: channels[%d] = %d beyond n_blocks %d", i, c.channels[i], c.n_blocks);
  IMG_REQUIRE(isfinite(img->p) && img->p >= 0.0 && img->p < 1.0, "tcn image: p %g outside [0, 1)", img->p);
  return lmx_table_take(file, lmx_tcn_tensor_rows, img);
}

void lmx_tcn_fill_info(const LmxTcnImage& img, int max_clips, int max_samples, lmx_tcn_info_t* info) {
  const lmx_tcn_weights_t& c = img.cfg;
  info->input_dim = c.input_dim;
  info->n_blocks = c.n_blocks;
  info->k = c.k;
  info->head = c.head;
  info->receptive_field = lmx_tcn_receptive_field(c.k, c.n_blocks);
  info->max_clips = max_clips;
  info->max_samples = max_samples;
  for (int i = 0; i < LMX_TCN_MAX_BLOCKS; ++i) info->channels[i] = c.channels[i];
  info->p = img.p;
}

extern "C" int lmx_tcn_image_check_host(const char* path_host, lmx_tcn_info_t* info_host) {
  LmxTcnImage img;
  if (const int rc = lmx_tcn_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_tcn_fill_info(img, 0, 0, info_host);
  return LMX_OK;
}
