// host_xfm_image.cpp — reader of the gait transformer's weight image (xfm_image.h has the config block and the tensors; image.h the
// container; lmx/native.py write_xfm_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header
// and the directory against the file's real size, this file checks the config block (the list of include/lmx.h, through xfm.h's
// lmx_xfm_check_config) and asks for every tensor the configuration calls for.  A malformed file is LMX_EINVAL with the field named.
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

  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  const int F = c.input_dim, D = c.d_model, H = c.n_heads, dh = D / H, FF = c.ff, QD = D / 16;
  IMG_TAKE(file, "in.w", &img->in_w, "input_dim, d_model", LMX_IMG_F32, 4, lmx_gait_groups(F), QD, 64, 4);
  IMG_TAKE(file, "in.b", &img->in_b, "d_model", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "pe", &img->pe, "max_len, d_model", LMX_IMG_F32, 2, c.max_len, D);
  for (int l = 0; l < c.n_layers; ++l) {
    const std::string b = "layer." + std::to_string(l) + ".";
    LmxTensorRef* t = img->layer[l];
    IMG_TAKE(file, b + "ln1.g", &t[0], "d_model", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, b + "ln1.b", &t[1], "d_model", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, b + "qkv.w", &t[2], "n_heads, d_model", LMX_IMG_F32, 4, H * QD, 3 * dh / 16, 64, 4);
    IMG_TAKE(file, b + "qkv.b", &t[3], "n_heads, d_model", LMX_IMG_F32, 2, H, 3 * dh);
    IMG_TAKE(file, b + "out.w", &t[4], "d_model", LMX_IMG_F32, 4, QD, QD, 64, 4);
    IMG_TAKE(file, b + "out.b", &t[5], "d_model", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, b + "ln2.g", &t[6], "d_model", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, b + "ln2.b", &t[7], "d_model", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, b + "ff1.w", &t[8], "d_model, ff", LMX_IMG_F32, 4, QD, FF / 16, 64, 4);
    IMG_TAKE(file, b + "ff1.b", &t[9], "ff", LMX_IMG_F32, 1, FF);
    IMG_TAKE(file, b + "ff2.w", &t[10], "ff, d_model", LMX_IMG_F32, 4, FF / 16, QD, 64, 4);
    IMG_TAKE(file, b + "ff2.b", &t[11], "d_model", LMX_IMG_F32, 1, D);
  }
  IMG_TAKE(file, "lnf.g", &img->lnf_g, "d_model", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "lnf.b", &img->lnf_b, "d_model", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "head.fc1.w", &img->fc1_w, "head, d_model", LMX_IMG_F32, 2, c.head, D);
  IMG_TAKE(file, "head.fc1.b", &img->fc1_b, "head", LMX_IMG_F32, 1, c.head);
  IMG_TAKE(file, "head.fc2.w", &img->fc2_w, "head", LMX_IMG_F32, 1, c.head);
  IMG_TAKE(file, "head.fc2.b", &img->fc2_b, "one class", LMX_IMG_F32, 1, 1);
  return LMX_OK;
}

void lmx_xfm_bind(const LmxXfmImage& img, const char* data, lmx_xfm_weights_t* w) {
  auto at = [&](const LmxTensorRef& r) { return r.nbytes ? reinterpret_cast<const float*>(data + (r.offset - img.data_offset)) : nullptr; };
  *w = img.cfg;
  w->in_w = at(img.in_w);
  w->in_b = at(img.in_b);
  w->pe = at(img.pe);
  for (int l = 0; l < img.cfg.n_layers; ++l) {
    const LmxTensorRef* t = img.layer[l];
    w->ln1_g[l] = at(t[0]), w->ln1_b[l] = at(t[1]), w->qkv_w[l] = at(t[2]), w->qkv_b[l] = at(t[3]);
    w->out_w[l] = at(t[4]), w->out_b[l] = at(t[5]), w->ln2_g[l] = at(t[6]), w->ln2_b[l] = at(t[7]);
    w->ff1_w[l] = at(t[8]), w->ff1_b[l] = at(t[9]), w->ff2_w[l] = at(t[10]), w->ff2_b[l] = at(t[11]);
  }
  w->lnf_g = at(img.lnf_g);
  w->lnf_b = at(img.lnf_b);
  w->fc1_w = at(img.fc1_w);
  w->fc1_b = at(img.fc1_b);
  w->fc2_w = at(img.fc2_w);
  w->fc2_b = at(img.fc2_b);
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
