// host_sam_image.cpp — reader of the SAM weight image (sam_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_sam_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block and asks for every tensor the configuration calls for,
// per plan the image claims to hold.  Everything the model handle later allocates or indexes by (sam_model.hip) comes out of here
// validated; a malformed file is LMX_EINVAL with the field or tensor named.
#include <math.h>

#include "sam_image.h"

namespace {

int check_config(const LmxSamCfg& c) {
  IMG_REQUIRE(c.encoder == LMX_SAM_ENC_VIT, "sam image: encoder %d is not the SAM v1 ViT (%d); no other encoder is served", c.encoder,
              (int)LMX_SAM_ENC_VIT);
  IMG_REQUIRE(c.hidden > 0 && c.hidden <= 16384 && c.hidden % 8 == 0, "sam image: hidden %d (a multiple of 8 up to 16384)", c.hidden);
  IMG_REQUIRE(c.heads > 0 && c.hidden % c.heads == 0, "sam image: hidden %d is not a multiple of heads %d", c.hidden, c.heads);
  const int hd = c.hidden / c.heads;
  IMG_REQUIRE(hd % 8 == 0 && hd <= 96,
              "sam image: head dim %d (hidden %d / heads %d) is not supported: the attention kernels serve multiples of 8 up to 96", hd, c.hidden,
              c.heads);
  IMG_REQUIRE(c.layers > 0 && c.layers <= 1024, "sam image: layers %d", c.layers);
  IMG_REQUIRE(c.mlp > 0 && c.mlp <= 65536 && c.mlp % 8 == 0, "sam image: mlp %d (a multiple of 8 up to 65536)", c.mlp);
  IMG_REQUIRE(c.patch > 0 && c.patch <= 64 && c.patch * c.patch * 3 % 8 == 0, "sam image: patch %d (3 * patch^2 a multiple of 8, patch up to 64)", c.patch);
  IMG_REQUIRE(c.image >= c.patch && c.image <= 8192 && c.image % c.patch == 0, "sam image: image %d is not a multiple of patch %d (up to 8192)", c.image,
              c.patch);
  const int g = c.image / c.patch;
  IMG_REQUIRE(c.window > 0 && c.window <= g, "sam image: window %d against a grid of %d", c.window, g);
  IMG_REQUIRE(c.out_ch == LMX_SAM_DEC_D, "sam image: out_ch %d is not the mask decoder's width %d", c.out_ch, (int)LMX_SAM_DEC_D);
  IMG_REQUIRE(c.plans >= 1 && c.plans <= 3, "sam image: plans mask %d holds no plan (bit 0: f16, bit 1: exact)", c.plans);
  IMG_REQUIRE(c.n_global >= 0 && c.n_global <= c.layers, "sam image: n_global %d for %d layers", c.n_global, c.layers);
  IMG_REQUIRE(c.reserved == 0, "sam image: reserved config field is %d, not 0", c.reserved);
  IMG_REQUIRE(isfinite(c.eps) && c.eps > 0.0, "sam image: eps %g", c.eps);
  if (c.plans & (1 << LMX_SAM_EXACT)) {
    // SamVitEncoder.embed's `lin` takes its one-launch route (lmx_k_gemm a_rep = 2) under these conditions only; the explicit
    // [a | a] copy it makes for toy shapes is not restated in C++
    const int Kp = c.patch * c.patch * 3;
    IMG_REQUIRE(c.hidden % 64 == 0, "sam image: the exact plan needs hidden %d to be a multiple of 64 (one launch per Linear, a_rep = 2)", c.hidden);
    IMG_REQUIRE(c.mlp % 64 == 0, "sam image: the exact plan needs mlp %d to be a multiple of 64 (one launch per Linear, a_rep = 2)", c.mlp);
    IMG_REQUIRE(Kp % 64 == 0, "sam image: the exact plan needs 3 * patch^2 = %d (patch %d) to be a multiple of 64", Kp, c.patch);
    IMG_REQUIRE(g * g >= 512, "sam image: the exact plan needs (image %d / patch %d)^2 tokens of at least 512 (the LDS-DMA GEMM's M)", c.image, c.patch);
    IMG_REQUIRE(c.hidden >= 96 && c.mlp >= 96, "sam image: the exact plan needs hidden %d and mlp %d of at least 96 (the LDS-DMA GEMM's N)", c.hidden,
                c.mlp);
  }
  return LMX_OK;
}

}  // namespace

std::vector<LmxSamLinear> lmx_sam_linears() {
  std::vector<LmxSamLinear> out;
  auto add = [&](const std::string& name, int N, int K) {
    LmxSamLinear l;
    l.name = name;
    l.N = N;
    l.K = K;
    out.push_back(l);
  };
  const int D = LMX_SAM_DEC_D;
  auto attn = [&](const std::string& p, int inner) {
    add(p + ".q", inner, D);
    add(p + ".k", inner, D);
    add(p + ".v", inner, D);
    add(p + ".o", D, inner);
  };
  for (int i = 0; i < 2; ++i) {
    const std::string p = "L" + std::to_string(i);
    attn(p + ".sa", D);
    attn(p + ".t2i", D / 2);
    add(p + ".lin1", LMX_SAM_DEC_MLP, D);
    add(p + ".lin2", D, LMX_SAM_DEC_MLP);
    attn(p + ".i2t", D / 2);
  }
  attn("fin", D / 2);
  add("up1", 4 * 64, D);
  add("up2", 4 * 32, 64);
  add("hyp0.in", D, D);
  add("hyp0.mid", D, D);
  add("hyp0.out", 32, D);
  add("iou.in", D, D);
  add("iou.mid", D, D);
  add("iou.out", 4, D);
  return out;
}

void lmx_sam_resized_hw(int image, int h, int w, int* nh, int* nw) {
  const double scale = (double)image * 1.0 / (double)(h > w ? h : w);
  const double fh = (double)h * scale, fw = (double)w * scale;  // (rounded products first: Python's h * scale + 0.5 has no fused step)
  *nh = (int)(fh + 0.5);
  *nw = (int)(fw + 0.5);
}

void lmx_sam_fill_info(const LmxSamCfg& c, int max_batch, lmx_sam_info_t* info) {
  info->encoder = c.encoder;
  info->hidden = c.hidden;
  info->heads = c.heads;
  info->layers = c.layers;
  info->mlp = c.mlp;
  info->window = c.window;
  info->patch = c.patch;
  info->image = c.image;
  info->plans = c.plans;
  info->max_batch = max_batch;
}

int lmx_sam_image_parse(const char* path, LmxSamImage* img) {
  IMG_REQUIRE(img, "sam image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("sam image", path, LMX_IMAGE_SAM, "SAM", &file)) return rc;
  const std::vector<unsigned char>& cb = file.config;
  const uint32_t fixed = LMX_SAM_CONFIG_INTS * 4 + 8, config_bytes = (uint32_t)cb.size();
  IMG_REQUIRE(config_bytes >= fixed && config_bytes % 8 == 0,
              "sam image: config_bytes %u (a multiple of 8 from %u: %d integers, eps, then the global-attention layer indices)", config_bytes, fixed,
              (int)LMX_SAM_CONFIG_INTS);
  LmxSamCfg& c = img->cfg;
  int32_t* ints[LMX_SAM_CONFIG_INTS] = {&c.encoder, &c.hidden, &c.heads, &c.layers, &c.mlp,      &c.window,
                                        &c.patch,   &c.image,  &c.out_ch, &c.plans, &c.n_global, &c.reserved};
  for (int i = 0; i < LMX_SAM_CONFIG_INTS; ++i) *ints[i] = rd<int32_t>(cb.data() + 4 * i);
  c.eps = rd<double>(cb.data() + 4 * LMX_SAM_CONFIG_INTS);
  if (const int rc = check_config(c)) return rc;
  IMG_REQUIRE((uint32_t)((c.n_global * 4 + 7) / 8 * 8) == config_bytes - fixed,
              "sam image: n_global %d indices (padded to 8 bytes) do not fill the %u bytes the config block has behind eps", c.n_global,
              config_bytes - fixed);
  c.global_idx.clear();
  for (int i = 0; i < c.n_global; ++i) {
    const int32_t g = rd<int32_t>(cb.data() + fixed + 4 * i);
    IMG_REQUIRE(g >= 0 && g < c.layers, "sam image: global_idx[%d] = %d is not a layer of 0 .. %d", i, g, c.layers - 1);
    IMG_REQUIRE(i == 0 || g > c.global_idx.back(), "sam image: global_idx[%d] = %d does not ascend", i, g);
    c.global_idx.push_back(g);
  }
  for (uint32_t at = fixed + 4u * (uint32_t)c.n_global; at < config_bytes; ++at)
    IMG_REQUIRE(cb[at] == 0, "sam image: the padding behind the %d global_idx entries is not zero", c.n_global);

  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  const bool f16 = c.plans & (1 << LMX_SAM_F16), exact = c.plans & (1 << LMX_SAM_EXACT);
  const int D = c.hidden, I = c.mlp, g = c.grid(), Kp = c.patch * c.patch * 3, hd = D / c.heads, C = c.out_ch;
  // the encoder
  IMG_TAKE(file, "enc.pe_b", &img->pe_b, "hidden", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "enc.pos", &img->pos, "(image / patch)^2, hidden", LMX_IMG_F32, 2, g * g, D);
  IMG_TAKE(file, "enc.lut", &img->lut, "3, 256", LMX_IMG_F32, 2, 3, 256);
  IMG_TAKE(file, "enc.n1.g", &img->n1_g, "out_ch", LMX_IMG_F32, 1, C);
  IMG_TAKE(file, "enc.n1.b", &img->n1_b, "out_ch", LMX_IMG_F32, 1, C);
  IMG_TAKE(file, "enc.n2.g", &img->n2_g, "out_ch", LMX_IMG_F32, 1, C);
  IMG_TAKE(file, "enc.n2.b", &img->n2_b, "out_ch", LMX_IMG_F32, 1, C);
  if (f16) {
    IMG_TAKE(file, "enc.pe_w", &img->pe_w, "hidden, 3 * patch^2", LMX_IMG_F16, 2, D, Kp);
    IMG_TAKE(file, "enc.n1.w", &img->n1_w, "out_ch, hidden", LMX_IMG_F16, 2, C, D);
    IMG_TAKE(file, "enc.n2.w", &img->n2_w, "out_ch, 9 * out_ch", LMX_IMG_F16, 2, C, 9 * C);
  }
  if (exact) {
    IMG_TAKE(file, "enc.x2.pe", &img->x_pe, "hidden, 2 * 3 * patch^2", LMX_IMG_F16, 2, D, 2 * Kp);
    IMG_TAKE(file, "enc.x2.n1", &img->x_n1, "out_ch, 2 * hidden", LMX_IMG_F16, 2, C, 2 * D);
    IMG_TAKE(file, "enc.x2.n2.hi", &img->x_n2_hi, "out_ch, 9 * out_ch", LMX_IMG_F16, 2, C, 9 * C);
    IMG_TAKE(file, "enc.x2.n2.lo", &img->x_n2_lo, "out_ch, 9 * out_ch", LMX_IMG_F16, 2, C, 9 * C);
  }
  img->layers.assign((size_t)c.layers, LmxSamLayerRefs());
  for (int i = 0; i < c.layers; ++i) {
    LmxSamLayerRefs& L = img->layers[(size_t)i];
    const std::string p = "enc.L" + std::to_string(i) + ".", x = "enc.x2.L" + std::to_string(i) + ".";
    const int S = c.is_global(i) ? g : c.window;
    IMG_TAKE(file, p + "g1", &L.g1, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "b1", &L.b1, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "bqkv", &L.bqkv, "3 * hidden", LMX_IMG_F32, 1, 3 * D);
    IMG_TAKE(file, p + "padkv", &L.padkv, "3 * hidden", LMX_IMG_F16, 1, 3 * D);
    IMG_TAKE(file, p + "rh", &L.rh, "2 S - 1, hidden / heads; S = image / patch for a layer of global_idx, window otherwise", LMX_IMG_F32, 2, 2 * S - 1,
             hd);
    IMG_TAKE(file, p + "rw", &L.rw, "2 S - 1, hidden / heads; S = image / patch for a layer of global_idx, window otherwise", LMX_IMG_F32, 2, 2 * S - 1,
             hd);
    IMG_TAKE(file, p + "bo", &L.bo, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "g2", &L.g2, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "b2", &L.b2, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "bb1", &L.bb1, "mlp", LMX_IMG_F32, 1, I);
    IMG_TAKE(file, p + "bb2", &L.bb2, "hidden", LMX_IMG_F32, 1, D);
    if (f16) {
      IMG_TAKE(file, p + "wqkv", &L.wqkv, "3 * hidden, hidden", LMX_IMG_F16, 2, 3 * D, D);
      IMG_TAKE(file, p + "wo", &L.wo, "hidden, hidden", LMX_IMG_F16, 2, D, D);
      IMG_TAKE(file, p + "w1", &L.w1, "mlp, hidden", LMX_IMG_F16, 2, I, D);
      IMG_TAKE(file, p + "w2", &L.w2, "hidden, mlp", LMX_IMG_F16, 2, D, I);
    }
    if (exact) {
      IMG_TAKE(file, x + "qkv", &L.xqkv, "3 * hidden, 2 * hidden", LMX_IMG_F16, 2, 3 * D, 2 * D);
      IMG_TAKE(file, x + "proj", &L.xproj, "hidden, 2 * hidden", LMX_IMG_F16, 2, D, 2 * D);
      IMG_TAKE(file, x + "fc1", &L.xfc1, "mlp, 2 * hidden", LMX_IMG_F16, 2, I, 2 * D);
      IMG_TAKE(file, x + "fc2", &L.xfc2, "hidden, 2 * mlp", LMX_IMG_F16, 2, D, 2 * I);
    }
  }
  // the prompt encoder and the mask decoder
  const int DD = LMX_SAM_DEC_D;
  IMG_TAKE(file, "dec.gauss", &img->gauss, "2, 128", LMX_IMG_F32, 2, 2, DD / 2);
  IMG_TAKE(file, "dec.corner", &img->corner, "2, 256", LMX_IMG_F32, 2, 2, DD);
  IMG_TAKE(file, "dec.key_pe", &img->key_pe, "(image / patch)^2, 256", LMX_IMG_F32, 2, g * g, DD);
  IMG_TAKE(file, "dec.no_mask", &img->no_mask, "1, 256", LMX_IMG_F32, 2, 1, DD);
  IMG_TAKE(file, "dec.out_tokens", &img->out_tokens, "5, 256", LMX_IMG_F32, 2, (int)LMX_SAM_OUT_TOKENS, DD);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 4; ++j) {
      const std::string p = "dec.L" + std::to_string(i) + ".ln" + std::to_string(j + 1);
      IMG_TAKE(file, p + ".g", &img->dec_ln[i][j].g, "256", LMX_IMG_F32, 1, DD);
      IMG_TAKE(file, p + ".b", &img->dec_ln[i][j].b, "256", LMX_IMG_F32, 1, DD);
    }
  IMG_TAKE(file, "dec.ln_final.g", &img->ln_final.g, "256", LMX_IMG_F32, 1, DD);
  IMG_TAKE(file, "dec.ln_final.b", &img->ln_final.b, "256", LMX_IMG_F32, 1, DD);
  IMG_TAKE(file, "dec.up_ln.g", &img->up_ln.g, "64", LMX_IMG_F32, 1, 64);
  IMG_TAKE(file, "dec.up_ln.b", &img->up_ln.b, "64", LMX_IMG_F32, 1, 64);
  img->linears = lmx_sam_linears();
  for (LmxSamLinear& l : img->linears) {
    if (f16) {
      IMG_TAKE(file, "dec.f16." + l.name + ".w", &l.w, "N, K of the mask decoder's Linear", LMX_IMG_F16, 2, l.N, l.K);
      IMG_TAKE(file, "dec.f16." + l.name + ".b", &l.b, "N of the mask decoder's Linear", LMX_IMG_F32, 1, l.N);
    }
    if (exact) {
      IMG_TAKE(file, "dec.x3." + l.name + ".w", &l.xw, "N, 3 K of the mask decoder's Linear", LMX_IMG_F16, 2, l.N, 3 * l.K);
      IMG_TAKE(file, "dec.x3." + l.name + ".b", &l.xb, "N of the mask decoder's Linear", LMX_IMG_F32, 1, l.N);
      IMG_TAKE(file, "dec.x3." + l.name + ".s", &l.xs, "N of the mask decoder's Linear", LMX_IMG_F32, 1, l.N);
    }
  }
  return LMX_OK;
}

extern "C" int lmx_sam_image_check_host(const char* path_host, lmx_sam_info_t* info_host) {
  LmxSamImage img;
  if (const int rc = lmx_sam_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_sam_fill_info(img.cfg, 0, info_host);
  return LMX_OK;
}
