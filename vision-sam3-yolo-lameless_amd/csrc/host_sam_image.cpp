// host_sam_image.cpp — reader of the SAM weight image (sam_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_sam_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block and asks for every tensor the configuration calls for,
// per plan the image claims to hold.  Everything the model handle later allocates or indexes by (sam_model.hip) comes out of here
// validated; a malformed file is LMX_EINVAL with the field or tensor named.
#include <math.h>
#include <string.h>

#include "sam_image.h"

namespace {

int check_config(const LmxSamCfg& c) {
  IMG_REQUIRE(c.encoder == LMX_SAM_ENC_VIT, "sam image: encoder %d is not the SAM v1 ViT (%d) nor Hiera (%d); no other encoder is served", c.encoder,
              (int)LMX_SAM_ENC_VIT, (int)LMX_SAM_ENC_HIERA);
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

namespace {

// the prompt encoder and the mask decoder of either encoder's image, for the plans of img->cfg.plans; g: the embedding's grid
int take_decoder(const LmxImageFile& file, LmxSamImage* img, int g) {
  const bool f16 = img->cfg.plans & (1 << LMX_SAM_F16), exact = img->cfg.plans & (1 << LMX_SAM_EXACT);
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

// ---- encoder Hiera: the config block behind `encoder` (sam_image.h), the block table it stands for, and every tensor of it ----------
enum { HIERA_INTS = 12, HIERA_KPAD = 152 };

int parse_hiera(const LmxImageFile& file, LmxSamImage* img) {
  const std::vector<unsigned char>& cb = file.config;
  const uint32_t fixed = HIERA_INTS * 4 + 8, config_bytes = (uint32_t)cb.size();  // (at least `fixed`, a multiple of 8: checked by the caller)
  int32_t v[HIERA_INTS];
  for (int i = 0; i < HIERA_INTS; ++i) v[i] = rd<int32_t>(cb.data() + 4 * i);
  LmxSamCfg& c = img->cfg;
  lmx_hiera_config_t& hc = c.hiera;
  memset(&hc, 0, sizeof(hc));
  const int n_blocks = v[3];
  hc.hidden = v[1], hc.n_stages = v[2], hc.n_global = v[4], hc.n_top_down = v[5], hc.q_pool_stages = v[6], hc.image = v[7], hc.fpn_dim = v[8];
  hc.pos_bkg[0] = v[10], hc.pos_bkg[1] = v[11];
  hc.eps = rd<double>(cb.data() + 4 * HIERA_INTS);
  IMG_REQUIRE(hc.n_stages >= 3 && hc.n_stages <= LMX_HIERA_MAX_STAGES, "sam image: hiera n_stages %d (3 .. %d: the embedding is the third stage's level)",
              hc.n_stages, (int)LMX_HIERA_MAX_STAGES);
  IMG_REQUIRE(hc.n_global >= 0 && hc.n_global <= LMX_HIERA_MAX_GLOBAL, "sam image: hiera n_global %d (0 .. %d)", hc.n_global, (int)LMX_HIERA_MAX_GLOBAL);
  IMG_REQUIRE(hc.n_top_down >= 0 && hc.n_top_down <= LMX_HIERA_MAX_STAGES, "sam image: hiera n_top_down %d (0 .. %d)", hc.n_top_down, (int)LMX_HIERA_MAX_STAGES);
  const uint32_t n_tail = 4u * (uint32_t)hc.n_stages + (uint32_t)hc.n_global + (uint32_t)hc.n_top_down;
  IMG_REQUIRE((n_tail * 4 + 7) / 8 * 8 == config_bytes - fixed,
              "sam image: hiera n_stages %d, n_global %d, n_top_down %d call for %u integers (padded to 8 bytes) behind eps, the config block has %u bytes there",
              hc.n_stages, hc.n_global, hc.n_top_down, n_tail, config_bytes - fixed);
  const unsigned char* at = cb.data() + fixed;
  int32_t* per_stage[4] = {hc.blocks, hc.dims, hc.heads, hc.windows};
  for (int32_t* a : per_stage)
    for (int s = 0; s < hc.n_stages; ++s, at += 4) a[s] = rd<int32_t>(at);
  for (int i = 0; i < hc.n_global; ++i, at += 4) hc.global_blocks[i] = rd<int32_t>(at);
  for (int i = 0; i < hc.n_top_down; ++i, at += 4) hc.fpn_top_down[i] = rd<int32_t>(at);
  for (; at < cb.data() + config_bytes; ++at) IMG_REQUIRE(*at == 0, "sam image: the padding behind the hiera config arrays is not zero");
  int nb = 0;
  if (const int rc = lmx_hiera_check_config(&hc, "sam image: hiera", &nb)) return rc;
  IMG_REQUIRE(nb == n_blocks, "sam image: hiera n_blocks %d is not the sum of blocks[], %d", n_blocks, nb);
  for (int i = 0; i < hc.n_global; ++i)
    IMG_REQUIRE(i == 0 || hc.global_blocks[i] > hc.global_blocks[i - 1], "sam image: hiera global_blocks[%d] = %d does not ascend", i, hc.global_blocks[i]);
  for (int i = 0; i < hc.n_top_down; ++i)
    IMG_REQUIRE(hc.fpn_top_down[i] >= 0 && hc.fpn_top_down[i] < hc.n_stages, "sam image: hiera fpn_top_down[%d] = %d is not a stage of 0 .. %d", i,
                hc.fpn_top_down[i], hc.n_stages - 1);
  IMG_REQUIRE(hc.hidden == hc.dims[0], "sam image: hiera hidden %d is not dims[0] = %d", hc.hidden, hc.dims[0]);
  IMG_REQUIRE(hc.pos_bkg[0] > 0 && hc.pos_bkg[1] > 0, "sam image: hiera pos_bkg %d x %d", hc.pos_bkg[0], hc.pos_bkg[1]);
  IMG_REQUIRE(isfinite(hc.eps) && hc.eps > 0.0, "sam image: hiera eps %g", hc.eps);
  c.plans = v[9];
  IMG_REQUIRE(c.plans >= 1 && c.plans <= 3, "sam image: plans mask %d holds no plan (bit 0: f16, bit 1: exact)", c.plans);
  // the decoder's grid: the embedding is level 2 of the FPN, [image / 16][image / 16][fpn_dim], and must be [64][64][256]
  IMG_REQUIRE(hc.q_pool_stages >= 2, "sam image: hiera q_pool_stages %d: the embedding's level is a sixteenth of the image only behind two pooling stages",
              hc.q_pool_stages);
  IMG_REQUIRE(hc.image % 16 == 0 && hc.image / 16 == 64, "sam image: hiera image %d: the mask decoder reads an embedding of 64 x 64, image / 16 is %d", hc.image,
              hc.image / 16);
  IMG_REQUIRE(hc.fpn_dim == LMX_SAM_DEC_D, "sam image: hiera fpn_dim %d is not the mask decoder's width %d", hc.fpn_dim, (int)LMX_SAM_DEC_D);
  c.hidden = hc.dims[0], c.heads = hc.heads[0], c.layers = nb, c.mlp = 0, c.window = hc.windows[0], c.patch = 16, c.image = hc.image, c.out_ch = hc.fpn_dim;
  c.n_global = hc.n_global, c.reserved = 0, c.eps = hc.eps;
  c.global_idx.assign(hc.global_blocks, hc.global_blocks + hc.n_global);

  std::vector<LmxHieraBlock> blocks((size_t)nb);
  std::vector<int> stage_end((size_t)nb);
  lmx_hiera_block_table(&hc, blocks.data(), stage_end.data());
  const int g4 = hc.image / 4;
  IMG_TAKE(file, "enc.pe_w", &img->pe_w, "hidden, 152", LMX_IMG_F16, 2, hc.hidden, (int)HIERA_KPAD);
  IMG_TAKE(file, "enc.pe_b", &img->pe_b, "hidden", LMX_IMG_F32, 1, hc.hidden);
  IMG_TAKE(file, "enc.pos", &img->pos, "(image / 4)^2, hidden", LMX_IMG_F32, 2, g4 * g4, hc.hidden);
  IMG_TAKE(file, "enc.lut", &img->lut, "3, 256", LMX_IMG_F32, 2, 3, 256);
  img->hiera_blocks.assign((size_t)nb, LmxHieraBlockRefs());
  for (int i = 0; i < nb; ++i) {
    LmxHieraBlockRefs& B = img->hiera_blocks[(size_t)i];
    const LmxHieraBlock& b = B.shape = blocks[(size_t)i];
    const int Din = b.dim, D = b.D, H = b.heads;
    IMG_REQUIRE(Din % 8 == 0 && D % 8 == 0, "sam image: hiera block %d: dims %d -> %d are not multiples of 8 (the GEMMs' K)", i, Din, D);
    IMG_REQUIRE(D % H == 0, "sam image: hiera block %d: dim %d is not a multiple of heads %d", i, D, H);
    B.fused = lmx_hiera_fused_attn(b);
    // a block of a fused class takes the launch path where the grid is not whole windows, so every block needs a head dim it serves
    IMG_REQUIRE(D / H % 8 == 0 && D / H <= 96,
                "sam image: hiera block %d: head dim %d (dims %d / heads %d) is not supported: the attention kernels serve multiples of 8 up to 96", i, D / H, D,
                H);
    const std::string p = "enc.B" + std::to_string(i) + ".";
    IMG_TAKE(file, p + "g1", &B.g1, "dims (the block's input width)", LMX_IMG_F32, 1, Din);
    IMG_TAKE(file, p + "b1", &B.b1, "dims (the block's input width)", LMX_IMG_F32, 1, Din);
    IMG_TAKE(file, p + "wqkv", &B.wqkv, "3 * dims, dims (output, input width of the block)", LMX_IMG_F16, 2, 3 * D, Din);
    IMG_TAKE(file, p + "bqkv", &B.bqkv, "3 * dims", LMX_IMG_F32, 1, 3 * D);
    IMG_TAKE(file, p + "padkv", &B.padkv, "3 * dims", LMX_IMG_F16, 1, 3 * D);
    IMG_TAKE(file, p + "wo", &B.wo, "dims, dims", LMX_IMG_F16, 2, D, D);
    IMG_TAKE(file, p + "bo", &B.bo, "dims", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "g2", &B.g2, "dims", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "b2", &B.b2, "dims", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "w1", &B.w1, "4 * dims, dims", LMX_IMG_F16, 2, 4 * D, D);
    IMG_TAKE(file, p + "bb1", &B.bb1, "4 * dims", LMX_IMG_F32, 1, 4 * D);
    IMG_TAKE(file, p + "w2", &B.w2, "dims, 4 * dims", LMX_IMG_F16, 2, D, 4 * D);
    IMG_TAKE(file, p + "bb2", &B.bb2, "dims", LMX_IMG_F32, 1, D);
    if (Din != D) {
      IMG_TAKE(file, p + "wp", &B.wp, "dims, dims (output, input width of a block that opens a stage)", LMX_IMG_F16, 2, D, Din);
      IMG_TAKE(file, p + "bp", &B.bp, "dims", LMX_IMG_F32, 1, D);
    }
    if (B.fused == LMX_HIERA_ATTN8) {
      IMG_TAKE(file, p + "attn.0", &B.attn[0], "pack_hiera_attn: 3 * heads * 64, 128", LMX_IMG_F16, 2, 3 * H * 64, 128);
      IMG_TAKE(file, p + "attn.1", &B.attn[1], "pack_hiera_attn: 3 * heads * 64", LMX_IMG_F32, 1, 3 * H * 64);
      IMG_TAKE(file, p + "attn.2", &B.attn[2], "pack_hiera_attn: dims, heads * 64", LMX_IMG_F16, 2, D, H * 64);
      IMG_TAKE(file, p + "attn.3", &B.attn[3], "pack_hiera_attn: dims", LMX_IMG_F32, 1, D);
    } else if (B.fused == LMX_HIERA_ATTN4) {
      IMG_TAKE(file, p + "attn.0", &B.attn[0], "pack_hiera_attn4: 4 * heads images of 16384", LMX_IMG_F16, 2, 4 * H, 16384);
      IMG_TAKE(file, p + "attn.1", &B.attn[1], "pack_hiera_attn4: heads * 192 + dims", LMX_IMG_F32, 1, H * 192 + D);
    } else if (B.fused == LMX_HIERA_ATTN_POOL) {
      const bool wide = Din > 128;
      IMG_TAKE(file, p + "attn.0", &B.attn[0], "pack_hiera_attn_pool: 14 (input width 112) or 47 (224) images of 16384", LMX_IMG_F16, 2, wide ? 47 : 14, 16384);
      IMG_TAKE(file, p + "attn.1", &B.attn[1], "pack_hiera_attn_pool: heads * 192 + dims (input width 224) or + 2 * dims (112)", LMX_IMG_F32, 1,
               H * 192 + (wide ? D : 2 * D));
    }
    if (D == 112 || D == 224) {  // FUSED_MLP_WIDTHS
      IMG_TAKE(file, p + "mlp_img.0", &B.mlp_img[0], "pack_ln_mlp: 4 * dims / 64 images of 16384 (dims 112), twice as many (224)", LMX_IMG_F16, 2,
               D == 112 ? 4 * D / 64 : 2 * (4 * D / 64), 16384);
      IMG_TAKE(file, p + "mlp_img.1", &B.mlp_img[1], "pack_ln_mlp: 9 * dims", LMX_IMG_F32, 1, 9 * D);
    }
  }
  for (int s = 2; s < hc.n_stages; ++s) {
    const std::string p = "enc.neck." + std::to_string(s);
    IMG_TAKE(file, p + ".w", &img->neck_w[s], "fpn_dim, dims of the stage", LMX_IMG_F16, 2, hc.fpn_dim, hc.dims[s]);
    IMG_TAKE(file, p + ".b", &img->neck_b[s], "fpn_dim", LMX_IMG_F32, 1, hc.fpn_dim);
  }
  return take_decoder(file, img, 64);
}

}  // namespace

int lmx_sam_image_parse(const char* path, LmxSamImage* img) {
  IMG_REQUIRE(img, "sam image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("sam image", path, LMX_IMAGE_SAM, "SAM", &file)) return rc;
  const std::vector<unsigned char>& cb = file.config;
  const uint32_t fixed = LMX_SAM_CONFIG_INTS * 4 + 8, config_bytes = (uint32_t)cb.size();
  IMG_REQUIRE(config_bytes >= fixed && config_bytes % 8 == 0,
              "sam image: config_bytes %u (a multiple of 8 from %u: %d integers, eps, then the global-attention layer indices)", config_bytes, fixed,
              (int)LMX_SAM_CONFIG_INTS);
  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  LmxSamCfg& c = img->cfg;
  c.encoder = rd<int32_t>(cb.data());
  if (c.encoder == LMX_SAM_ENC_HIERA) return parse_hiera(file, img);
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
  return take_decoder(file, img, g);
}

extern "C" int lmx_sam_image_check_host(const char* path_host, lmx_sam_info_t* info_host) {
  LmxSamImage img;
  if (const int rc = lmx_sam_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_sam_fill_info(img.cfg, 0, info_host);
  return LMX_OK;
}
