// sam_image.h — the weight image of SAM v1 (ViT image encoder + prompt encoder + mask decoder; written by lmx/native.py write_sam_image,
// read by host_sam_image.cpp) as the model handle (sam_model.hip) sees it.  Host code only: nothing here needs HIP.
//
// The container is image.h's (header, config block, directory of 88-byte entries, 64-byte aligned data, version 1), kind SAM:
//   config  at 48      12 x i32 (LmxSamCfg's integers in declaration order; `encoder` is LMX_SAM_ENC_VIT — LMX_SAM_ENC_HIERA has the
//                      block described further down, any other value is refused), f64 eps, then
//                      n_global x i32 global-attention layer indices (ascending), zero-padded to a multiple of 8 bytes
//   tensors            each bit for bit what SamVitEncoder / MaskDecoder hold on the device (D = hidden, I = mlp, g = image / patch,
//                      Kp = 3 * patch^2, hd = D / heads, S = g for a global layer and `window` otherwise, C = out_ch = 256):
//     encoder, both plans   enc.pe_b f32 [D], enc.pos f32 [g*g][D], enc.lut f32 [3][256], enc.n1.g / enc.n1.b / enc.n2.g / enc.n2.b f32 [C];
//                           per layer i: enc.L<i>.g1 .b1 .g2 .b2 .bo .bb2 f32 [D], .bqkv f32 [3D], .bb1 f32 [I], .padkv f16 [3D],
//                           .rh .rw f32 [2S-1][hd]
//     encoder, plan f16     enc.pe_w f16 [D][Kp], enc.n1.w f16 [C][D], enc.n2.w f16 [C][9C]; enc.L<i>.wqkv f16 [3D][D], .wo f16 [D][D],
//                           .w1 f16 [I][D], .w2 f16 [D][I]
//     encoder, plan exact   the [whi | wlo] form of the same weights (SamVitEncoder._split2): enc.x2.pe f16 [D][2Kp], enc.x2.n1 f16
//                           [C][2D], enc.x2.n2.hi / enc.x2.n2.lo f16 [C][9C]; enc.x2.L<i>.qkv f16 [3D][2D], .proj f16 [D][2D],
//                           .fc1 f16 [I][2D], .fc2 f16 [D][2I]
//     decoder, both plans   dec.gauss f32 [2][128], dec.corner f32 [2][256], dec.key_pe f32 [g*g][256], dec.no_mask f32 [1][256],
//                           dec.out_tokens f32 [5][256]; the LayerNorms dec.L<i>.ln1 .. ln4, dec.ln_final (.g / .b f32 [256]) and
//                           dec.up_ln (.g / .b f32 [64])
//     decoder Linears       for each `lin` of lmx_sam_linears() (N x K):  plan f16: dec.f16.<lin>.w f16 [N][K], .b f32 [N];
//                           plan exact: dec.x3.<lin>.w f16 [N][3K] = [whi | whi / 2048 | wlo], .b f32 [N] (shifted), .s f32 [N] (scale)
//   (an entry the reader does not ask for — the point prompts' embeddings, the mask-input parameters — is ignored)
//
// An image whose encoder is Hiera (lmx.sam.HieraEncoder; `encoder` = LMX_SAM_ENC_HIERA) has its own config block behind that field
// and its own encoder tensors; the decoder part is the one above (g = 64: the reader refuses a configuration whose embedding is not
// [64][64][256]), and `plans` names the DECODER plans the image holds — the Hiera trunk has one plan, f16 operands.
//   config  at 48      12 x i32: encoder, hidden, n_stages, n_blocks (the sum of blocks[]), n_global, n_top_down, q_pool_stages, image,
//                      fpn_dim, plans, pos_bkg[0], pos_bkg[1]; f64 eps; then i32 blocks[n_stages], dims[n_stages], heads[n_stages],
//                      windows[n_stages], global_blocks[n_global] (ascending), fpn_top_down[n_top_down], zero-padded to a multiple of
//                      8 bytes: everything lmx.sam.HieraConfig has (lmx_hiera_config_t, include/lmx.h)
//   tensors            each bit for bit what a loaded HieraEncoder holds (g4 = image / 4; per block i of HieraConfig.block_plan():
//                      Din -> D, `heads`; no packing or swizzling is restated in C++):
//     enc.pe_w f16 [hidden][152], enc.pe_b f32 [hidden], enc.pos f32 [g4*g4][hidden] (the windowed position table), enc.lut f32 [3][256]
//     enc.B<i>.g1 .b1 f32 [Din]; .wqkv f16 [3D][Din], .bqkv f32 [3D], .padkv f16 [3D]; .wo f16 [D][D], .bo f32 [D]; .g2 .b2 f32 [D];
//              .w1 f16 [4D][D], .bb1 f32 [4D], .w2 f16 [D][4D], .bb2 f32 [D]; where Din != D: .wp f16 [D][Din], .bp f32 [D]
//     enc.B<i>.attn.<j>   the packed operands of a block of a fused class (lmx_hiera_fused_attn, hiera_config.h):
//              attn8      (pack_hiera_attn)       .0 f16 [3*heads*64][128], .1 f32 [3*heads*64], .2 f16 [D][heads*64], .3 f32 [D]
//              attn4      (pack_hiera_attn4)      .0 f16 [4*heads][16384], .1 f32 [heads*192 + D]
//              attn_pool  (pack_hiera_attn_pool)  .0 f16 [14][16384], .1 f32 [2D + heads*192] (Din 112);  [47][16384], [D + heads*192] (Din 224)
//     enc.B<i>.mlp_img.0 f16 [4D/64 (D 112) | 2*4D/64 (D 224)][16384], .1 f32 [9D]   (pack_ln_mlp) where D is 112 or 224
//     enc.neck.<s>.w f16 [fpn_dim][dims[s]], .b f32 [fpn_dim] for the levels s = 2 .. n_stages - 1 that outputs="embedding" reads
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "hiera_config.h"
#include "image.h"

enum { LMX_SAM_CONFIG_INTS = 12 };
enum { LMX_SAM_DEC_D = 256, LMX_SAM_DEC_HEADS = 8, LMX_SAM_DEC_MLP = 2048, LMX_SAM_OUT_TOKENS = 5 };

struct LmxSamCfg {
  // LMX_SAM_ENC_VIT, or LMX_SAM_ENC_HIERA: `hiera` is the configuration, and the fields below are what lmx_sam_info_t documents for
  // it (hidden = dims[0], heads = heads[0], layers = the number of blocks, mlp = 0, window = windows[0], patch = 16, out_ch = fpn_dim)
  int32_t encoder;
  int32_t hidden, heads, layers, mlp, window, patch, image, out_ch;
  int32_t plans;  // bit (1 << LMX_SAM_F16) | bit (1 << LMX_SAM_EXACT)
  int32_t n_global, reserved;
  double eps;
  std::vector<int32_t> global_idx;
  lmx_hiera_config_t hiera;
  int grid() const { return image / patch; }
  bool is_global(int layer) const {
    for (int32_t g : global_idx)
      if (g == layer) return true;
    return false;
  }
};

struct LmxSamLayerRefs {
  LmxTensorRef g1, b1, bqkv, padkv, rh, rw, bo, g2, b2, bb1, bb2;  // both plans
  LmxTensorRef wqkv, wo, w1, w2;                                   // plan f16
  LmxTensorRef xqkv, xproj, xfc1, xfc2;                            // plan exact: [whi | wlo]
};

// one Linear of the mask decoder: its short name and its dimensions
struct LmxSamLinear {
  std::string name;
  int N = 0, K = 0;
  LmxTensorRef w, b;        // plan f16
  LmxTensorRef xw, xb, xs;  // plan exact
};

struct LmxSamNorm {
  LmxTensorRef g, b;
};

// one block of the Hiera trunk; fused: lmx_hiera_fused_attn's class, whose packed operands are attn[0 ..]
struct LmxHieraBlockRefs {
  LmxHieraBlock shape;
  int fused = 0;
  LmxTensorRef g1, b1, wqkv, bqkv, padkv, wo, bo, g2, b2, w1, bb1, w2, bb2, wp, bp, attn[4], mlp_img[2];
};

struct LmxSamImage {
  LmxSamCfg cfg;
  std::vector<LmxHieraBlockRefs> hiera_blocks;                                // encoder Hiera
  LmxTensorRef neck_w[LMX_HIERA_MAX_STAGES], neck_b[LMX_HIERA_MAX_STAGES];  // ... levels 2 .. n_stages - 1
  uint64_t data_offset = 0, file_bytes = 0;
  LmxTensorRef pe_w, pe_b, pos, lut, n1_w, n1_g, n1_b, n2_w, n2_g, n2_b, x_pe, x_n1, x_n2_hi, x_n2_lo;
  std::vector<LmxSamLayerRefs> layers;
  LmxTensorRef gauss, corner, key_pe, no_mask, out_tokens;
  LmxSamNorm dec_ln[2][4], ln_final, up_ln;
  std::vector<LmxSamLinear> linears;  // in lmx_sam_linears()'s order
};

// the Linears the box-prompt decoder with one mask touches, in launch order of first use: L<i>.sa.{q,k,v,o}, L<i>.t2i.*, L<i>.lin1,
// L<i>.lin2, L<i>.i2t.* for i = 0, 1; fin.*; up1; up2; hyp0.{in,mid,out}; iou.{in,mid,out}
std::vector<LmxSamLinear> lmx_sam_linears();
// ResizeLongestSide.get_preprocess_shape: int(x * scale + 0.5) with scale = image / max(h, w) in double
void lmx_sam_resized_hw(int image, int h, int w, int* nh, int* nw);
// Parse and validate the header, the config block and the directory of `path` (the tensor data is not read).  LMX_EINVAL with the
// offending field or tensor named in lmx_last_error; `img` is complete only on LMX_OK.
int lmx_sam_image_parse(const char* path, LmxSamImage* img);
void lmx_sam_fill_info(const LmxSamCfg& c, int max_batch, lmx_sam_info_t* info);
