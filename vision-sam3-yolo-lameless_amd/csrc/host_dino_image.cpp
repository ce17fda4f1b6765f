// host_dino_image.cpp — reader of the DINO weight image (dino_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_dino_image writes it).  HOST code without HIP: the container reader (host_image.cpp) checks the header and the
// directory against the file's real size, this file checks the config block and asks for every tensor the configuration calls for.
// Everything a model handle later allocates or indexes by (dino_model.hip) comes out of here validated; a malformed file is
// LMX_EINVAL with the field named.
#include <math.h>

#include "dino_image.h"

namespace {

int check_config(const LmxDinoCfg& c) {
  IMG_REQUIRE(c.arch == LMX_DINO_V2 || c.arch == LMX_DINO_V3, "dino image: arch %d is neither dinov2 (0) nor dinov3 (1)", c.arch);
  IMG_REQUIRE(c.hidden > 0 && c.hidden <= 16384 && c.hidden % 8 == 0, "dino image: hidden %d (a multiple of 8 up to 16384)", c.hidden);
  IMG_REQUIRE(c.heads > 0 && c.hidden % c.heads == 0, "dino image: hidden %d is not a multiple of heads %d", c.hidden, c.heads);
  const int hd = c.hidden / c.heads;
  IMG_REQUIRE(hd % 8 == 0 && hd <= 96,
              "dino image: head dim %d (hidden %d / heads %d) is not supported: the attention kernels serve multiples of 8 up to 96", hd,
              c.hidden, c.heads);
  IMG_REQUIRE(c.layers > 0 && c.layers <= 1024, "dino image: layers %d", c.layers);
  IMG_REQUIRE(c.gated == 0 || c.gated == 1, "dino image: gated %d is not a flag", c.gated);
  IMG_REQUIRE(c.mlp > 0 && c.mlp <= 65536 && c.mlp % (c.gated ? 16 : 8) == 0, "dino image: mlp %d (a multiple of %d up to 65536)", c.mlp,
              c.gated ? 16 : 8);
  IMG_REQUIRE(c.patch > 0 && c.patch <= 64, "dino image: patch %d", c.patch);
  IMG_REQUIRE(c.image >= c.patch && c.image <= 8192, "dino image: image %d with patch %d", c.image, c.patch);
  IMG_REQUIRE(c.grid == c.image / c.patch, "dino image: grid %d is not image %d / patch %d", c.grid, c.image, c.patch);
  IMG_REQUIRE(c.n_prefix >= 1 && c.n_prefix <= 256, "dino image: n_prefix %d", c.n_prefix);
  IMG_REQUIRE(c.tokens == c.n_prefix + c.grid * c.grid, "dino image: tokens %d is not n_prefix %d + grid %d squared", c.tokens, c.n_prefix,
              c.grid);
  IMG_REQUIRE(c.k_pad == (c.patch * c.patch * 3 + 7) / 8 * 8, "dino image: k_pad %d is not 3 * patch^2 = %d rounded up to 8", c.k_pad,
              c.patch * c.patch * 3);
  IMG_REQUIRE((c.has_pos == 0 || c.has_pos == 1) && (c.has_rope == 0 || c.has_rope == 1), "dino image: has_pos %d / has_rope %d are not flags",
              c.has_pos, c.has_rope);
  IMG_REQUIRE(c.recipe_kind == LMX_RECIPE_PIL || c.recipe_kind == LMX_RECIPE_FLOAT, "dino image: recipe_kind %d is neither pil (0) nor float (1)",
              c.recipe_kind);
  // the float recipe's tables have one row per pixel of the network's input, and the kernel writes whole patches
  IMG_REQUIRE(c.recipe_kind != LMX_RECIPE_FLOAT || c.grid * c.patch == c.image, "dino image: image %d is not a multiple of patch %d (float recipe)",
              c.image, c.patch);
  IMG_REQUIRE(c.filt == LMX_FILT_BILINEAR || c.filt == LMX_FILT_BICUBIC, "dino image: filt %d is neither bilinear (2) nor bicubic (3)", c.filt);
  IMG_REQUIRE(c.shortest_edge >= 0 && c.size_h >= 0 && c.size_w >= 0 && c.crop >= 0 && c.shortest_edge <= 65536 && c.size_h <= 65536 &&
                  c.size_w <= 65536,
              "dino image: shortest_edge %d / size %d x %d / crop %d", c.shortest_edge, c.size_h, c.size_w, c.crop);
  IMG_REQUIRE((c.size_h > 0) == (c.size_w > 0) && (c.shortest_edge > 0) != (c.size_h > 0),
              "dino image: the recipe needs either shortest_edge (%d) or size_h x size_w (%d x %d)", c.shortest_edge, c.size_h, c.size_w);
  IMG_REQUIRE(c.crop > 0 || c.size_h > 0, "dino image: crop 0 needs size_h x size_w");
  IMG_REQUIRE((c.crop > 0 ? c.crop : c.size_h) == c.image, "dino image: the recipe feeds %d (crop %d, size_h %d), the config block's image is %d",
              c.crop > 0 ? c.crop : c.size_h, c.crop, c.size_h, c.image);
  IMG_REQUIRE(isfinite(c.eps) && c.eps > 0.0, "dino image: eps %g", c.eps);
  IMG_REQUIRE(isfinite(c.rescale) && c.rescale != 0.0, "dino image: rescale %g", c.rescale);
  for (int i = 0; i < 3; ++i)
    IMG_REQUIRE(isfinite(c.mean[i]) && isfinite(c.std[i]) && (float)c.std[i] != 0.f, "dino image: mean / std of channel %d: %g / %g", i, c.mean[i],
                c.std[i]);
  return LMX_OK;
}

}  // namespace

int lmx_dino_image_parse(const char* path, LmxDinoImage* img) {
  IMG_REQUIRE(img, "dino image: null argument");
  LmxImageFile file;
  if (const int rc = lmx_image_open("dino image", path, LMX_IMAGE_DINO, "DINO", &file)) return rc;
  IMG_REQUIRE(file.config.size() == LMX_DINO_CONFIG_BYTES, "dino image: config_bytes %u, a DINO config block has %d", (unsigned)file.config.size(),
              (int)LMX_DINO_CONFIG_BYTES);
  const unsigned char* raw = file.config.data();
  LmxDinoCfg& c = img->cfg;
  int32_t* ints[20] = {&c.arch,  &c.hidden,  &c.heads,   &c.layers,      &c.mlp,  &c.gated,         &c.patch,  &c.image,  &c.grid, &c.n_prefix,
                       &c.tokens, &c.k_pad, &c.has_pos, &c.has_rope, &c.recipe_kind, &c.filt, &c.shortest_edge, &c.size_h, &c.size_w, &c.crop};
  for (int i = 0; i < 20; ++i) *ints[i] = rd<int32_t>(raw + 4 * i);
  double* dbl[8] = {&c.eps, &c.rescale, &c.mean[0], &c.mean[1], &c.mean[2], &c.std[0], &c.std[1], &c.std[2]};
  for (int i = 0; i < 8; ++i) *dbl[i] = rd<double>(raw + 80 + 8 * i);
  if (const int rc = check_config(c)) return rc;

  const int D = c.hidden, I = c.mlp, hd = c.hidden / c.heads, np = c.grid * c.grid, I1 = c.gated ? 2 * I : I;
  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  IMG_TAKE(file, "pe_w", &img->pe_w, "hidden, k_pad", LMX_IMG_F16, 2, D, c.k_pad);
  IMG_TAKE(file, "pe_b", &img->pe_b, "hidden", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "prefix", &img->prefix, "n_prefix, hidden", LMX_IMG_F32, 2, c.n_prefix, D);
  img->pos = img->rope_cos = img->rope_sin = LmxTensorRef();
  if (c.has_pos) IMG_TAKE(file, "pos", &img->pos, "tokens, hidden", LMX_IMG_F32, 2, c.tokens, D);
  if (c.has_rope) {
    IMG_TAKE(file, "rope_cos", &img->rope_cos, "grid^2, hidden / heads", LMX_IMG_F32, 2, np, hd);
    IMG_TAKE(file, "rope_sin", &img->rope_sin, "grid^2, hidden / heads", LMX_IMG_F32, 2, np, hd);
  }
  img->layers.assign((size_t)c.layers, LmxDinoLayerRefs());
  for (int i = 0; i < c.layers; ++i) {
    LmxDinoLayerRefs& L = img->layers[(size_t)i];
    const std::string p = "layer." + std::to_string(i) + ".";
    IMG_TAKE(file, p + "g1", &L.g1, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "b1", &L.b1, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "wqkv", &L.wqkv, "3 hidden, hidden", LMX_IMG_F16, 2, 3 * D, D);
    IMG_TAKE(file, p + "bqkv", &L.bqkv, "3 hidden", LMX_IMG_F32, 1, 3 * D);
    IMG_TAKE(file, p + "wo", &L.wo, "hidden, hidden", LMX_IMG_F16, 2, D, D);
    IMG_TAKE(file, p + "bo", &L.bo, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "ls1", &L.ls1, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "g2", &L.g2, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "b2", &L.b2, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "w1", &L.w1, "mlp (x 2 if gated), hidden", LMX_IMG_F16, 2, I1, D);
    IMG_TAKE(file, p + "bb1", &L.bb1, "mlp (x 2 if gated)", LMX_IMG_F32, 1, I1);
    IMG_TAKE(file, p + "w2", &L.w2, "hidden, mlp", LMX_IMG_F16, 2, D, I);
    IMG_TAKE(file, p + "bb2", &L.bb2, "hidden", LMX_IMG_F32, 1, D);
    IMG_TAKE(file, p + "ls2", &L.ls2, "hidden", LMX_IMG_F32, 1, D);
  }
  IMG_TAKE(file, "gf", &img->gf, "hidden", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "bf", &img->bf, "hidden", LMX_IMG_F32, 1, D);
  IMG_TAKE(file, "lut", &img->lut, "3 x 256", LMX_IMG_F32, 2, 3, 256);
  return LMX_OK;
}

int lmx_dino_resized(const LmxDinoCfg& c, int h, int w, int* nh, int* nw) {
  IMG_REQUIRE(h > 0 && w > 0 && h <= 65536 && w <= 65536, "lmx_dino: frame size %d x %d", h, w);
  if (c.size_h > 0) {
    *nh = c.size_h;
    *nw = c.size_w;
  } else {
    // transformers get_resize_output_image_size(default_to_square=False): int(edge * long / short), a true division in double
    const int sh = w <= h ? w : h, lg = w <= h ? h : w;
    if (sh == c.shortest_edge) {
      *nh = h;
      *nw = w;
    } else {
      const int64_t nl = (int64_t)((double)((int64_t)c.shortest_edge * lg) / (double)sh);
      IMG_REQUIRE(nl <= (1 << 20), "lmx_dino: frame %d x %d resizes to a long side of %lld", h, w, (long long)nl);
      *nh = w <= h ? (int)nl : c.shortest_edge;
      *nw = w <= h ? c.shortest_edge : (int)nl;
    }
  }
  IMG_REQUIRE(*nh >= c.image && *nw >= c.image, "lmx_dino: frame %dx%d resizes to %dx%d, smaller than the %d crop", h, w, *nh, *nw, c.image);
  return LMX_OK;
}

void lmx_dino_fill_info(const LmxDinoCfg& c, int max_batch, lmx_dino_info_t* info) {
  info->arch = c.arch;
  info->hidden = c.hidden;
  info->heads = c.heads;
  info->layers = c.layers;
  info->tokens = c.tokens;
  info->image = c.image;
  info->patch = c.patch;
  info->gated = c.gated;
  info->recipe_kind = c.recipe_kind;
  info->max_batch = max_batch;
}

extern "C" int lmx_dino_image_check_host(const char* path_host, lmx_dino_info_t* info_host) {
  LmxDinoImage img;
  if (const int rc = lmx_dino_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_dino_fill_info(img.cfg, 0, info_host);
  return LMX_OK;
}
