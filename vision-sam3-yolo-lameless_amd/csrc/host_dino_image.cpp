// host_dino_image.cpp — reader of the DINO weight image (dino_image.h has the layout; lmx/native.py write_dino_image writes it).
// HOST code without HIP: it parses and validates the header, the config block and the tensor directory, and never trusts a number
// from the file before it has been checked against the file's real size and against the config block.  Everything a model handle
// later allocates or indexes by (dino_model.hip) comes out of here validated; a malformed file is LMX_EINVAL with the field named.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <map>
#include <string>

#include "dino_image.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define IMG_REQUIRE(cond, ...)    \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

namespace {

struct Entry {
  uint32_t dtype, rank;
  int32_t shape[4];
  uint64_t offset, nbytes;
};

struct File {
  FILE* f = nullptr;
  ~File() {
    if (f) fclose(f);
  }
};

template <class T>
T rd(const unsigned char* p) {  // the image is little-endian, and so is every host this library is built for
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

const int ELEM[3] = {2, 4, 4};  // LMX_IMG_F16, LMX_IMG_F32, LMX_IMG_I32
const char* const DTYPE_NAME[3] = {"f16", "f32", "i32"};

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

struct Want {
  const char* field;  // the config numbers the shape comes from (named in the message)
  uint32_t dtype, rank;
  int32_t shape[2];
};

// the tensor `name` with exactly this dtype and shape, inside the file
int take(const std::map<std::string, Entry>& dir, const std::string& name, const Want& w, uint64_t data_offset, uint64_t file_bytes,
         LmxTensorRef* ref) {
  const auto it = dir.find(name);
  IMG_REQUIRE(it != dir.end(), "dino image: missing tensor '%s'", name.c_str());
  const Entry& e = it->second;
  IMG_REQUIRE(e.dtype == w.dtype, "dino image: tensor '%s' has dtype %u, expected %s", name.c_str(), e.dtype, DTYPE_NAME[w.dtype]);
  bool same = e.rank == w.rank;
  for (uint32_t i = 0; same && i < w.rank; ++i) same = e.shape[i] == w.shape[i];
  IMG_REQUIRE(same, "dino image: tensor '%s' has rank %u shape [%d, %d], the config block (%s) says rank %u [%d, %d]", name.c_str(), e.rank,
              e.shape[0], e.rank > 1 ? e.shape[1] : 1, w.field, w.rank, w.shape[0], w.rank > 1 ? w.shape[1] : 1);
  uint64_t bytes = (uint64_t)ELEM[w.dtype];
  for (uint32_t i = 0; i < w.rank; ++i) bytes *= (uint64_t)w.shape[i];  // each factor <= 2^18: no overflow
  IMG_REQUIRE(e.nbytes == bytes, "dino image: tensor '%s' has nbytes %llu, its shape holds %llu", name.c_str(), (unsigned long long)e.nbytes,
              (unsigned long long)bytes);
  IMG_REQUIRE(e.offset % 64 == 0, "dino image: tensor '%s' has offset %llu, not a multiple of 64", name.c_str(), (unsigned long long)e.offset);
  IMG_REQUIRE(e.offset >= data_offset && e.offset <= file_bytes && e.nbytes <= file_bytes - e.offset,
              "dino image: tensor '%s' has offset %llu + nbytes %llu outside the data [%llu, %llu) of the file", name.c_str(),
              (unsigned long long)e.offset, (unsigned long long)e.nbytes, (unsigned long long)data_offset, (unsigned long long)file_bytes);
  ref->offset = e.offset;
  ref->nbytes = e.nbytes;
  return LMX_OK;
}

}  // namespace

int lmx_dino_image_parse(const char* path, LmxDinoImage* img) {
  IMG_REQUIRE(path && img, "dino image: null argument");
  File fh;
  fh.f = fopen(path, "rb");
  IMG_REQUIRE(fh.f, "dino image: cannot open '%s'", path);
  struct stat st;
  IMG_REQUIRE(fstat(fileno(fh.f), &st) == 0 && S_ISREG(st.st_mode), "dino image: '%s' is not a regular file", path);
  const uint64_t real = (uint64_t)st.st_size;
  unsigned char hb[LMX_IMAGE_HEADER_BYTES];
  IMG_REQUIRE(real >= sizeof(hb) && fread(hb, 1, sizeof(hb), fh.f) == sizeof(hb),
              "dino image: header: the file has %llu bytes, the header alone %d (truncated?)", (unsigned long long)real, (int)sizeof(hb));
  IMG_REQUIRE(memcmp(hb, "LMXIMAGE", 8) == 0, "dino image: magic is not 'LMXIMAGE': not a weight image");
  const uint32_t version = rd<uint32_t>(hb + 8), kind = rd<uint32_t>(hb + 12), config_bytes = rd<uint32_t>(hb + 16);
  const uint32_t n_tensors = rd<uint32_t>(hb + 20);
  const uint64_t dir_offset = rd<uint64_t>(hb + 24), data_offset = rd<uint64_t>(hb + 32), file_bytes = rd<uint64_t>(hb + 40);
  IMG_REQUIRE(version == LMX_IMAGE_VERSION, "dino image: version %u, this library reads version %u", version, LMX_IMAGE_VERSION);
  IMG_REQUIRE(kind == LMX_IMAGE_DINO, "dino image: kind %u is not DINO (%d)", kind, (int)LMX_IMAGE_DINO);
  IMG_REQUIRE(config_bytes == LMX_DINO_CONFIG_BYTES, "dino image: config_bytes %u, a DINO config block has %d", config_bytes,
              (int)LMX_DINO_CONFIG_BYTES);
  IMG_REQUIRE(n_tensors >= 1 && n_tensors <= (1u << 20), "dino image: n_tensors %u", n_tensors);
  const uint64_t cfg_end = LMX_IMAGE_HEADER_BYTES + (uint64_t)config_bytes, dir_bytes = (uint64_t)n_tensors * LMX_IMAGE_ENTRY_BYTES;
  IMG_REQUIRE(real >= cfg_end, "dino image: header: the file has %llu bytes and ends inside the config block (truncated?)", (unsigned long long)real);
  IMG_REQUIRE(dir_offset >= cfg_end && dir_offset <= real && dir_bytes <= real - dir_offset,
              "dino image: directory of %u entries at dir_offset %llu does not fit the file's %llu bytes (truncated?)", n_tensors,
              (unsigned long long)dir_offset, (unsigned long long)real);
  IMG_REQUIRE(file_bytes == real, "dino image: file_bytes says %llu, the file has %llu (truncated?)", (unsigned long long)file_bytes,
              (unsigned long long)real);
  IMG_REQUIRE(data_offset >= dir_offset + dir_bytes && data_offset <= file_bytes && data_offset % 64 == 0,
              "dino image: data_offset %llu (a multiple of 64 between the directory's end %llu and file_bytes %llu)", (unsigned long long)data_offset,
              (unsigned long long)(dir_offset + dir_bytes), (unsigned long long)file_bytes);

  unsigned char cb[LMX_DINO_CONFIG_BYTES];
  IMG_REQUIRE(fread(cb, 1, sizeof(cb), fh.f) == sizeof(cb), "dino image: header: cannot read the config block");
  LmxDinoCfg& c = img->cfg;
  int32_t* ints[20] = {&c.arch,  &c.hidden,  &c.heads,   &c.layers,      &c.mlp,  &c.gated,         &c.patch,  &c.image,  &c.grid, &c.n_prefix,
                       &c.tokens, &c.k_pad, &c.has_pos, &c.has_rope, &c.recipe_kind, &c.filt, &c.shortest_edge, &c.size_h, &c.size_w, &c.crop};
  for (int i = 0; i < 20; ++i) *ints[i] = rd<int32_t>(cb + 4 * i);
  double* dbl[8] = {&c.eps, &c.rescale, &c.mean[0], &c.mean[1], &c.mean[2], &c.std[0], &c.std[1], &c.std[2]};
  for (int i = 0; i < 8; ++i) *dbl[i] = rd<double>(cb + 80 + 8 * i);
  if (const int rc = check_config(c)) return rc;

  // the directory: names -> entries (an entry the reader does not know is ignored)
  IMG_REQUIRE(fseeko(fh.f, (off_t)dir_offset, SEEK_SET) == 0, "dino image: directory: cannot seek to dir_offset %llu", (unsigned long long)dir_offset);
  std::map<std::string, Entry> dir;
  for (uint32_t i = 0; i < n_tensors; ++i) {
    unsigned char eb[LMX_IMAGE_ENTRY_BYTES];
    IMG_REQUIRE(fread(eb, 1, sizeof(eb), fh.f) == sizeof(eb), "dino image: directory: cannot read entry %u", i);
    IMG_REQUIRE(memchr(eb, 0, LMX_IMAGE_NAME_BYTES) != nullptr && eb[0] != 0, "dino image: directory entry %u has no NUL-terminated name", i);
    Entry e;
    e.dtype = rd<uint32_t>(eb + 48);
    e.rank = rd<uint32_t>(eb + 52);
    for (int k = 0; k < 4; ++k) e.shape[k] = rd<int32_t>(eb + 56 + 4 * k);
    e.offset = rd<uint64_t>(eb + 72);
    e.nbytes = rd<uint64_t>(eb + 80);
    const std::string name(reinterpret_cast<const char*>(eb));
    IMG_REQUIRE(e.dtype <= LMX_IMG_I32 && e.rank >= 1 && e.rank <= 4, "dino image: tensor '%s' has dtype %u rank %u", name.c_str(), e.dtype, e.rank);
    IMG_REQUIRE(dir.emplace(name, e).second, "dino image: tensor '%s' is listed twice", name.c_str());
  }

  const int D = c.hidden, I = c.mlp, hd = c.hidden / c.heads, np = c.grid * c.grid, I1 = c.gated ? 2 * I : I;
  img->data_offset = data_offset;
  img->file_bytes = file_bytes;
#define TAKE(name, ref, field, dt, rank, s0, s1)                                                               \
  do {                                                                                                         \
    const Want w_ = {field, dt, rank, {s0, s1}};                                                               \
    if (const int rc_ = take(dir, name, w_, data_offset, file_bytes, ref)) return rc_;                         \
  } while (0)
  TAKE("pe_w", &img->pe_w, "hidden, k_pad", LMX_IMG_F16, 2, D, c.k_pad);
  TAKE("pe_b", &img->pe_b, "hidden", LMX_IMG_F32, 1, D, 1);
  TAKE("prefix", &img->prefix, "n_prefix, hidden", LMX_IMG_F32, 2, c.n_prefix, D);
  img->pos = img->rope_cos = img->rope_sin = LmxTensorRef();
  if (c.has_pos) TAKE("pos", &img->pos, "tokens, hidden", LMX_IMG_F32, 2, c.tokens, D);
  if (c.has_rope) {
    TAKE("rope_cos", &img->rope_cos, "grid^2, hidden / heads", LMX_IMG_F32, 2, np, hd);
    TAKE("rope_sin", &img->rope_sin, "grid^2, hidden / heads", LMX_IMG_F32, 2, np, hd);
  }
  img->layers.assign((size_t)c.layers, LmxDinoLayerRefs());
  for (int i = 0; i < c.layers; ++i) {
    LmxDinoLayerRefs& L = img->layers[(size_t)i];
    const std::string p = "layer." + std::to_string(i) + ".";
    TAKE(p + "g1", &L.g1, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "b1", &L.b1, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "wqkv", &L.wqkv, "3 hidden, hidden", LMX_IMG_F16, 2, 3 * D, D);
    TAKE(p + "bqkv", &L.bqkv, "3 hidden", LMX_IMG_F32, 1, 3 * D, 1);
    TAKE(p + "wo", &L.wo, "hidden, hidden", LMX_IMG_F16, 2, D, D);
    TAKE(p + "bo", &L.bo, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "ls1", &L.ls1, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "g2", &L.g2, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "b2", &L.b2, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "w1", &L.w1, "mlp (x 2 if gated), hidden", LMX_IMG_F16, 2, I1, D);
    TAKE(p + "bb1", &L.bb1, "mlp (x 2 if gated)", LMX_IMG_F32, 1, I1, 1);
    TAKE(p + "w2", &L.w2, "hidden, mlp", LMX_IMG_F16, 2, D, I);
    TAKE(p + "bb2", &L.bb2, "hidden", LMX_IMG_F32, 1, D, 1);
    TAKE(p + "ls2", &L.ls2, "hidden", LMX_IMG_F32, 1, D, 1);
  }
  TAKE("gf", &img->gf, "hidden", LMX_IMG_F32, 1, D, 1);
  TAKE("bf", &img->bf, "hidden", LMX_IMG_F32, 1, D, 1);
  TAKE("lut", &img->lut, "3 x 256", LMX_IMG_F32, 2, 3, 256);
#undef TAKE
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
