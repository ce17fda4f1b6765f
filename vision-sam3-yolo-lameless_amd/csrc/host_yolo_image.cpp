// host_yolo_image.cpp — reader of the YOLO weight image (yolo_image.h has the layout; lmx/native.py write_yolo_image writes it).
// HOST code without HIP.  Like the DINO reader it never trusts a number from the file before it has been checked against the file's
// real size and against the config block, and it derives what the configuration calls for ITSELF: lmx_yolo_layer_table is the twin of
// lmx/yolo.py's layer_table, YoloConfig.ch / depth, Detect's widths c2 / c3 / c4 and their padding.  Everything the model handle later
// allocates or indexes by (yolo_model.hip) comes out of here validated; a malformed file is LMX_EINVAL with the field or tensor named.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <map>
#include <string>

#include "yolo_image.h"

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
const int MAX_CONFIG_BYTES = 1 << 20, MAX_NC = 4096, MAX_IMGSZ = 8192;

// lmx/yolo.py SCALES: depth multiple, width multiple, max channels
bool scale_of(int letter, double* depth, double* width, int* max_ch) {
  switch (letter) {
    case 'n': *depth = 0.33, *width = 0.25, *max_ch = 1024; return true;
    case 's': *depth = 0.33, *width = 0.50, *max_ch = 1024; return true;
    case 'm': *depth = 0.67, *width = 0.75, *max_ch = 768; return true;
    case 'l': *depth = 1.0, *width = 1.0, *max_ch = 512; return true;
    case 'x': *depth = 1.0, *width = 1.25, *max_ch = 512; return true;
  }
  return false;
}

int check_config(const LmxYoloCfg& c) {
  double d, w;
  int mc;
  IMG_REQUIRE(scale_of(c.scale, &d, &w, &mc), "yolo image: scale %d is none of 'n' 's' 'm' 'l' 'x'", c.scale);
  IMG_REQUIRE(c.nc >= 1 && c.nc <= MAX_NC, "yolo image: nc %d outside 1 .. %d", c.nc, MAX_NC);
  IMG_REQUIRE(c.nc_pad == (c.nc + 3) / 4 * 4, "yolo image: nc_pad %d is not nc %d rounded up to 4", c.nc_pad, c.nc);
  IMG_REQUIRE(c.imgsz >= 32 && c.imgsz <= MAX_IMGSZ && c.imgsz % 32 == 0, "yolo image: imgsz %d (a multiple of 32 up to %d)", c.imgsz, MAX_IMGSZ);
  IMG_REQUIRE((c.kpt_k == 0 && c.kpt_ndim == 0) || (c.kpt_k >= 1 && c.kpt_k <= 1024 && (c.kpt_ndim == 2 || c.kpt_ndim == 3)),
              "yolo image: keypoint shape kpt_k %d x kpt_ndim %d (0 x 0, or K x 2 | 3)", c.kpt_k, c.kpt_ndim);
  IMG_REQUIRE(c.nk_pad == (c.kpt_k * c.kpt_ndim + 3) / 4 * 4, "yolo image: nk_pad %d is not kpt_k %d x kpt_ndim %d rounded up to 4", c.nk_pad,
              c.kpt_k, c.kpt_ndim);
  IMG_REQUIRE(c.plans >= 1 && c.plans <= 3, "yolo image: plans mask %d holds no plan (bit 0: f16, bit 1: exact)", c.plans);
  IMG_REQUIRE(c.n_names == c.nc, "yolo image: n_names %d is not nc %d", c.n_names, c.nc);
  IMG_REQUIRE(c.names_bytes >= c.n_names && c.names_bytes <= MAX_CONFIG_BYTES, "yolo image: names_bytes %d for %d names", c.names_bytes, c.n_names);
  return LMX_OK;
}

struct Want {
  uint32_t dtype, rank;
  int32_t shape[4];
};

// the tensor `name` with exactly this dtype and shape, inside the file
int take(const std::map<std::string, Entry>& dir, const std::string& name, const Want& w, uint64_t data_offset, uint64_t file_bytes,
         LmxTensorRef* ref) {
  const auto it = dir.find(name);
  IMG_REQUIRE(it != dir.end(), "yolo image: missing tensor '%s'", name.c_str());
  const Entry& e = it->second;
  IMG_REQUIRE(e.dtype == w.dtype, "yolo image: tensor '%s' has dtype %u, expected %s", name.c_str(), e.dtype, DTYPE_NAME[w.dtype]);
  bool same = e.rank == w.rank;
  for (uint32_t i = 0; same && i < w.rank; ++i) same = e.shape[i] == w.shape[i];
  IMG_REQUIRE(same, "yolo image: tensor '%s' has rank %u shape [%d, %d, %d, %d], the configuration calls for rank %u [%d, %d, %d, %d]", name.c_str(),
              e.rank, e.shape[0], e.shape[1], e.shape[2], e.shape[3], w.rank, w.shape[0], w.shape[1], w.shape[2], w.shape[3]);
  uint64_t bytes = (uint64_t)ELEM[w.dtype];
  for (uint32_t i = 0; i < w.rank; ++i) bytes *= (uint64_t)w.shape[i];  // Cout <= 2^13, K <= 2^17: no overflow
  IMG_REQUIRE(e.nbytes == bytes, "yolo image: tensor '%s' has nbytes %llu, its shape holds %llu", name.c_str(), (unsigned long long)e.nbytes,
              (unsigned long long)bytes);
  IMG_REQUIRE(e.offset % 64 == 0, "yolo image: tensor '%s' has offset %llu, not a multiple of 64", name.c_str(), (unsigned long long)e.offset);
  IMG_REQUIRE(e.offset >= data_offset && e.offset <= file_bytes && e.nbytes <= file_bytes - e.offset,
              "yolo image: tensor '%s' has offset %llu + nbytes %llu outside the data [%llu, %llu) of the file", name.c_str(),
              (unsigned long long)e.offset, (unsigned long long)e.nbytes, (unsigned long long)data_offset, (unsigned long long)file_bytes);
  ref->offset = e.offset;
  ref->nbytes = e.nbytes;
  return LMX_OK;
}

}  // namespace

int lmx_yolo_layer_table(const LmxYoloCfg& c, std::vector<LmxYoloModule>* table, int* c2_out, int* c3_out, int* c4p_out) {
  double depth, width;
  int max_ch;
  IMG_REQUIRE(scale_of(c.scale, &depth, &width, &max_ch), "yolo image: scale %d is none of 'n' 's' 'm' 'l' 'x'", c.scale);
  // YoloConfig.ch: _make_divisible(min(c, max_ch) * width, 8); YoloConfig.depth: max(round(n * depth), 1), Python's round (half to even)
  auto ch = [&](int v) { return (int)(ceil((v < max_ch ? v : max_ch) * width / 8) * 8); };
  auto dp = [&](int n) {
    const int r = (int)nearbyint(n * depth);
    return r > 1 ? r : 1;
  };
  auto conv = [&](int v) { return LmxYoloModule{LMX_YM_CONV, 0, ch(v), 0, 0}; };
  auto c2f = [&](int v, int n, int sc) { return LmxYoloModule{LMX_YM_C2F, 0, ch(v), dp(n), sc}; };
  const LmxYoloModule up{LMX_YM_UP, 0, 0, 0, 0}, cat{LMX_YM_CAT, 0, 0, 0, 0};
  std::vector<LmxYoloModule>& L = *table;
  L = {conv(64), conv(128), c2f(128, 3, 1), conv(256), c2f(256, 6, 1), conv(512), c2f(512, 6, 1), conv(1024), c2f(1024, 3, 1),
       LmxYoloModule{LMX_YM_SPPF, 0, ch(1024), 0, 0}, up, cat, c2f(512, 3, 0), up, cat, c2f(256, 3, 0), conv(256), cat, c2f(512, 3, 0),
       conv(512), cat, c2f(1024, 3, 0), LmxYoloModule{LMX_YM_DETECT, 0, 0, 0, 0}};
  const int cat_src[23] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0, 0, 4, 0, 0, 12, 0, 0, 9, 0, 0};
  int out_c[23];
  for (int i = 0; i < 23; ++i) {
    LmxYoloModule& m = L[(size_t)i];
    if (m.kind == LMX_YM_CONV || m.kind == LMX_YM_C2F || m.kind == LMX_YM_SPPF) {
      m.c1 = i == 0 ? 3 : out_c[i - 1];
      out_c[i] = m.c2;
    } else if (m.kind == LMX_YM_UP) {
      out_c[i] = out_c[i - 1];
    } else if (m.kind == LMX_YM_CAT) {
      out_c[i] = out_c[i - 1] + out_c[cat_src[i]];
    } else {
      out_c[i] = 0;
    }
  }
  const int ch0 = out_c[15], nk = c.kpt_k * c.kpt_ndim;
  int c2 = ch0 / 4 > 16 ? ch0 / 4 : 16;
  if (c2 < 64) c2 = 64;  // max(16, ch[0] // 4, reg_max * 4)
  const int ncm = c.nc < 100 ? c.nc : 100, c3 = ch0 > ncm ? ch0 : ncm;
  const int c4 = nk ? (ch0 / 4 > nk ? ch0 / 4 : nk) : 0;
  IMG_REQUIRE(c3 % 8 == 0, "yolo image: nc %d gives Detect's class branch %d channels, not a multiple of 8 (lmx_k_gemm's K)", c.nc, c3);
  *c2_out = c2;
  *c3_out = c3;
  *c4p_out = (c4 + 7) / 8 * 8;
  return LMX_OK;
}

const LmxYoloConv* lmx_yolo_find_conv(const LmxYoloImage& img, const std::string& name) {
  for (const LmxYoloConv& c : img.convs)
    if (c.name == name) return &c;
  return nullptr;
}

void lmx_yolo_fill_info(const LmxYoloCfg& c, int max_batch, lmx_yolo_info_t* info) {
  info->scale = c.scale;
  info->nc = c.nc;
  info->imgsz = c.imgsz;
  info->kpt_k = c.kpt_k;
  info->kpt_ndim = c.kpt_ndim;
  info->plans = c.plans;
  info->max_batch = max_batch;
}

int lmx_yolo_image_parse(const char* path, LmxYoloImage* img) {
  IMG_REQUIRE(path && img, "yolo image: null argument");
  File fh;
  fh.f = fopen(path, "rb");
  IMG_REQUIRE(fh.f, "yolo image: cannot open '%s'", path);
  struct stat st;
  IMG_REQUIRE(fstat(fileno(fh.f), &st) == 0 && S_ISREG(st.st_mode), "yolo image: '%s' is not a regular file", path);
  const uint64_t real = (uint64_t)st.st_size;
  unsigned char hb[LMX_IMAGE_HEADER_BYTES];
  IMG_REQUIRE(real >= sizeof(hb) && fread(hb, 1, sizeof(hb), fh.f) == sizeof(hb),
              "yolo image: header: the file has %llu bytes, the header alone %d (truncated?)", (unsigned long long)real, (int)sizeof(hb));
  IMG_REQUIRE(memcmp(hb, "LMXIMAGE", 8) == 0, "yolo image: magic is not 'LMXIMAGE': not a weight image");
  const uint32_t version = rd<uint32_t>(hb + 8), kind = rd<uint32_t>(hb + 12), config_bytes = rd<uint32_t>(hb + 16);
  const uint32_t n_tensors = rd<uint32_t>(hb + 20);
  const uint64_t dir_offset = rd<uint64_t>(hb + 24), data_offset = rd<uint64_t>(hb + 32), file_bytes = rd<uint64_t>(hb + 40);
  IMG_REQUIRE(version == LMX_IMAGE_VERSION, "yolo image: version %u, this library reads version %u", version, LMX_IMAGE_VERSION);
  IMG_REQUIRE(kind == LMX_IMAGE_YOLO, "yolo image: kind %u is not YOLO (%d)", kind, (int)LMX_IMAGE_YOLO);
  const uint32_t fixed = LMX_YOLO_CONFIG_INTS * 4;
  IMG_REQUIRE(config_bytes >= fixed && config_bytes <= (uint32_t)MAX_CONFIG_BYTES && config_bytes % 8 == 0,
              "yolo image: config_bytes %u (a multiple of 8 from %u: %d integers, then the names blob)", config_bytes, fixed, (int)LMX_YOLO_CONFIG_INTS);
  IMG_REQUIRE(n_tensors >= 1 && n_tensors <= (1u << 20), "yolo image: n_tensors %u", n_tensors);
  const uint64_t cfg_end = LMX_IMAGE_HEADER_BYTES + (uint64_t)config_bytes, dir_bytes = (uint64_t)n_tensors * LMX_IMAGE_ENTRY_BYTES;
  IMG_REQUIRE(real >= cfg_end, "yolo image: header: the file has %llu bytes and ends inside the config block (truncated?)", (unsigned long long)real);
  IMG_REQUIRE(dir_offset >= cfg_end && dir_offset <= real && dir_bytes <= real - dir_offset,
              "yolo image: directory of %u entries at dir_offset %llu does not fit the file's %llu bytes (truncated?)", n_tensors,
              (unsigned long long)dir_offset, (unsigned long long)real);
  IMG_REQUIRE(file_bytes == real, "yolo image: file_bytes says %llu, the file has %llu (truncated?)", (unsigned long long)file_bytes,
              (unsigned long long)real);
  IMG_REQUIRE(data_offset >= dir_offset + dir_bytes && data_offset <= file_bytes && data_offset % 64 == 0,
              "yolo image: data_offset %llu (a multiple of 64 between the directory's end %llu and file_bytes %llu)", (unsigned long long)data_offset,
              (unsigned long long)(dir_offset + dir_bytes), (unsigned long long)file_bytes);

  // the config block: the integers, then the class names
  std::vector<unsigned char> cb(config_bytes);
  IMG_REQUIRE(fread(cb.data(), 1, cb.size(), fh.f) == cb.size(), "yolo image: header: cannot read the config block");
  LmxYoloCfg& c = img->cfg;
  int32_t* ints[LMX_YOLO_CONFIG_INTS] = {&c.scale, &c.nc, &c.nc_pad, &c.imgsz, &c.kpt_k, &c.kpt_ndim, &c.nk_pad, &c.plans, &c.n_names, &c.names_bytes};
  for (int i = 0; i < LMX_YOLO_CONFIG_INTS; ++i) *ints[i] = rd<int32_t>(cb.data() + 4 * i);
  if (const int rc = check_config(c)) return rc;
  IMG_REQUIRE((uint32_t)((c.names_bytes + 7) / 8 * 8) == config_bytes - fixed,
              "yolo image: names_bytes %d (padded to 8) does not fill the %u bytes the config block has behind its integers", c.names_bytes,
              config_bytes - fixed);
  const unsigned char* blob = cb.data() + fixed;
  IMG_REQUIRE(blob[c.names_bytes - 1] == 0, "yolo image: names blob: the last name has no NUL terminator");
  img->names.clear();
  for (int at = 0; at < c.names_bytes;) {
    const size_t len = strlen(reinterpret_cast<const char*>(blob + at));  // terminated: the blob's last byte is NUL
    img->names.emplace_back(reinterpret_cast<const char*>(blob + at), len);
    at += (int)len + 1;
  }
  IMG_REQUIRE((int)img->names.size() == c.n_names, "yolo image: names blob holds %d NUL-terminated names, n_names says %d", (int)img->names.size(),
              c.n_names);
  for (uint32_t at = fixed + (uint32_t)c.names_bytes; at < config_bytes; ++at)
    IMG_REQUIRE(cb[at] == 0, "yolo image: names blob: the padding behind names_bytes %d is not zero", c.names_bytes);
  if (const int rc = lmx_yolo_layer_table(c, &img->table, &img->c2, &img->c3, &img->c4p)) return rc;

  // the directory: names -> entries (an entry the reader does not know is ignored)
  IMG_REQUIRE(fseeko(fh.f, (off_t)dir_offset, SEEK_SET) == 0, "yolo image: directory: cannot seek to dir_offset %llu", (unsigned long long)dir_offset);
  std::map<std::string, Entry> dir;
  for (uint32_t i = 0; i < n_tensors; ++i) {
    unsigned char eb[LMX_IMAGE_ENTRY_BYTES];
    IMG_REQUIRE(fread(eb, 1, sizeof(eb), fh.f) == sizeof(eb), "yolo image: directory: cannot read entry %u", i);
    IMG_REQUIRE(memchr(eb, 0, LMX_IMAGE_NAME_BYTES) != nullptr && eb[0] != 0, "yolo image: directory entry %u has no NUL-terminated name", i);
    Entry e;
    e.dtype = rd<uint32_t>(eb + 48);
    e.rank = rd<uint32_t>(eb + 52);
    for (int k = 0; k < 4; ++k) e.shape[k] = rd<int32_t>(eb + 56 + 4 * k);
    e.offset = rd<uint64_t>(eb + 72);
    e.nbytes = rd<uint64_t>(eb + 80);
    const std::string name(reinterpret_cast<const char*>(eb));
    IMG_REQUIRE(e.dtype <= LMX_IMG_I32 && e.rank >= 1 && e.rank <= 4, "yolo image: tensor '%s' has dtype %u rank %u", name.c_str(), e.dtype, e.rank);
    IMG_REQUIRE(dir.emplace(name, e).second, "yolo image: tensor '%s' is listed twice", name.c_str());
  }

  // the convolutions the layer table calls for, in YoloDetector.w's order
  img->data_offset = data_offset;
  img->file_bytes = file_bytes;
  img->convs.clear();
  auto add = [&](const std::string& name, int k, int cout, int cin) {
    LmxYoloConv cv;
    cv.name = name;
    cv.k = k;
    cv.cout = cout;
    cv.cin = cin;
    img->convs.push_back(cv);
  };
  const std::vector<LmxYoloModule>& T = img->table;
  for (int i = 1; i < 23; ++i) {
    const LmxYoloModule& m = T[(size_t)i];
    const std::string p = "model." + std::to_string(i);
    if (m.kind == LMX_YM_CONV) {
      add(p, 3, m.c2, m.c1);
    } else if (m.kind == LMX_YM_C2F) {
      const int ch = m.c2 / 2;
      add(p + ".cv1", 1, 2 * ch, m.c1);
      add(p + ".cv2", 1, m.c2, (2 + m.n) * ch);
      for (int j = 0; j < m.n; ++j) {
        add(p + ".m." + std::to_string(j) + ".cv1", 3, ch, ch);
        add(p + ".m." + std::to_string(j) + ".cv2", 3, ch, ch);
      }
    } else if (m.kind == LMX_YM_SPPF) {
      add(p + ".cv1", 1, m.c1 / 2, m.c1);
      add(p + ".cv2", 1, m.c2, m.c1 / 2 * 4);
    } else if (m.kind == LMX_YM_DETECT) {
      const int feat[3] = {T[15].c2, T[18].c2, T[21].c2};
      for (int l = 0; l < 3; ++l) {
        const std::string s = "." + std::to_string(l);
        add(p + ".cv2" + s + ".0", 3, img->c2, feat[l]);
        add(p + ".cv2" + s + ".1", 3, img->c2, img->c2);
        add(p + ".cv2" + s + ".2", 1, 64, img->c2);
        add(p + ".cv3" + s + ".0", 3, img->c3, feat[l]);
        add(p + ".cv3" + s + ".1", 3, img->c3, img->c3);
        add(p + ".cv3" + s + ".2", 1, c.nc_pad, img->c3);
      }
      if (c.kpt_k)
        for (int l = 0; l < 3; ++l) {
          const std::string s = "." + std::to_string(l);
          add(p + ".cv4" + s + ".0", 3, img->c4p, feat[l]);
          add(p + ".cv4" + s + ".1", 3, img->c4p, img->c4p);
          add(p + ".cv4" + s + ".2", 1, c.nk_pad, img->c4p);
        }
    }
  }
#define TAKE(name, ref, dt, rank, s0, s1, s2, s3)                                                                 \
  do {                                                                                                            \
    const Want w_ = {dt, rank, {s0, s1, s2, s3}};                                                                 \
    if (const int rc_ = take(dir, name, w_, data_offset, file_bytes, ref)) return rc_;                            \
  } while (0)
  TAKE("stem.w", &img->stem_w, LMX_IMG_F32, 4, 3, 3, 3, T[0].c2);
  TAKE("stem.b", &img->stem_b, LMX_IMG_F32, 1, T[0].c2, 0, 0, 0);
  for (LmxYoloConv& cv : img->convs) {
    const int K = cv.k * cv.k * cv.cin;
    if (c.plans & (1 << LMX_YOLO_F16)) {
      TAKE("f16." + cv.name + ".w", &cv.w, LMX_IMG_F16, 2, cv.cout, K, 0, 0);
      TAKE("f16." + cv.name + ".b", &cv.b, LMX_IMG_F32, 1, cv.cout, 0, 0, 0);
    }
    if (c.plans & (1 << LMX_YOLO_EXACT)) {
      TAKE("x3." + cv.name + ".w", &cv.xw, LMX_IMG_F16, 2, cv.cout, 3 * K, 0, 0);
      TAKE("x3." + cv.name + ".b", &cv.xb, LMX_IMG_F32, 1, cv.cout, 0, 0, 0);
      TAKE("x3." + cv.name + ".s", &cv.xs, LMX_IMG_F32, 1, cv.cout, 0, 0, 0);
    }
  }
#undef TAKE
  return LMX_OK;
}

extern "C" int lmx_yolo_image_check_host(const char* path_host, lmx_yolo_info_t* info_host) {
  LmxYoloImage img;
  if (const int rc = lmx_yolo_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_yolo_fill_info(img.cfg, 0, info_host);
  return LMX_OK;
}
