// host_yolo_image.cpp — reader of the YOLO weight image (yolo_image.h has the config block and the tensors; image.h the container;
// lmx/native.py write_yolo_image writes it).  HOST code without HIP.  The container reader (host_image.cpp) checks the header and the
// directory against the file's real size; this file checks the config block and derives what the configuration calls for ITSELF:
// lmx_yolo_layer_table is the twin of lmx/yolo.py's layer_table, YoloConfig.ch / depth, Detect's widths c2 / c3 / c4 and their padding.
// Everything the model handle later allocates or indexes by (yolo_model.hip) comes out of here validated; a malformed file is
// LMX_EINVAL with the field or tensor named.
#include <math.h>

#include "yolo_image.h"

namespace {

const int MAX_NC = 4096, MAX_IMGSZ = 8192;

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
  IMG_REQUIRE(c.names_bytes >= c.n_names && c.names_bytes <= LMX_IMAGE_MAX_CONFIG_BYTES, "yolo image: names_bytes %d for %d names", c.names_bytes, c.n_names);
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
  IMG_REQUIRE(img, "yolo image: null argument");
  LmxImageFile file;
  const uint32_t fixed = LMX_YOLO_CONFIG_INTS * 4;
  if (const int rc = lmx_image_open("yolo image", path, LMX_IMAGE_YOLO, "YOLO", &file)) return rc;
  // the config block: the integers, then the class names
  const std::vector<unsigned char>& cb = file.config;
  const uint32_t config_bytes = (uint32_t)cb.size();
  IMG_REQUIRE(config_bytes >= fixed && config_bytes % 8 == 0, "yolo image: config_bytes %u (a multiple of 8 from %u: %d integers, then the names blob)",
              config_bytes, fixed, (int)LMX_YOLO_CONFIG_INTS);
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

  // the convolutions the layer table calls for, in YoloDetector.w's order
  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
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
  IMG_TAKE(file, "stem.w", &img->stem_w, "3, 3, 3, C0", LMX_IMG_F32, 4, 3, 3, 3, T[0].c2);
  IMG_TAKE(file, "stem.b", &img->stem_b, "C0", LMX_IMG_F32, 1, T[0].c2);
  for (LmxYoloConv& cv : img->convs) {
    const int K = cv.k * cv.k * cv.cin;
    if (c.plans & (1 << LMX_YOLO_F16)) {
      IMG_TAKE(file, "f16." + cv.name + ".w", &cv.w, "Cout, k*k*Cin", LMX_IMG_F16, 2, cv.cout, K);
      IMG_TAKE(file, "f16." + cv.name + ".b", &cv.b, "Cout", LMX_IMG_F32, 1, cv.cout);
    }
    if (c.plans & (1 << LMX_YOLO_EXACT)) {
      IMG_TAKE(file, "x3." + cv.name + ".w", &cv.xw, "Cout, 3*k*k*Cin", LMX_IMG_F16, 2, cv.cout, 3 * K);
      IMG_TAKE(file, "x3." + cv.name + ".b", &cv.xb, "Cout", LMX_IMG_F32, 1, cv.cout);
      IMG_TAKE(file, "x3." + cv.name + ".s", &cv.xs, "Cout", LMX_IMG_F32, 1, cv.cout);
    }
  }
  return LMX_OK;
}

extern "C" int lmx_yolo_image_check_host(const char* path_host, lmx_yolo_info_t* info_host) {
  LmxYoloImage img;
  if (const int rc = lmx_yolo_image_parse(path_host, &img)) return rc;
  if (info_host) lmx_yolo_fill_info(img.cfg, 0, info_host);
  return LMX_OK;
}
