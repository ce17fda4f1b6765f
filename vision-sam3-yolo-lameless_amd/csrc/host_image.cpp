// host_image.cpp — reader of the weight-image container (image.h has the layout; lmx/native.py write_image writes it).
// HOST code without HIP, shared by every model's reader: it parses and validates the header and the tensor directory, hands the config
// block's bytes to the model, and never trusts a number from the file before it has been checked against the file's real size.
// lmx_image_take is the one place a tensor's dtype, shape, size, alignment and position are checked; a malformed file is LMX_EINVAL
// with the field or tensor named.
#include <stdio.h>
#include <sys/stat.h>

#include "image.h"

namespace {

struct File {
  FILE* f = nullptr;
  ~File() {
    if (f) fclose(f);
  }
};

const int ELEM[3] = {2, 4, 4};  // LMX_IMG_F16, LMX_IMG_F32, LMX_IMG_I32
const char* const DTYPE_NAME[3] = {"f16", "f32", "i32"};

std::string shape_text(const int32_t* shape, uint32_t rank) {
  std::string s = "[";
  for (uint32_t i = 0; i < rank && i < 4; ++i) s += (i ? ", " : "") + std::to_string(shape[i]);
  return s + "]";
}

}  // namespace

int lmx_image_open(const char* who, const char* path, uint32_t want_kind, const char* kind_name, LmxImageFile* img) {
  IMG_REQUIRE(path && img, "%s: null argument", who);
  img->who = who;
  File fh;
  fh.f = fopen(path, "rb");
  IMG_REQUIRE(fh.f, "%s: cannot open '%s'", who, path);
  struct stat st;
  IMG_REQUIRE(fstat(fileno(fh.f), &st) == 0 && S_ISREG(st.st_mode), "%s: '%s' is not a regular file", who, path);
  const uint64_t real = (uint64_t)st.st_size;
  unsigned char hb[LMX_IMAGE_HEADER_BYTES];
  IMG_REQUIRE(real >= sizeof(hb) && fread(hb, 1, sizeof(hb), fh.f) == sizeof(hb),
              "%s: header: the file has %llu bytes, the header alone %d (truncated?)", who, (unsigned long long)real, (int)sizeof(hb));
  IMG_REQUIRE(memcmp(hb, "LMXIMAGE", 8) == 0, "%s: magic is not 'LMXIMAGE': not a weight image", who);
  const uint32_t version = rd<uint32_t>(hb + 8), kind = rd<uint32_t>(hb + 12), config_bytes = rd<uint32_t>(hb + 16);
  const uint32_t n_tensors = rd<uint32_t>(hb + 20);
  const uint64_t dir_offset = rd<uint64_t>(hb + 24), data_offset = rd<uint64_t>(hb + 32), file_bytes = rd<uint64_t>(hb + 40);
  IMG_REQUIRE(version == LMX_IMAGE_VERSION, "%s: version %u, this library reads version %u", who, version, LMX_IMAGE_VERSION);
  IMG_REQUIRE(kind == want_kind, "%s: kind %u is not %s (%u)", who, kind, kind_name, want_kind);
  IMG_REQUIRE(config_bytes <= (uint32_t)LMX_IMAGE_MAX_CONFIG_BYTES, "%s: config_bytes %u, a config block has at most %d", who, config_bytes,
              (int)LMX_IMAGE_MAX_CONFIG_BYTES);
  IMG_REQUIRE(n_tensors >= 1 && n_tensors <= (1u << 20), "%s: n_tensors %u", who, n_tensors);
  const uint64_t cfg_end = LMX_IMAGE_HEADER_BYTES + (uint64_t)config_bytes, dir_bytes = (uint64_t)n_tensors * LMX_IMAGE_ENTRY_BYTES;
  IMG_REQUIRE(real >= cfg_end, "%s: header: the file has %llu bytes and ends inside the config block (truncated?)", who, (unsigned long long)real);
  IMG_REQUIRE(dir_offset >= cfg_end && dir_offset <= real && dir_bytes <= real - dir_offset,
              "%s: directory of %u entries at dir_offset %llu does not fit the file's %llu bytes (truncated?)", who, n_tensors,
              (unsigned long long)dir_offset, (unsigned long long)real);
  IMG_REQUIRE(file_bytes == real, "%s: file_bytes says %llu, the file has %llu (truncated?)", who, (unsigned long long)file_bytes,
              (unsigned long long)real);
  IMG_REQUIRE(data_offset >= dir_offset + dir_bytes && data_offset <= file_bytes && data_offset % 64 == 0,
              "%s: data_offset %llu (a multiple of 64 between the directory's end %llu and file_bytes %llu)", who, (unsigned long long)data_offset,
              (unsigned long long)(dir_offset + dir_bytes), (unsigned long long)file_bytes);
  img->data_offset = data_offset;
  img->file_bytes = file_bytes;

  img->config.resize(config_bytes);
  IMG_REQUIRE(fread(img->config.data(), 1, config_bytes, fh.f) == config_bytes, "%s: header: cannot read the config block", who);

  IMG_REQUIRE(fseeko(fh.f, (off_t)dir_offset, SEEK_SET) == 0, "%s: directory: cannot seek to dir_offset %llu", who, (unsigned long long)dir_offset);
  img->dir.clear();
  for (uint32_t i = 0; i < n_tensors; ++i) {
    unsigned char eb[LMX_IMAGE_ENTRY_BYTES];
    IMG_REQUIRE(fread(eb, 1, sizeof(eb), fh.f) == sizeof(eb), "%s: directory: cannot read entry %u", who, i);
    IMG_REQUIRE(memchr(eb, 0, LMX_IMAGE_NAME_BYTES) != nullptr && eb[0] != 0, "%s: directory entry %u has no NUL-terminated name", who, i);
    LmxImageEntry e;
    e.dtype = rd<uint32_t>(eb + 48);
    e.rank = rd<uint32_t>(eb + 52);
    for (int k = 0; k < 4; ++k) e.shape[k] = rd<int32_t>(eb + 56 + 4 * k);
    e.offset = rd<uint64_t>(eb + 72);
    e.nbytes = rd<uint64_t>(eb + 80);
    const std::string name(reinterpret_cast<const char*>(eb));
    IMG_REQUIRE(e.dtype <= LMX_IMG_I32 && e.rank >= 1 && e.rank <= 4, "%s: tensor '%s' has dtype %u rank %u", who, name.c_str(), e.dtype, e.rank);
    IMG_REQUIRE(img->dir.emplace(name, e).second, "%s: tensor '%s' is listed twice", who, name.c_str());
  }
  return LMX_OK;
}

int lmx_image_take(const LmxImageFile& img, const std::string& name, const LmxImageWant& w, LmxTensorRef* ref) {
  const char* who = img.who;
  const auto it = img.dir.find(name);
  IMG_REQUIRE(it != img.dir.end(), "%s: missing tensor '%s'", who, name.c_str());
  const LmxImageEntry& e = it->second;
  IMG_REQUIRE(e.dtype == w.dtype, "%s: tensor '%s' has dtype %u, expected %s", who, name.c_str(), e.dtype, DTYPE_NAME[w.dtype]);
  bool same = e.rank == w.rank;
  for (uint32_t i = 0; same && i < w.rank; ++i) same = e.shape[i] == w.shape[i];
  IMG_REQUIRE(same, "%s: tensor '%s' has rank %u shape %s, the config block (%s) says rank %u %s", who, name.c_str(), e.rank,
              shape_text(e.shape, e.rank).c_str(), w.field, w.rank, shape_text(w.shape, w.rank).c_str());
  uint64_t bytes = (uint64_t)ELEM[w.dtype];
  for (uint32_t i = 0; i < w.rank; ++i) bytes *= (uint64_t)w.shape[i];  // each model bounds its config numbers: far below 2^64
  IMG_REQUIRE(e.nbytes == bytes, "%s: tensor '%s' has nbytes %llu, its shape holds %llu", who, name.c_str(), (unsigned long long)e.nbytes,
              (unsigned long long)bytes);
  IMG_REQUIRE(e.offset % 64 == 0, "%s: tensor '%s' has offset %llu, not a multiple of 64", who, name.c_str(), (unsigned long long)e.offset);
  IMG_REQUIRE(e.offset >= img.data_offset && e.offset <= img.file_bytes && e.nbytes <= img.file_bytes - e.offset,
              "%s: tensor '%s' has offset %llu + nbytes %llu outside the data [%llu, %llu) of the file", who, name.c_str(),
              (unsigned long long)e.offset, (unsigned long long)e.nbytes, (unsigned long long)img.data_offset, (unsigned long long)img.file_bytes);
  ref->offset = e.offset;
  ref->nbytes = e.nbytes;
  return LMX_OK;
}
