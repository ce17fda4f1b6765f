// weights_table.h — the weight table of the four sequence and graph models (TCN, gait transformer, graph transformer, GraphGPS), stated
// ONCE per model: which tensors a configuration calls for, under which names, with which shapes, and which pointer of
// lmx_<model>_weights_t each one fills.  A model states its table as lmx_<model>_tensor_rows (host_<model>.cpp, next to its
// check_config); what reads an image, binds the weights to a copy of its data, or tells Python the table (lmx_h_<model>_tensors) is
// written here once, over the rows.  Host code only: nothing here needs HIP.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <initializer_list>

#include "image.h"

struct LmxTensorRow {  // one tensor a configuration calls for
  std::string name;    // its name in the weight image and in pack_tensors ("layer.3.qkv.w", "block.2.res.b", "vu1_w")
  const char* field;   // the config numbers its shape comes from: the text lmx_image_take puts in a mismatch message
  int rank;
  int32_t shape[4];    // unused dimensions 0
  size_t at;           // offsetof the const float* inside lmx_<model>_weights_t that takes it (array fields: + index * sizeof(float*))
};

inline void lmx_row(std::vector<LmxTensorRow>* rows, const std::string& name, const char* field, size_t at, std::initializer_list<int32_t> shape) {
  LmxTensorRow r = {name, field, (int)shape.size(), {0, 0, 0, 0}, at};
  int i = 0;
  for (const int32_t d : shape) r.shape[i++] = d;
  rows->push_back(r);
}
// one row inside a table function (`rows` in scope): the tensor `name` fills `member` of the weights struct W, element `index` of it
// where the member is an array of pointers
#define LMX_ROW(W, member, index, name, field, ...) \
  lmx_row(rows, name, field, offsetof(W, member) + (size_t)(index) * sizeof(const float*), {__VA_ARGS__})

// a model's table function: appends every tensor `cfg` calls for; `cfg` has passed lmx_<model>_check_config(.., false)
template <class Weights>
using LmxTensorRowsFn = void (*)(const Weights& cfg, std::vector<LmxTensorRow>* rows);

// A parsed weight image of one of the four models: LmxTcnImage, LmxXfmImage, LmxGfmImage and LmxGnnImage are this.
template <class Weights>
struct LmxTableImage {
  Weights cfg = {};  // the integers; its pointers stay null until lmx_table_bind
  double p = 0.0;    // the dropout probability
  uint64_t data_offset = 0, file_bytes = 0;
  std::vector<LmxTensorRow> rows;  // what cfg calls for
  std::vector<LmxTensorRef> refs;  // where the file has it, row for row
};

// The tail of a model's image reader, after it has decoded and checked the config block into img->cfg and img->p: every tensor of the
// table with exactly its shape, as f32.  LMX_EINVAL with the tensor and `field` named.
template <class Weights>
int lmx_table_take(const LmxImageFile& file, LmxTensorRowsFn<Weights> tensor_rows, LmxTableImage<Weights>* img) {
  img->data_offset = file.data_offset;
  img->file_bytes = file.file_bytes;
  img->rows.clear();
  tensor_rows(img->cfg, &img->rows);
  img->refs.assign(img->rows.size(), LmxTensorRef());
  for (size_t i = 0; i < img->rows.size(); ++i) {
    const LmxTensorRow& r = img->rows[i];
    const LmxImageWant want = {r.field, LMX_IMG_F32, (uint32_t)r.rank, {r.shape[0], r.shape[1], r.shape[2], r.shape[3]}};
    if (const int rc = lmx_image_take(file, r.name, want, &img->refs[i])) return rc;
  }
  return LMX_OK;
}

// the weights with every pointer into `data`, a copy of the image's data section [data_offset, file_bytes) in host or device memory;
// a pointer no row names stays null
template <class Weights>
void lmx_table_bind(const LmxTableImage<Weights>& img, const char* data, Weights* w) {
  *w = img.cfg;
  for (size_t i = 0; i < img.rows.size(); ++i)
    *reinterpret_cast<const float**>(reinterpret_cast<char*>(w) + img.rows[i].at) =
        reinterpret_cast<const float*>(data + (img.refs[i].offset - img.data_offset));
}

// lmx_h_<model>_tensors (include/lmx.h): the configuration checked as the forwards check it, then its rows in the public form
template <class Weights>
int lmx_table_export(const char* fn, const char* who, const Weights* cfg, int (*check_config)(const char*, const Weights*, bool),
                     LmxTensorRowsFn<Weights> tensor_rows, lmx_tensor_row_t* out, int cap, int* n) {
  IMG_REQUIRE(who && n, "%s: null who or n_host", fn);
  *n = 0;
  if (const int rc = check_config(who, cfg, false)) return rc;
  std::vector<LmxTensorRow> rows;
  tensor_rows(*cfg, &rows);
  *n = (int)rows.size();
  if (!out && cap == 0) return LMX_OK;
  IMG_REQUIRE(out, "%s: rows_host is null with cap %d", who, cap);
  IMG_REQUIRE(cap >= *n, "%s: cap %d is below the %d tensors the configuration calls for", who, cap, *n);
  memset(out, 0, rows.size() * sizeof(*out));
  for (size_t i = 0; i < rows.size(); ++i) {
    snprintf(out[i].name, sizeof(out[i].name), "%s", rows[i].name.c_str());
    out[i].rank = rows[i].rank;
    memcpy(out[i].shape, rows[i].shape, sizeof(out[i].shape));
    out[i].pointer_at = (int64_t)rows[i].at;
  }
  return LMX_OK;
}
