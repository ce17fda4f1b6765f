// records.hip — the per-frame record matrix of the multi-GPU gather (lmx/dist.py pack_records) in ONE launch.
// Byte work, bound by HBM: the record of a 1080p frame is ~270 KB, nearly all of it mask bits, so the figure of merit is bytes
// moved / time, as for the kernels of pre.hip and sam.hip.
//
// The kernel is a gather over the DESTINATION: the output is walked as one flat run of 8-byte words (the stride and every field offset
// are multiples of 8, so a word lies in one row and belongs to one field, to the `valid` word or to nothing), a thread owns the two
// words of one 16-byte block of the output's address space, finds each word's field in a table that travels in the kernel arguments,
// reads the source bytes and stores the block once.  Every output byte is stored exactly once — field bytes, the zeros behind a
// field's last byte, rows a map leaves out and padding rows alike — so nothing has to clear `out` first and nothing races.
// Loads: 16 bytes where the block lies inside one field row and the source address is 16-byte aligned (lane i at base + 16 i: the
// widest coalesced form), 8 bytes where a whole word is 8-byte aligned, else the word at its own unaligned address, and single bytes
// for a field row's ragged tail (never a byte behind the source's end).  Stores: one 16-byte store per block; the 8-byte store only at
// the two ends of an output that starts or ends on an odd word.
#include <string.h>

#include "common.h"

namespace {

// the field table as kernel arguments.  Indexed with compile-time constants only (the unrolled scans below): a table indexed by a
// lane's own field number would be copied to scratch memory first.
struct RecTable {
  const uint8_t* src[LMX_RECORD_MAX_FIELDS];
  int64_t row_bytes[LMX_RECORD_MAX_FIELDS], offset[LMX_RECORD_MAX_FIELDS];
  int32_t map[LMX_RECORD_MAX_FIELDS], n_src[LMX_RECORD_MAX_FIELDS];
  const int32_t* maps[LMX_RECORD_MAX_MAPS];
  int n_fields;
};

// where output word (row r, byte column col) comes from: p = its first source byte and nb = 1 .. 8 bytes to take, or nb = 0: zeros
struct Word {
  const uint8_t* p;
  int nb;
};

__device__ __forceinline__ Word find_word(const RecTable& T, int64_t r, int64_t col, int64_t n_valid) {
  if (r >= n_valid) return Word{nullptr, 0};  // a padding row: zeros, and no map is read for it
  // fields ascend: the last one that starts at or before col
  const uint8_t* src = nullptr;
  int64_t rb = 0, off = 0;
  int map = -1, n_src = 0;
#pragma unroll
  for (int f = 0; f < LMX_RECORD_MAX_FIELDS; ++f)
    if (f < T.n_fields && col >= T.offset[f]) {
      src = T.src[f];
      rb = T.row_bytes[f];
      off = T.offset[f];
      map = T.map[f];
      n_src = T.n_src[f];
    }
  const int64_t at = col - off;  // byte of the field's row
  if (src == nullptr || at >= rb) return Word{nullptr, 0};
  int64_t s = r;
  if (map >= 0) {
    const int32_t* m = T.maps[0];
#pragma unroll
    for (int k = 1; k < LMX_RECORD_MAX_MAPS; ++k)
      if (map == k) m = T.maps[k];
    s = m[r];
  }
  if (s < 0 || s >= n_src) return Word{nullptr, 0};
  const int64_t left = rb - at;
  return Word{src + s * rb + at, left < 8 ? (int)left : 8};
}

__device__ __forceinline__ u32x2 load_word(const Word& w) {
  u32x2 v = {0u, 0u};
  if (w.nb == 8) {
    if ((reinterpret_cast<uintptr_t>(w.p) & 7) == 0)
      v = *reinterpret_cast<const u32x2*>(w.p);
    else
      __builtin_memcpy(&v, w.p, 8);  // the word at its own address
  } else {
    uint64_t x = 0;
    for (int i = 0; i < w.nb; ++i) x |= (uint64_t)w.p[i] << (8 * i);
    v[0] = (unsigned)x;
    v[1] = (unsigned)(x >> 32);
  }
  return v;
}

// thread = one 16-byte block of the output's address space = words 2 b - lead and 2 b - lead + 1 of the flat output (lead = 1: `out`
// starts on the second word of a block).  wps: words per row.
__global__ __launch_bounds__(256) void pack_records_kernel(RecTable T, int64_t n_valid, int64_t wps, int64_t n_words, int lead, int narrow,
                                                           uint8_t* __restrict__ out) {
  const int64_t blocks = (n_words + lead + 1) / 2;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w0 = 2 * b - lead;
    const bool has0 = w0 >= 0, has1 = w0 + 1 < n_words;
    const int64_t wa = has0 ? w0 : 0;  // the first word this thread owns
    int64_t r0, c0;
    if (narrow) {  // the word count fits 31 bits: a 32-bit division
      r0 = (unsigned)wa / (unsigned)wps;
      c0 = (unsigned)wa - (unsigned)r0 * (unsigned)wps;
    } else {
      r0 = wa / wps;
      c0 = wa - r0 * wps;
    }
    // the second word: the next one of the row, or the first of the next row
    int64_t r1 = r0, c1 = c0 + 1;
    if (c1 == wps) r1 = r0 + 1, c1 = 0;
    if (!has0) r1 = r0, c1 = c0;  // (wa is this thread's only word, handled as the second one)
    u32x2 v0 = {0u, 0u}, v1 = {0u, 0u};
    Word a = {nullptr, 0}, c = {nullptr, 0};
    if (has0) {
      if (c0 == 0)
        v0[0] = r0 < n_valid ? 1u : 0u;
      else
        a = find_word(T, r0, c0 * 8, n_valid);
    }
    if (has1) {
      if (c1 == 0)
        v1[0] = r1 < n_valid ? 1u : 0u;
      else
        c = find_word(T, r1, c1 * 8, n_valid);
    }
    if (a.nb == 8 && c.nb == 8 && c.p == a.p + 8 && (reinterpret_cast<uintptr_t>(a.p) & 15) == 0) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(a.p);
      v0[0] = v[0], v0[1] = v[1], v1[0] = v[2], v1[1] = v[3];
    } else {
      if (a.nb) v0 = load_word(a);
      if (c.nb) v1 = load_word(c);
    }
    uint8_t* d = out + w0 * 8;
    if (has0 && has1) {
      u32x4 v;
      v[0] = v0[0], v[1] = v0[1], v[2] = v1[0], v[3] = v1[1];
      *reinterpret_cast<u32x4*>(d) = v;
    } else if (has0) {
      *reinterpret_cast<u32x2*>(d) = v0;
    } else if (has1) {
      *reinterpret_cast<u32x2*>(d + 8) = v1;
    }
  }
}

}  // namespace

extern "C" int lmx_k_pack_records(const lmx_record_field_t* fields_host, int n_fields, const int32_t* const* row_maps_host, int n_maps,
                                  int64_t n_valid, int64_t n_rows, int64_t stride, uint8_t* out, lmx_stream_t stream) {
  LMX_REQUIRE(n_fields >= 0 && n_fields <= LMX_RECORD_MAX_FIELDS, "lmx_k_pack_records: n_fields %d outside 0 .. %d", n_fields, LMX_RECORD_MAX_FIELDS);
  LMX_REQUIRE(n_maps >= 0 && n_maps <= LMX_RECORD_MAX_MAPS, "lmx_k_pack_records: n_maps %d outside 0 .. %d", n_maps, LMX_RECORD_MAX_MAPS);
  LMX_REQUIRE(n_fields == 0 || fields_host != nullptr, "lmx_k_pack_records: null pointer (fields_host)");
  LMX_REQUIRE(n_maps == 0 || row_maps_host != nullptr, "lmx_k_pack_records: null pointer (row_maps_host)");
  LMX_REQUIRE(n_rows >= 0 && n_valid >= 0 && n_valid <= n_rows, "lmx_k_pack_records: n_valid %lld outside 0 .. n_rows = %lld", (long long)n_valid,
              (long long)n_rows);
  LMX_REQUIRE(stride >= 8 && stride % 8 == 0, "lmx_k_pack_records: stride %lld is no multiple of 8 from 8 on", (long long)stride);
  LMX_REQUIRE(n_rows <= INT64_MAX / stride, "lmx_k_pack_records: %lld rows of %lld bytes", (long long)n_rows, (long long)stride);
  RecTable T;
  memset(&T, 0, sizeof(T));
  T.n_fields = n_fields;
  int64_t end = 8;  // where the previous field ended
  for (int f = 0; f < n_fields; ++f) {
    const lmx_record_field_t& F = fields_host[f];
    LMX_REQUIRE(F.row_bytes > 0, "lmx_k_pack_records: field %d has row_bytes %lld", f, (long long)F.row_bytes);
    LMX_REQUIRE(F.offset % 8 == 0 && F.offset >= end, "lmx_k_pack_records: field %d at offset %lld: offsets are multiples of 8 and ascend (the bytes before %lld are taken)",
                f, (long long)F.offset, (long long)end);
    LMX_REQUIRE(F.row_bytes <= stride - F.offset, "lmx_k_pack_records: field %d ends at byte %lld of a %lld-byte row", f, (long long)(F.offset + F.row_bytes),
                (long long)stride);
    LMX_REQUIRE(F.map >= -1 && F.map < n_maps, "lmx_k_pack_records: field %d follows map %d of %d", f, F.map, n_maps);
    LMX_REQUIRE(F.n_src >= 0 && (F.n_src == 0 || F.src != nullptr), "lmx_k_pack_records: field %d has %d source rows at %p", f, F.n_src, F.src);
    T.src[f] = static_cast<const uint8_t*>(F.src);
    T.row_bytes[f] = F.row_bytes;
    T.offset[f] = F.offset;
    T.map[f] = F.map;
    T.n_src[f] = F.src ? F.n_src : 0;
    end = F.offset + F.row_bytes;
  }
  for (int k = 0; k < n_maps; ++k) {
    LMX_REQUIRE(row_maps_host[k] != nullptr || n_rows == 0, "lmx_k_pack_records: null pointer (row map %d)", k);
    T.maps[k] = row_maps_host[k];
  }
  if (n_rows == 0) return LMX_OK;
  LMX_REQUIRE(out != nullptr && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "lmx_k_pack_records: out %p is null or not 8-byte aligned", (void*)out);
  const int64_t wps = stride / 8, n_words = n_rows * wps;
  const int lead = (int)((reinterpret_cast<uintptr_t>(out) >> 3) & 1);
  const int64_t blocks = (n_words + lead + 1) / 2;
  int64_t grid = (blocks + 255) / 256;
  if (grid > 256 * 8) grid = 256 * 8;
  hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), T, n_valid, wps, n_words, lead,
                     n_words < 0x7fffffffll ? 1 : 0, out);
  return lmx_launch_check("pack_records_kernel");
}
