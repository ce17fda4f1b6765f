// fused_check_main.cpp — the host arithmetic of the fused record (csrc/host_records.cpp: lmx_h_record_layout, lmx_h_stream_plan,
// lmx_h_row_map) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and swept
// (tests/test_fused_sanitized.py).
//   fused_check_main QUERIES    QUERIES: a text file, one query per line, integers separated by blanks:
//     0 h w hidden max_det scheduled        lmx_h_record_layout
//     1 n_chunks max_streams layout         lmx_h_stream_plan
//     2 n n_idx idx[n_idx]                  lmx_h_row_map (the list is named "det_idx")
//   one line of output per query: "<return code>\t<error text>\t<the results, blank separated>":
//     layout: stride, then name dtype ndim shape0 shape1 offset nbytes per field; plan: pool det emb, then the stream of each pass;
//     row map: the n map entries, then the n flags.
// The arrays handed to the library are heap blocks of exactly the entries it is told about, so that a write past the last one is a report.
// The functions report through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/lmx.h"

static char g_error[512];  // the size of the library's buffer: a long message is cut at the same place

void lmx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s QUERIES\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    fprintf(stderr, "%s: cannot read %s\n", argv[0], argv[1]);
    return 2;
  }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<long> v;
    for (long x; ss >> x;) v.push_back(x);
    size_t at = 0;
    auto next = [&]() -> int { return at < v.size() ? (int)v[at++] : 0; };
    const int kind = next();
    g_error[0] = 0;
    if (kind == 0) {
      const int h = next(), w = next(), hidden = next(), max_det = next(), scheduled = next();
      std::vector<lmx_record_layout_t> lay(1);
      const int rc = lmx_h_record_layout(h, w, hidden, max_det, scheduled, lay.data());
      printf("%d\t%s\t", rc, g_error);
      if (rc == LMX_OK) {
        printf("%lld", (long long)lay[0].stride);
        for (int i = 0; i < lay[0].n_fields; ++i) {
          const lmx_record_field_layout_t& f = lay[0].fields[i];
          printf(" %s %d %d %lld %lld %lld %lld", f.name, f.dtype, f.ndim, (long long)f.shape[0], (long long)f.shape[1], (long long)f.offset,
                 (long long)f.nbytes);
        }
      }
    } else if (kind == 1) {
      const int n_chunks = next(), max_streams = next(), layout = next();
      std::vector<int32_t> sam((size_t)(n_chunks > 0 ? n_chunks : 0));
      int pool = 0, det = 0, emb = 0;
      const int rc = lmx_h_stream_plan(n_chunks, max_streams, layout, &pool, &det, &emb, sam.empty() ? nullptr : sam.data());
      printf("%d\t%s\t", rc, g_error);
      if (rc == LMX_OK) {
        printf("%d %d %d", pool, det, emb);
        for (int32_t s : sam) printf(" %d", (int)s);
      }
    } else if (kind == 2) {
      const int n = next(), n_idx = next();
      std::vector<int32_t> idx((size_t)(n_idx > 0 ? n_idx : 0)), map((size_t)(n > 0 ? n : 0)), ran(map.size());
      for (int32_t& i : idx) i = next();
      const int rc = lmx_h_row_map(n, idx.empty() ? nullptr : idx.data(), n_idx, "det_idx", map.empty() ? nullptr : map.data(),
                                   ran.empty() ? nullptr : ran.data());
      printf("%d\t%s\t", rc, g_error);
      if (rc == LMX_OK) {
        bool first = true;
        for (const std::vector<int32_t>* a : {&map, &ran})
          for (int32_t x : *a) {
            printf(first ? "%d" : " %d", (int)x);
            first = false;
          }
      }
    } else {
      fprintf(stderr, "%s: query kind %d\n", argv[0], kind);
      return 2;
    }
    printf("\n");
  }
  return 0;
}
