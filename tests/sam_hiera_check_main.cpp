// sam_hiera_check_main.cpp — the reader of a SAM weight image whose encoder is Hiera (csrc/host_image.cpp + host_sam_image.cpp) and the
// Hiera block plan on the host (csrc/host_hiera_plan.cpp) as a stand-alone program, so that they can be built with
// -fsanitize=address,undefined, fed corrupted files and swept over frame and batch sizes (tests/test_sam_hiera_sanitized.py).
//   sam_hiera_check_main check PATH...   one line per file: "<return code>\t<path>\t<error text>"
//   sam_hiera_check_main plan QUERIES    QUERIES: a text file, one query per line, integers separated by blanks:
//     n_stages  blocks[n_stages]  dims[..]  heads[..]  windows[..]  n_global  global_blocks[n_global]  q_pool_stages  image
//     then either   0 n nh nw lowest               lmx_h_hiera_plan
//          or       1 n lowest rows[n_blocks]      lmx_h_hiera_plan_rows
//   one line of output per query: "<return code>\t<error text>\t<rows, blank separated>\t<the 20 fields of every record, blank separated>"
// The arrays handed to the library are heap blocks of exactly n_blocks entries, so that a write past the last block is a report.
// The plan reports through lmx_set_error, which lives in api.hip with the rest of the library: this program brings its own.
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
  if (argc >= 2 && strcmp(argv[1], "check") == 0) {
    for (int i = 2; i < argc; ++i) {
      g_error[0] = 0;
      lmx_sam_info_t info;
      const int rc = lmx_sam_image_check_host(argv[i], &info);
      printf("%d\t%s\t%s\n", rc, argv[i], g_error);
    }
    return 0;
  }
  if (argc != 3 || strcmp(argv[1], "plan") != 0) {
    fprintf(stderr, "usage: %s check PATH... | plan QUERIES\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[2]);
  if (!in) {
    fprintf(stderr, "%s: cannot read %s\n", argv[0], argv[2]);
    return 2;
  }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<long> v;
    for (long x; ss >> x;) v.push_back(x);
    size_t at = 0;
    auto next = [&]() -> int { return at < v.size() ? (int)v[at++] : 0; };
    lmx_hiera_config_t c;
    memset(&c, 0, sizeof(c));
    c.n_stages = next();
    if (c.n_stages < 0 || c.n_stages > LMX_HIERA_MAX_STAGES) {
      fprintf(stderr, "%s: a query of %d stages does not fit the structure\n", argv[0], c.n_stages);
      return 2;
    }
    int32_t* per_stage[4] = {c.blocks, c.dims, c.heads, c.windows};
    for (int32_t* a : per_stage)
      for (int s = 0; s < c.n_stages; ++s) a[s] = next();
    c.n_global = next();
    if (c.n_global < 0 || c.n_global > LMX_HIERA_MAX_GLOBAL) {
      fprintf(stderr, "%s: a query of %d global blocks does not fit the structure\n", argv[0], c.n_global);
      return 2;
    }
    for (int i = 0; i < c.n_global; ++i) c.global_blocks[i] = next();
    c.q_pool_stages = next();
    c.image = next();
    const int mode = next();
    g_error[0] = 0;
    int nb = 0, rc = lmx_h_hiera_blocks(&c, &nb);
    std::vector<int> rows;
    std::vector<lmx_hiera_block_t> recs;
    if (rc == LMX_OK) {
      rows.assign((size_t)nb, 0);
      recs.assign((size_t)nb, lmx_hiera_block_t());
      if (mode == 0) {
        const int n = next(), nh = next(), nw = next(), lowest = next();
        rc = lmx_h_hiera_plan(&c, n, nh, nw, lowest, recs.data(), rows.data());
      } else {
        const int n = next(), lowest = next();
        for (int& r : rows) r = next();
        rc = lmx_h_hiera_plan_rows(&c, n, rows.data(), lowest, recs.data());
      }
    }
    printf("%d\t%s\t", rc, g_error);
    if (rc == LMX_OK) {
      for (size_t i = 0; i < rows.size(); ++i) printf(i ? " %d" : "%d", rows[i]);
      printf("\t");
      for (size_t i = 0; i < recs.size(); ++i) {
        const lmx_hiera_block_t& P = recs[i];
        const int32_t f[20] = {P.H,      P.W,   P.Hf,       P.Ho,        P.Wo,   P.Hfo, P.join,     P.attn,  P.ln1, P.shortcut, P.query,
                               P.window, P.ln_out, P.mlp, P.emit_ln1, P.stage_end, P.keep, P.x16, P.join_out, P.clone};
        for (int k = 0; k < 20; ++k) printf(i || k ? " %d" : "%d", f[k]);
      }
    } else {
      printf("\t");
    }
    printf("\n");
  }
  return 0;
}
