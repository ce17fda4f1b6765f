// gfm_check_main.cpp — the host half of the graph transformer (csrc/host_gfm.cpp: the graph builder and the host forward) as a
// stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_gfm_sanitized.py writes.
//   gfm_check_main check PATH...    one line per file: "<return code>\t<path>\t<error text>" (the reader of the weight image, csrc/host_image.cpp
//                                   and csrc/host_gfm_image.cpp)
//   gfm_check_main CONFIG WEIGHTS GRAPH N E K TIMED S SEED TARGET
//     CONFIG   eight decimal integers, comma-separated: input_dim,d_model,n_heads,n_layers,ff,edge_dim,max_degree,max_spd
//     WEIGHTS  the f32 tensors of the weight table (lmx_gfm_tensor_rows, lmx.kernels.gfm_tensor_shapes) in its order, one after the other
//     GRAPH    N x input_dim f32 node features, N x E f32 embeddings, N f32 timestamps (read only when TIMED is 1)
//   Prints the edges, the attributes, the degrees, idx and win, then pred, stats and (S = 0) node_pred and attn_to_target, floats as hex.
// Every buffer is sized exactly, so that a read or a write past an end is the sanitizer's to see.  The library reports through
// lmx_set_error, which lives in api.hip with the rest of it: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/gfm_image.h"
#include "check_main.h"

int main(int argc, char** argv) {
  if (check_mode(argc, argv, lmx_gfm_image_check_host)) return 0;
  if (argc != 11) {
    fprintf(stderr, "usage: %s CONFIG WEIGHTS GRAPH N E K TIMED S SEED TARGET\n", argv[0]);
    return 2;
  }
  lmx_gfm_weights_t w;
  memset(&w, 0, sizeof(w));
  if (sscanf(argv[1], "%d,%d,%d,%d,%d,%d,%d,%d", &w.input_dim, &w.d_model, &w.n_heads, &w.n_layers, &w.ff, &w.edge_dim, &w.max_degree, &w.max_spd) != 8)
    return 2;
  if (lmx_gfm_check_config("gfm_check_main", &w, false)) return fail("config");
  const int N = atoi(argv[4]), E = atoi(argv[5]), k = atoi(argv[6]), timed = atoi(argv[7]), S = atoi(argv[8]), target = atoi(argv[10]);
  uint64_t seed = strtoull(argv[9], nullptr, 10);
  const int F = w.input_dim, D = w.d_model;

  // the tensors of the weight table in its order, each in an allocation of its own size, its address where the table says
  std::vector<LmxTensorRow> rows;
  lmx_gfm_tensor_rows(w, &rows);
  std::vector<size_t> counts;
  for (const LmxTensorRow& r : rows) {
    size_t count = 1;
    for (int d = 0; d < r.rank; ++d) count *= (size_t)r.shape[d];
    counts.push_back(count);
  }
  std::vector<char*> blocks;
  if (!load_tensors(argv[2], counts, false, blocks)) return 2;
  bind_blocks(rows, blocks, &w);

  if (N < 1 || N > 4096 || E < 1 || E > 4096 || k < 0) return 2;
  std::vector<float> x((size_t)N * F), emb((size_t)N * E), ts((size_t)(timed ? N : 0));
  FILE* f = fopen(argv[3], "rb");
  if (!f || !read_all(f, x) || !read_all(f, emb) || (timed && !read_all(f, ts))) return 2;
  fclose(f);
  const int kk = k < N - 1 ? k : N - 1, cap = N * kk + 2 * (N - 1);
  std::vector<int32_t> edges((size_t)cap * 2), win((size_t)N * N);
  std::vector<float> attr((size_t)cap * 3);
  std::vector<uint8_t> din((size_t)N), dout((size_t)N), idx((size_t)N * N), has_time(1, (uint8_t)timed);
  int32_t ne = 0;
  if (lmx_h_gfm_graph(emb.data(), timed ? ts.data() : nullptr, N, E, k, w.max_degree, w.max_spd, edges.data(), attr.data(), &ne, din.data(),
                      dout.data(), idx.data(), win.data()))
    return fail("graph");
  for (int e = 0; e < ne; ++e) printf("edge %d %d %a %a %a\n", edges[2 * e], edges[2 * e + 1], attr[3 * e], attr[3 * e + 1], attr[3 * e + 2]);
  for (int i = 0; i < N; ++i) printf("degree %d %d\n", din[i], dout[i]);
  long long si = 0, sw = 0;
  for (int i = 0; i < N * N; ++i) si += (long long)idx[i] * (i + 1), sw += (long long)(win[i] + 2) * (i + 1);
  printf("matrices %lld %lld\n", si, sw);

  // exactly the edges the builder made: the forward may read no further
  std::vector<float> used(attr.begin(), attr.begin() + (size_t)ne * 3);
  const int32_t node_off[2] = {0, N}, edge_off[2] = {0, ne};
  lmx_gfm_graphs_t g;
  memset(&g, 0, sizeof(g));
  g.n = 1, g.node_off_host = node_off, g.edge_off_host = edge_off, g.x = x.data(), g.timestamps = timed ? ts.data() : nullptr;
  g.has_time = timed ? has_time.data() : nullptr, g.deg_in = din.data(), g.deg_out = dout.data(), g.idx = idx.data(), g.win = win.data();
  g.edge_attr = ne ? used.data() : nullptr, g.target = &target;
  const int Smax = S > 0 ? S : 1;
  std::vector<float> pred((size_t)Smax), node((size_t)N), at((size_t)N), trunk((size_t)Smax * N * D), vn((size_t)Smax * D);
  float stats[2];
  if (lmx_h_gfm_forward(&w, &g, &seed, S, 0.1, pred.data(), stats, S == 0 ? node.data() : nullptr, S == 0 ? at.data() : nullptr, trunk.data(),
                        vn.data()))
    return fail("forward");
  for (float v : pred) printf("pred %a\n", v);
  printf("stats %a %a\n", stats[0], stats[1]);
  if (S == 0)
    for (int i = 0; i < N; ++i) printf("node %a %a\n", node[i], at[i]);
  for (char* p : blocks) free(p);
  return 0;
}
