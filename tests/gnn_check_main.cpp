// gnn_check_main.cpp — the host half of GraphGPS (csrc/host_gnn.cpp: the graph builder with both encodings and the host forward) as a
// stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_gnn_sanitized.py writes.
//   gnn_check_main check PATH...    one line per file: "<return code>\t<path>\t<error text>" (the reader of the weight image, csrc/host_image.cpp
//                                   and csrc/host_gnn_image.cpp)
//   gnn_check_main CONFIG WEIGHTS GRAPH N E K TIMED S SEED
//     CONFIG   seven decimal integers, comma-separated: input_dim,d_model,n_heads,n_layers,pe_dim,ff,edge_dim
//     WEIGHTS  the f32 tensors of the weight table (lmx_gnn_tensor_rows, lmx.kernels.gnn_tensor_shapes) in its order, one after the other
//     GRAPH    N x input_dim f32 node features, N x E f32 embeddings, N f64 timestamps (read only when TIMED is 1)
//   Prints the edges, the attributes, the CSR, the degrees, both encodings, then (S > 0) node_mc and stats or (S = 0) graph_pred,
//   node_pred and attn_weights, floats as hex.
// Every buffer is sized exactly, so that a read or a write past an end is the sanitizer's to see.  The library reports through
// lmx_set_error, which lives in api.hip with the rest of it: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/gnn_image.h"
#include "check_main.h"

int main(int argc, char** argv) {
  if (check_mode(argc, argv, lmx_gnn_image_check_host)) return 0;
  if (argc != 10) {
    fprintf(stderr, "usage: %s CONFIG WEIGHTS GRAPH N E K TIMED S SEED\n", argv[0]);
    return 2;
  }
  lmx_gnn_weights_t w;
  memset(&w, 0, sizeof(w));
  if (sscanf(argv[1], "%d,%d,%d,%d,%d,%d,%d", &w.input_dim, &w.d_model, &w.n_heads, &w.n_layers, &w.pe_dim, &w.ff, &w.edge_dim) != 7) return 2;
  if (lmx_gnn_check_config("gnn_check_main", &w, false)) return fail("config");
  const int N = atoi(argv[4]), E = atoi(argv[5]), k = atoi(argv[6]), timed = atoi(argv[7]), S = atoi(argv[8]);
  uint64_t seed = strtoull(argv[9], nullptr, 10);
  const int F = w.input_dim, D = w.d_model;

  // the tensors of the weight table in its order, each in an allocation of its own size, its address where the table says
  std::vector<LmxTensorRow> rows;
  lmx_gnn_tensor_rows(w, &rows);
  std::vector<size_t> counts;
  for (const LmxTensorRow& r : rows) {
    size_t count = 1;
    for (int d = 0; d < r.rank; ++d) count *= (size_t)r.shape[d];
    counts.push_back(count);
  }
  std::vector<char*> blocks;
  if (!load_tensors(argv[2], counts, true, blocks)) return 2;
  bind_blocks(rows, blocks, &w);

  if (N < 1 || N > 4096 || E < 1 || E > 4096 || k < 1) return 2;
  std::vector<float> x((size_t)N * F), emb((size_t)N * E);
  std::vector<double> ts((size_t)(timed ? N : 0));
  FILE* f = fopen(argv[3], "rb");
  if (!f || !read_all(f, x) || !read_all(f, emb) || (timed && !read_all(f, ts))) return 2;
  fclose(f);
  const int kk = N <= k ? (N - 1 > 1 ? N - 1 : 1) : k, cap = N > 1 ? N * kk + (timed ? 2 * (N - 1) : 0) : 0;  // exactly what the rules give
  std::vector<int32_t> edges((size_t)cap * 2), ptr((size_t)N + 1), cse((size_t)cap), deg((size_t)N);
  std::vector<float> attr((size_t)cap * 3), lap((size_t)N * LMX_GNN_LAP_K), rw((size_t)N * LMX_GNN_RW_K);
  int32_t ne = 0;
  if (lmx_h_gnn_graph(emb.data(), timed ? ts.data() : nullptr, N, E, k, cap ? edges.data() : nullptr, cap ? attr.data() : nullptr, &ne, ptr.data(),
                      cap ? cse.data() : nullptr, deg.data(), lap.data(), rw.data()))
    return fail("graph");
  if (ne != cap) return fail("edge count");
  for (int e = 0; e < ne; ++e) printf("edge %d %d %a %a %a\n", edges[2 * e], edges[2 * e + 1], attr[3 * e], attr[3 * e + 1], attr[3 * e + 2]);
  for (int i = 0; i <= N; ++i) printf("ptr %d\n", ptr[i]);
  for (int e = 0; e < ne; ++e) printf("csr %d\n", cse[e]);
  for (int i = 0; i < N; ++i) {
    printf("node %d", deg[i]);
    for (int c = 0; c < LMX_GNN_LAP_K; ++c) printf(" %a", lap[(size_t)i * LMX_GNN_LAP_K + c]);
    for (int c = 0; c < LMX_GNN_RW_K; ++c) printf(" %a", rw[(size_t)i * LMX_GNN_RW_K + c]);
    printf("\n");
  }
  std::vector<double> lam((size_t)N), vec((size_t)N * N);
  if (lmx_h_gnn_laplacian(cap ? edges.data() : nullptr, ne, N, lam.data(), vec.data())) return fail("laplacian");
  for (int i = 0; i < N; ++i) printf("eigenvalue %a\n", lam[i]);

  std::vector<int32_t> src((size_t)ne), dst((size_t)ne);
  for (int e = 0; e < ne; ++e) src[e] = edges[2 * e], dst[e] = edges[2 * e + 1];
  const int32_t node_off[2] = {0, N}, edge_off[2] = {0, ne};
  lmx_gnn_graphs_t g;
  memset(&g, 0, sizeof(g));
  g.n = 1, g.node_off_host = node_off, g.edge_off_host = edge_off, g.x = x.data(), g.lap = lap.data(), g.rw = rw.data();
  g.edge_src = ne ? src.data() : nullptr, g.edge_dst = ne ? dst.data() : nullptr, g.edge_attr = ne ? attr.data() : nullptr;
  g.csr_ptr = ptr.data(), g.csr_edge = ne ? cse.data() : nullptr, g.deg = deg.data();
  const int Smax = S > 0 ? S : 1;
  std::vector<float> mc((size_t)N * S), stats((size_t)(S ? 2 * N : 0)), node((size_t)(S ? 0 : N)), at((size_t)(S ? 0 : N)), trunk((size_t)Smax * N * D);
  float gp = 0.0f;
  if (lmx_h_gnn_forward(&w, &g, &seed, S, 0.1, S ? mc.data() : nullptr, S ? stats.data() : nullptr, S ? nullptr : &gp, S ? nullptr : node.data(),
                        S ? nullptr : at.data(), trunk.data()))
    return fail("forward");
  if (S) {
    for (int i = 0; i < N; ++i) {
      printf("mc");
      for (int s = 0; s < S; ++s) printf(" %a", mc[(size_t)i * S + s]);
      printf(" %a %a\n", stats[2 * i], stats[2 * i + 1]);
    }
  } else {
    printf("graph %a\n", gp);
    for (int i = 0; i < N; ++i) printf("eval %a %a\n", node[i], at[i]);
  }
  for (char* p : blocks) free(p);
  return 0;
}
