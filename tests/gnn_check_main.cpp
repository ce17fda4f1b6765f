// gnn_check_main.cpp — the host half of GraphGPS (csrc/host_gnn.cpp: the graph builder with both encodings and the host forward) as a
// stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_gnn_sanitized.py writes.
//   gnn_check_main check PATH...    one line per file: "<return code>\t<path>\t<error text>" (the reader of the weight image, csrc/host_image.cpp
//                                   and csrc/host_gnn_image.cpp)
//   gnn_check_main CONFIG WEIGHTS GRAPH N E K TIMED S SEED
//     CONFIG   seven decimal integers, comma-separated: input_dim,d_model,n_heads,n_layers,pe_dim,ff,edge_dim
//     WEIGHTS  the f32 tensors of lmx.kernels.gnn_tensor_shapes in its order, one after the other
//     GRAPH    N x input_dim f32 node features, N x E f32 embeddings, N f64 timestamps (read only when TIMED is 1)
//   Prints the edges, the attributes, the CSR, the degrees, both encodings, then (S > 0) node_mc and stats or (S = 0) graph_pred,
//   node_pred and attn_weights, floats as hex.
// Every buffer is sized exactly, so that a read or a write past an end is the sanitizer's to see.  The library reports through
// lmx_set_error, which lives in api.hip with the rest of it: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/gnn_image.h"
#include "check_main.h"

static const float* take(const std::vector<char*>& blocks, size_t& next) { return reinterpret_cast<const float*>(blocks[next++]); }

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
  const int F = w.input_dim, D = w.d_model, H = w.n_heads, L = w.n_layers, FF = w.ff, P = w.pe_dim, dh = D / H, Q = D / 16, D2 = D / 2;

  // the tensors in the order of gnn_tensor_shapes, each in an allocation of its own size
  std::vector<size_t> counts = {(size_t)lmx_gnn_packed_floats(F, D - 2 * P), (size_t)D - 2 * P};
  for (int enc = 0; enc < 2; ++enc) {
    const size_t K = enc ? LMX_GNN_RW_K : LMX_GNN_LAP_K;
    const size_t one[] = {(size_t)2 * P * K, (size_t)2 * P, (size_t)P * 2 * P, (size_t)P, (size_t)P, (size_t)P};
    counts.insert(counts.end(), one, one + 6);
  }
  const size_t edge[] = {(size_t)D2 * 3, (size_t)D2, (size_t)lmx_gnn_packed_floats(D2, D), (size_t)D, (size_t)D, (size_t)D};
  counts.insert(counts.end(), edge, edge + 6);
  const size_t sq = (size_t)Q * Q * 256, v = (size_t)D;
  for (int l = 0; l < L; ++l) {
    const size_t front[] = {v, v, 4 * sq, 4 * v, sq, v};
    counts.insert(counts.end(), front, front + 6);
    if (l < L - 1) {
      const size_t update[] = {3 * sq, v, sq, v, v, v, v, v};
      counts.insert(counts.end(), update, update + 8);
    }
    const size_t back[] = {v, v, v, v, v, v, (size_t)H * Q * (3 * dh / 16) * 256, (size_t)H * 3 * dh, sq, v, v, v, v, v, (size_t)Q * (FF / 16) * 256,
                           (size_t)FF, (size_t)(FF / 16) * Q * 256, v};
    counts.insert(counts.end(), back, back + 18);
  }
  const size_t half = (size_t)Q * (D2 / 16) * 256;
  const size_t tail[] = {v, v, half, (size_t)D2, (size_t)D2, 1, half, (size_t)D2, (size_t)D2, 1, 2 * v * v, v, v * D2, (size_t)D2, (size_t)D2, 1};
  counts.insert(counts.end(), tail, tail + 16);
  std::vector<char*> blocks;
  if (!load_tensors(argv[2], counts, true, blocks)) return 2;
  size_t next = 0;
  const float** head[] = {&w.in_w, &w.in_b, &w.lap1_w, &w.lap1_b, &w.lap2_w, &w.lap2_b, &w.lap_g, &w.lap_beta, &w.rw1_w, &w.rw1_b,
                          &w.rw2_w, &w.rw2_b, &w.rw_g, &w.rw_beta, &w.ee1_w, &w.ee1_b, &w.ee2_w, &w.ee2_b, &w.ee_g, &w.ee_beta};
  for (const float** p : head) *p = take(blocks, next);
  for (int l = 0; l < L; ++l) {
    const float** front[] = {&w.ln1_g[l], &w.ln1_b[l], &w.abde_w[l], &w.abde_b[l], &w.c_w[l], &w.c_b[l]};
    for (const float** p : front) *p = take(blocks, next);
    if (l < L - 1) {
      const float** update[] = {&w.eu1_w[l], &w.eu1_b[l], &w.eu2_w[l], &w.eu2_b[l], &w.bne_g[l], &w.bne_b[l], &w.bne_mean[l], &w.bne_var[l]};
      for (const float** p : update) *p = take(blocks, next);
    }
    const float** back[] = {&w.bnn_g[l], &w.bnn_b[l], &w.bnn_mean[l], &w.bnn_var[l], &w.ln2_g[l], &w.ln2_b[l], &w.qkv_w[l], &w.qkv_b[l], &w.out_w[l],
                            &w.out_b[l], &w.lna_g[l], &w.lna_b[l], &w.ln3_g[l], &w.ln3_b[l], &w.ff1_w[l], &w.ff1_b[l], &w.ff2_w[l], &w.ff2_b[l]};
    for (const float** p : back) *p = take(blocks, next);
  }
  const float** rest[] = {&w.lnf_g, &w.lnf_b, &w.nh1_w, &w.nh1_b, &w.nh2_w, &w.nh2_b, &w.na1_w, &w.na1_b, &w.na2_w, &w.na2_b, &w.cl1_w, &w.cl1_b,
                          &w.cl2_w, &w.cl2_b, &w.cl3_w, &w.cl3_b};
  for (const float** p : rest) *p = take(blocks, next);

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
