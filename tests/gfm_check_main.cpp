// gfm_check_main.cpp — the host half of the graph transformer (csrc/host_gfm.cpp: the graph builder and the host forward) as a
// stand-alone program, so that it can be built with -fsanitize=address,undefined and fed the files tests/test_gfm_sanitized.py writes.
//   gfm_check_main check PATH...    one line per file: "<return code>\t<path>\t<error text>" (the reader of the weight image, csrc/host_image.cpp
//                                   and csrc/host_gfm_image.cpp)
//   gfm_check_main CONFIG WEIGHTS GRAPH N E K TIMED S SEED TARGET
//     CONFIG   eight decimal integers, comma-separated: input_dim,d_model,n_heads,n_layers,ff,edge_dim,max_degree,max_spd
//     WEIGHTS  the f32 tensors of lmx.kernels.gfm_tensor_shapes in its order, one after the other
//     GRAPH    N x input_dim f32 node features, N x E f32 embeddings, N f32 timestamps (read only when TIMED is 1)
//   Prints the edges, the attributes, the degrees, idx and win, then pred, stats and (S = 0) node_pred and attn_to_target, floats as hex.
// Every buffer is sized exactly, so that a read or a write past an end is the sanitizer's to see.  The library reports through
// lmx_set_error, which lives in api.hip with the rest of it: this program brings its own.
#include "../vision-sam3-yolo-lameless_amd/csrc/gfm_image.h"
#include "check_main.h"

static const float* take(const std::vector<char*>& blocks, size_t& next) { return reinterpret_cast<const float*>(blocks[next++]); }

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
  const int F = w.input_dim, D = w.d_model, H = w.n_heads, L = w.n_layers, FF = w.ff, dh = D / H, PD = lmx_gfm_pool_dim(D), Q = D / 16;

  // the tensors in the order of gfm_tensor_shapes, each in an allocation of its own size
  std::vector<size_t> counts = {(size_t)lmx_gfm_packed_floats(F, D), (size_t)D, (size_t)D, (size_t)D, (size_t)(w.max_degree + 1) * D,
                                (size_t)(w.max_degree + 1) * D, (size_t)lmx_gfm_packed_floats(D, D), (size_t)D, (size_t)D / 2,
                                (size_t)(w.max_spd + 2) * H, (size_t)2 * H * 3, (size_t)2 * H, (size_t)H * 2 * H, (size_t)H};
  for (int l = 0; l < L; ++l) {
    const size_t layer[] = {(size_t)D, (size_t)D, (size_t)H * Q * (3 * dh / 16) * 256, (size_t)H * 3 * dh, (size_t)Q * Q * 256, (size_t)D, (size_t)D,
                            (size_t)D, (size_t)Q * (FF / 16) * 256, (size_t)FF, (size_t)(FF / 16) * Q * 256, (size_t)D, (size_t)D,
                            (size_t)H * Q * (3 * dh / 16) * 256, (size_t)H * 3 * dh, (size_t)Q * Q * 256, (size_t)D};
    counts.insert(counts.end(), layer, layer + 17);
  }
  const size_t tail[] = {(size_t)D * 2 * D, (size_t)2 * D, (size_t)2 * D * D, (size_t)D, (size_t)D, (size_t)D, (size_t)D, (size_t)D,
                         (size_t)Q * (PD / 16) * 256, (size_t)PD, (size_t)PD, 1, (size_t)3 * D * D, (size_t)D, (size_t)D, (size_t)D,
                         (size_t)D * (D / 2), (size_t)D / 2, (size_t)(D / 2) * (D / 4), (size_t)D / 4, (size_t)D / 4, 1,
                         (size_t)Q * (PD / 16) * 256, (size_t)PD, (size_t)PD, 1};
  counts.insert(counts.end(), tail, tail + 26);
  std::vector<char*> blocks;
  if (!load_tensors(argv[2], counts, false, blocks)) return 2;
  size_t next = 0;
  const float** head[] = {&w.in_w, &w.in_b, &w.in_g, &w.in_beta, &w.deg_in, &w.deg_out, &w.time_w, &w.time_b, &w.div_term, &w.spd, &w.e1_w,
                          &w.e1_b, &w.e2_w, &w.e2_b};
  for (const float** p : head) *p = take(blocks, next);
  for (int l = 0; l < L; ++l) {
    const float** layer[] = {&w.ln1_g[l], &w.ln1_b[l], &w.qkv_w[l], &w.qkv_b[l], &w.out_w[l], &w.out_b[l], &w.ln2_g[l], &w.ln2_b[l], &w.ff1_w[l],
                             &w.ff1_b[l], &w.ff2_w[l], &w.ff2_b[l], &w.vn[l], &w.vqkv_w[l], &w.vqkv_b[l], &w.vout_w[l], &w.vout_b[l]};
    for (const float** p : layer) *p = take(blocks, next);
  }
  const float** rest[] = {&w.vu1_w, &w.vu1_b, &w.vu2_w, &w.vu2_b, &w.vu_g, &w.vu_beta, &w.lnf_g, &w.lnf_b, &w.pool1_w, &w.pool1_b, &w.pool2_w,
                          &w.pool2_b, &w.comb_w, &w.comb_b, &w.comb_g, &w.comb_beta, &w.ph1_w, &w.ph1_b, &w.ph2_w, &w.ph2_b, &w.ph3_w, &w.ph3_b,
                          &w.nh1_w, &w.nh1_b, &w.nh2_w, &w.nh2_b};
  for (const float** p : rest) *p = take(blocks, next);

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
