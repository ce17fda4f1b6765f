/* gnn_score.c — a video's GraphGPS severity score with its MC-dropout uncertainty, the cow score and the first neighbours' scores from
 * one graph in plain C: no Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/gnn_score.c -o gnn_score -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./gnn_score model.lmx graph.bin seed target [n_samples]
 *
 * model.lmx   a weight image, exported once from Python: lmx.native.write_gnn_image(cfg, weights, "model.lmx") with
 *             cfg, weights = lmx.checkpoints.gnn_from_state_dict(torch.load("enhancedgraphgps_lameness.pt"), num_heads=8)
 * graph.bin   int32 N, int32 E, int32 timed (little-endian), then N x input_dim float32 node features, N x E float32 embeddings and,
 *             when timed is 1 (the cow is known), N float64 timestamps in seconds: the videos of one cow
 * seed        the graph's 64-bit dropout seed in decimal; the service uses the first 8 bytes of SHA-256(video_id), little-endian
 * target      the node of the video that is being scored
 * Prints what services/gnn-pipeline/app/main.py:1483-1545 computes: the graph by the pinned rules of lmx_h_gnn_graph (k = 5), ten
 * samples by default (N >= 2: one node has no batch statistics), then the eval-mode cow score and the first five edges into the target.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "gnn_score: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s model.lmx graph.bin seed target [n_samples]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[3], NULL, 10);
  const int target = atoi(argv[4]);
  const int S = argc > 5 ? atoi(argv[5]) : 10, K = 5;
  lmx_gnn_info_t info;
  if (lmx_gnn_image_check_host(argv[1], &info)) return fail("image");
  int32_t head[3];
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(head, 4, 3, f) != 3 || head[0] < 1 || head[0] > info.max_nodes || head[1] < 1 || head[1] > 4096) {
    fprintf(stderr, "gnn_score: cannot read %s, or its N is outside 1 .. %d\n", argv[2], info.max_nodes);
    return 2;
  }
  const int N = head[0], E = head[1], timed = head[2] == 1, cap = N * K + 2 * (N - 1) + 1;
  float* x = malloc(sizeof(float) * N * info.input_dim);
  float* emb = malloc(sizeof(float) * N * E);
  double* ts = malloc(sizeof(double) * N);
  if (fread(x, 4, (size_t)N * info.input_dim, f) != (size_t)N * info.input_dim || fread(emb, 4, (size_t)N * E, f) != (size_t)N * E ||
      (timed && fread(ts, 8, N, f) != (size_t)N)) {
    fprintf(stderr, "gnn_score: %s is too short\n", argv[2]);
    return 2;
  }
  fclose(f);

  /* the graph, once: edges, attributes, the CSR by destination, the clamped in-degree and both raw encodings */
  int32_t* edges = malloc(sizeof(int32_t) * 2 * cap);
  float* attr = malloc(sizeof(float) * 3 * cap);
  int32_t* ptr = malloc(sizeof(int32_t) * (N + 1));
  int32_t* cse = malloc(sizeof(int32_t) * cap);
  int32_t* deg = malloc(sizeof(int32_t) * N);
  float* lap = malloc(sizeof(float) * N * LMX_GNN_LAP_K);
  float* rw = malloc(sizeof(float) * N * LMX_GNN_RW_K);
  int32_t n_edges = 0;
  if (lmx_h_gnn_graph(emb, timed ? ts : NULL, N, E, K, edges, attr, &n_edges, ptr, cse, deg, lap, rw)) return fail("graph");
  printf("%d nodes, %d edges\n", N, n_edges);
  int32_t* src = malloc(sizeof(int32_t) * (n_edges + 1));
  int32_t* dst = malloc(sizeof(int32_t) * (n_edges + 1));
  for (int e = 0; e < n_edges; ++e) src[e] = edges[2 * e], dst[e] = edges[2 * e + 1];

  lmx_gnn* m;
  if (lmx_gnn_open_host(argv[1], /*max_graphs=*/1, /*max_nodes_total=*/N, /*max_edges_total=*/n_edges, /*max_samples=*/S > 2 ? S : 2, &m))
    return fail("open");
  const int32_t node_off[2] = {0, N}, edge_off[2] = {0, n_edges};
  lmx_gnn_graphs_t g = {1, 0, node_off, edge_off, x, lap, rw, src, dst, attr, ptr, cse, deg};
  float* mc = malloc(sizeof(float) * N * (S > 0 ? S : 1));
  float* stats = malloc(sizeof(float) * 2 * N);
  float* node = malloc(sizeof(float) * N);
  float* attw = malloc(sizeof(float) * N);
  float cow = 0.0f;
  if (S > 0 && lmx_gnn_score_host(m, &g, &seed, S, mc, stats, NULL, NULL, NULL)) return fail("score");
  if (lmx_gnn_score_host(m, &g, NULL, 0, NULL, NULL, &cow, node, attw)) return fail("eval");
  if (target >= 0 && target < N) {
    if (S > 0) printf("severity_score %.6f uncertainty %.6f\n", stats[2 * target], stats[2 * target + 1]);
    printf("eval node_pred %.6f attention_weight %.6f\n", node[target], attw[target]);
  }
  printf("cow_severity_score %.6f\n", cow);
  for (int q = ptr[target >= 0 && target < N ? target : 0], shown = 0; target >= 0 && target < N && q < ptr[target + 1] && shown < 5; ++q, ++shown) {
    const int s = src[cse[q]]; /* the first five edges into the target, in edge order */
    printf("neighbour node %d %.6f\n", s, S > 0 ? stats[2 * s] : node[s]);
  }
  lmx_gnn_close(m);
  return 0;
}
