/* gfm_score.c — a cow's lameness score, its MC-dropout uncertainty, the node scores and the attention towards the target video from
 * one graph in plain C: no Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/gfm_score.c -o gfm_score -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./gfm_score model.lmx graph.bin seed target [n_samples]
 *
 * model.lmx   a weight image, exported once from Python: lmx.native.write_gfm_image(cfg, weights, "model.lmx") with
 *             cfg, weights = lmx.checkpoints.gfm_from_state_dict(torch.load("graphormer_lameness.pt"), num_heads=8)
 * graph.bin   int32 N, int32 E, int32 timed (little-endian), then N x input_dim float32 node features, N x E float32 embeddings and,
 *             when timed is 1, N float32 timestamps in seconds: the videos of one cow
 * seed        the graph's 64-bit dropout seed in decimal; the service uses the first 8 bytes of SHA-256(video_id), little-endian
 * target      the node of the video that is being scored
 * Prints what services/graph-transformer-pipeline/app/main.py:352-387 computes: the graph by the pinned rules of lmx_h_gfm_graph
 * (k = 5), ten samples by default, then the eval-mode node score of the target and the five nodes that attend to it most.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "gfm_score: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s model.lmx graph.bin seed target [n_samples]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[3], NULL, 10);
  const int32_t target = atoi(argv[4]);
  const int S = argc > 5 ? atoi(argv[5]) : 10, K = 5;
  lmx_gfm_info_t info;
  if (lmx_gfm_image_check_host(argv[1], &info)) return fail("image");
  int32_t head[3];
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(head, 4, 3, f) != 3 || head[0] < 1 || head[0] > info.max_nodes || head[1] < 1 || head[1] > 4096) {
    fprintf(stderr, "gfm_score: cannot read %s, or its N is outside 1 .. %d\n", argv[2], info.max_nodes);
    return 2;
  }
  const int N = head[0], E = head[1], timed = head[2] == 1, k = K < N - 1 ? K : N - 1, cap = N * k + 2 * (N - 1) + 1;
  float* x = malloc(sizeof(float) * N * info.input_dim);
  float* emb = malloc(sizeof(float) * N * E);
  float* ts = malloc(sizeof(float) * N);
  if (fread(x, 4, (size_t)N * info.input_dim, f) != (size_t)N * info.input_dim || fread(emb, 4, (size_t)N * E, f) != (size_t)N * E ||
      (timed && fread(ts, 4, N, f) != (size_t)N)) {
    fprintf(stderr, "gfm_score: %s is too short\n", argv[2]);
    return 2;
  }
  fclose(f);

  /* the graph, once: edges, attributes, clamped degrees, the shortest-path index matrix and the winning edge per pair */
  int32_t* edges = malloc(sizeof(int32_t) * 2 * cap);
  float* attr = malloc(sizeof(float) * 3 * cap);
  uint8_t* deg_in = malloc(N);
  uint8_t* deg_out = malloc(N);
  uint8_t* idx = malloc((size_t)N * N);
  int32_t* win = malloc(sizeof(int32_t) * N * N);
  int32_t n_edges = 0;
  if (lmx_h_gfm_graph(emb, timed ? ts : NULL, N, E, K, info.max_degree, info.max_spd, edges, attr, &n_edges, deg_in, deg_out, idx, win))
    return fail("graph");
  printf("%d nodes, %d edges\n", N, n_edges);

  lmx_gfm* m;
  if (lmx_gfm_open_host(argv[1], /*max_graphs=*/1, /*max_nodes_total=*/info.max_nodes, /*max_samples=*/S > 2 ? S : 2, &m)) return fail("open");
  const int32_t node_off[2] = {0, N}, edge_off[2] = {0, n_edges};
  const uint8_t has_time = 1;
  lmx_gfm_graphs_t g = {1, 0, node_off, edge_off, x, timed ? ts : NULL, timed ? &has_time : NULL, deg_in, deg_out, idx, win, attr, &target};
  float* pred = malloc(sizeof(float) * (S > 0 ? S : 1));
  float* node = malloc(sizeof(float) * N);
  float* attn = malloc(sizeof(float) * N);
  float stats[2], pred0, stats0[2];
  if (lmx_gfm_score_host(m, &g, &seed, S, pred, stats, NULL, NULL)) return fail("score");
  printf("cow_severity_score %.6f uncertainty %.6f\n", stats[0], stats[1]);
  if (lmx_gfm_score_host(m, &g, NULL, 0, &pred0, stats0, node, attn)) return fail("eval");
  if (target >= 0 && target < N) printf("node_prediction %.6f\n", node[target]);
  for (int shown = 0; shown < 5; ++shown) { /* the five largest entries of the attention column, the target itself left out */
    int best = -1;
    for (int i = 0; i < N; ++i)
      if (i != target && attn[i] >= 0.0f && (best < 0 || attn[i] > attn[best])) best = i;
    if (best < 0) break;
    printf("attention node %d %.6f\n", best, attn[best]);
    attn[best] = -1.0f;
  }
  lmx_gfm_close(m);
  return 0;
}
