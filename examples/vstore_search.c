/* vstore_search.c — a gallery of embeddings in HBM and a cosine top-5 search over it in plain C: no Python, no HIP code of the caller's
 * own.
 *
 *   cc -O2 -Iinclude examples/vstore_search.c -o vstore_search -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./vstore_search [rows [dim [planted_slot]]]
 *
 * Fills a store of `dim`-wide vectors (default 384) with `rows` pseudo-random raw vectors (default 1000) through
 * lmx_vstore_put_host, starting from a capacity of 16 so that the gallery grows on the way, replaces one slot in place, and asks
 * for the five nearest neighbours of a noisy copy of the vector in `planted_slot` (default 17).  The store normalises what it is
 * given; scores are cosines.  The handle maps nothing but slots: ids and payloads are the caller's to keep.
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "vstore_search: %s: %s\n", what, lmx_last_error());
  return 1;
}

/* a small generator of its own, so that every platform plants the same vectors: uniform in [-1, 1) */
static uint64_t state = 0x9E3779B97F4A7C15ull;
static float uniform(void) {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((double)(state >> 40) / 8388608.0 - 1.0);
}

int main(int argc, char** argv) {
  const int rows = argc > 1 ? atoi(argv[1]) : 1000, dim = argc > 2 ? atoi(argv[2]) : 384, planted = argc > 3 ? atoi(argv[3]) : 17;
  if (rows < 1 || planted < 0 || planted >= rows) {
    fprintf(stderr, "usage: %s [rows [dim [planted_slot]]] with 0 <= planted_slot < rows\n", argv[0]);
    return 2;
  }
  lmx_vstore* store = NULL;
  if (lmx_vstore_open(dim, /*capacity=*/16, &store) != LMX_OK) return fail("lmx_vstore_open");
  float* v = (float*)malloc((size_t)dim * sizeof(float));
  float* query = (float*)malloc((size_t)dim * sizeof(float));
  if (!v || !query) return 1;
  for (int r = 0; r < rows; ++r) {
    for (int i = 0; i < dim; ++i) v[i] = 3.0f * uniform(); /* raw, not unit: the store normalises */
    if (r == planted)
      for (int i = 0; i < dim; ++i) query[i] = v[i];
    if (lmx_vstore_put_host(store, r, v, LMX_VSTORE_F32) != LMX_OK) return fail("lmx_vstore_put_host");
  }
  /* replace the last slot in place: the count stays */
  for (int i = 0; i < dim; ++i) v[i] = uniform();
  if (planted != rows - 1 && lmx_vstore_put_host(store, rows - 1, v, LMX_VSTORE_F32) != LMX_OK) return fail("lmx_vstore_put_host (replace)");
  for (int i = 0; i < dim; ++i) query[i] += 0.05f * uniform();

  float scores[5];
  int32_t slots[5];
  if (lmx_vstore_search_host(store, query, LMX_VSTORE_F32, /*Q=*/1, /*limits=*/NULL, /*k=*/5, scores, slots) != LMX_OK)
    return fail("lmx_vstore_search_host");
  printf("vstore_search: %lld rows of %d elements\n", (long long)lmx_vstore_count(store), dim);
  for (int j = 0; j < 5; ++j) printf("rank %d slot %d score %.9g\n", j, (int)slots[j], scores[j]);
  printf("planted neighbour %s: slot %d\n", slots[0] == planted ? "found" : "MISSED", planted);
  lmx_vstore_close(store);
  free(v);
  free(query);
  return slots[0] == planted ? 0 : 1;
}
