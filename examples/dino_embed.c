/* dino_embed.c — DINO embeddings from raw frames in plain C: no Python, no HIP code of the caller's own.
 *
 *   cc -O2 -Iinclude examples/dino_embed.c -o dino_embed -Lvision-sam3-yolo-lameless_amd/lmx -llmx \
 *      -Wl,-rpath,$PWD/vision-sam3-yolo-lameless_amd/lmx -Wl,--allow-shlib-undefined
 *   ./dino_embed model.lmx frames.raw embeddings.f32 [max_batch]
 *
 * model.lmx     a weight image, exported once from Python: lmx.native.write_dino_image(embedder, "model.lmx")
 * frames.raw    int32 n, h, w (little-endian), then n * h * w * 3 bytes: BGR frames as cv2 delivers them
 * embeddings.f32  receives n * hidden float32: per frame, the mean over all tokens of the final LayerNorm
 *                 (services/dinov3-pipeline/app/main.py:98-113)
 * (--allow-shlib-undefined: liblmx.so's own dependency, the HIP runtime, is found at run time — ROCm's lib directory, or the one
 * torch ships, on LD_LIBRARY_PATH.) */
#include <stdio.h>
#include <stdlib.h>

#include "lmx.h"

static int fail(const char* what) {
  fprintf(stderr, "dino_embed: %s: %s\n", what, lmx_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.lmx frames.raw embeddings.f32 [max_batch]\n", argv[0]);
    return 2;
  }
  const int max_batch = argc > 4 ? atoi(argv[4]) : 8;
  lmx_dino_info_t info;
  if (lmx_dino_image_check_host(argv[1], &info) != LMX_OK) return fail("lmx_dino_image_check_host");

  FILE* f = fopen(argv[2], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) {
    fprintf(stderr, "dino_embed: %s: no int32 n, h, w header\n", argv[2]);
    return 1;
  }
  const int n = hdr[0], h = hdr[1], w = hdr[2];
  const size_t bytes = (size_t)n * h * w * 3;
  uint8_t* frames = (uint8_t*)malloc(bytes);
  float* emb = (float*)malloc((size_t)n * info.hidden * sizeof(float));
  if (!frames || !emb || fread(frames, 1, bytes, f) != bytes) {
    fprintf(stderr, "dino_embed: %s: fewer than %d frames of %d x %d\n", argv[2], n, h, w);
    return 1;
  }
  fclose(f);

  lmx_dino* model = NULL;
  if (lmx_dino_open_host(argv[1], max_batch, &model) != LMX_OK) return fail("lmx_dino_open_host");
  if (lmx_dino_embed_host(model, frames, n, h, w, /*rgb=*/0, emb) != LMX_OK) {
    lmx_dino_close(model);
    return fail("lmx_dino_embed_host");
  }
  lmx_dino_close(model);

  f = fopen(argv[3], "wb");
  if (!f || fwrite(emb, sizeof(float), (size_t)n * info.hidden, f) != (size_t)n * info.hidden || fclose(f) != 0) {
    fprintf(stderr, "dino_embed: cannot write %s\n", argv[3]);
    return 1;
  }
  printf("dino_embed: %d frames of %d x %d -> %d x %d float32 (%s, %d layers)\n", n, h, w, n, info.hidden,
         info.arch == LMX_DINO_V3 ? "dinov3" : "dinov2", info.layers);
  free(frames);
  free(emb);
  return 0;
}
