// hiera_config.h — lmx_hiera_config_t (include/lmx.h) on the host: its limits and the block table it stands for, shared by the block plan
// (host_hiera_plan.cpp) and the reader of a SAM weight image whose encoder is Hiera (host_sam_image.cpp).  Host code only: nothing
// here needs HIP, and nothing outside this header is needed to link it.
#pragma once
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define HIERA_REQUIRE(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

struct LmxHieraBlock {  // one entry of lmx.sam.HieraConfig.block_plan(): win 0 = global attention, qs 2 = the block pools its queries
  int dim, D, heads, win, qs;
};

// The limits of the structure and of the plan; *n_blocks = the sum of blocks[s].  `who` opens every message.
inline int lmx_hiera_check_config(const lmx_hiera_config_t* c, const char* who, int* n_blocks) {
  HIERA_REQUIRE(c, "%s: null config", who);
  HIERA_REQUIRE(c->n_stages >= 1 && c->n_stages <= LMX_HIERA_MAX_STAGES, "%s: n_stages %d (1 .. %d)", who, c->n_stages, (int)LMX_HIERA_MAX_STAGES);
  HIERA_REQUIRE(c->image >= 4 && c->image <= 8192 && c->image % 4 == 0, "%s: image %d (a multiple of 4 up to 8192)", who, c->image);
  int nb = 0;
  for (int s = 0; s < c->n_stages; ++s) {
    HIERA_REQUIRE(c->blocks[s] >= 1 && c->blocks[s] <= LMX_HIERA_MAX_BLOCKS, "%s: blocks[%d] = %d", who, s, c->blocks[s]);
    HIERA_REQUIRE(c->dims[s] > 0 && c->dims[s] <= 16384 && c->heads[s] > 0 && c->heads[s] <= c->dims[s] && c->windows[s] > 0 && c->windows[s] <= c->image,
                  "%s: stage %d: dims %d heads %d windows %d", who, s, c->dims[s], c->heads[s], c->windows[s]);
    nb += c->blocks[s];
    HIERA_REQUIRE(nb <= LMX_HIERA_MAX_BLOCKS, "%s: more than %d blocks", who, (int)LMX_HIERA_MAX_BLOCKS);
  }
  HIERA_REQUIRE(c->q_pool_stages >= 0 && c->q_pool_stages <= LMX_HIERA_MAX_STAGES, "%s: q_pool_stages %d", who, c->q_pool_stages);
  HIERA_REQUIRE(c->n_global >= 0 && c->n_global <= LMX_HIERA_MAX_GLOBAL, "%s: n_global %d (0 .. %d)", who, c->n_global, (int)LMX_HIERA_MAX_GLOBAL);
  for (int i = 0; i < c->n_global; ++i)
    HIERA_REQUIRE(c->global_blocks[i] >= 0 && c->global_blocks[i] < nb, "%s: global_blocks[%d] = %d is not a block of 0 .. %d", who, i,
                  c->global_blocks[i], nb - 1);
  *n_blocks = nb;
  return LMX_OK;
}

// HieraConfig.block_plan() of a checked configuration; stage_end[i]: the index of the stage block i ends, or -1
inline void lmx_hiera_block_table(const lmx_hiera_config_t* c, LmxHieraBlock* blocks, int* stage_end) {
  int t = 0;
  for (int s = 0; s < c->n_stages; ++s)
    for (int b = 0; b < c->blocks[s]; ++b, ++t) {
      const bool first = s > 0 && b == 0;
      LmxHieraBlock& B = blocks[t];
      B.dim = first ? c->dims[s - 1] : c->dims[s];
      B.D = c->dims[s];
      B.heads = c->heads[s];
      B.win = first ? c->windows[s - 1] : c->windows[s];
      for (int k = 0; k < c->n_global; ++k)
        if (c->global_blocks[k] == t) B.win = 0;
      B.qs = 0 < s && s <= c->q_pool_stages && b == 0 ? 2 : 0;
      stage_end[t] = b == c->blocks[s] - 1 ? s : -1;
    }
}

// lmx/sam.py FUSED_ATTN: the shape classes whose attention half is one kernel of csrc/hiera.hip, for which the encoder holds packed
// operands whatever a call's plan says -> LMX_HIERA_ATTN8 | LMX_HIERA_ATTN4 | LMX_HIERA_ATTN_POOL, or LMX_HIERA_LAUNCHES
inline int lmx_hiera_fused_attn(const LmxHieraBlock& b) {
  if (b.dim == 112 && b.D == 112 && b.heads == 2 && b.win == 8 && b.qs == 0) return LMX_HIERA_ATTN8;
  if (b.dim == 224 && b.D == 224 && b.heads == 4 && b.win == 4 && b.qs == 0) return LMX_HIERA_ATTN4;
  if (b.dim == 112 && b.D == 224 && b.heads == 4 && b.win == 8 && b.qs == 2) return LMX_HIERA_ATTN_POOL;
  if (b.dim == 224 && b.D == 448 && b.heads == 8 && b.win == 4 && b.qs == 2) return LMX_HIERA_ATTN_POOL;
  return LMX_HIERA_LAUNCHES;
}
