// host_hiera_plan.cpp — the Hiera encoder's block plan on the HOST, the C++ twin of lmx/sam.py (which stays the restatement the tests
// pin; tests/test_hiera_plan_c_host.py holds this file to it field by field):
//   lmx_h_hiera_plan_rows   one record per block for n frames on given rows per block      = hiera_plan(cfg, n, rows, True, lowest, True)
//   lmx_h_hiera_plan        the rows per block for a frame geometry, settled, and their plan = HieraEncoder._settle(nh, nw, n, lowest)
// with the shape rules of lmx/kernels.py behind them (hiera_attn8_ok, hiera_attn4_ok, hiera_attn_pool_ok, pooled_gemm_ok,
// ln_mlp_img_ok, FUSED_MLP_WIDTHS) and lmx/sam.py's FUSED_ATTN and attn8_ln_inside.  It is the Python plan of an encoder built the
// default way (fused_mlp, proj_ln) with none of the LMX_* development switches set: this file reads no environment variable.
// No HIP call; integers only.
#include <stdint.h>

#include "../../include/lmx.h"
#include "hiera_bands.h"
#include "hiera_config.h"

#define HP_REQUIRE HIERA_REQUIRE

namespace {

typedef LmxHieraBlock Block;

int fused_attn(const Block& b) { return lmx_hiera_fused_attn(b); }

// lmx/kernels.py: the shapes each kernel is built for (the class is fused_attn's; what is left is whole windows on the grid)
bool attn8_ok(const Block& b, int H, int W) { return H % 8 == 0 && W % 8 == 0; }
bool attn4_ok(const Block& b, int H, int W) { return H % 4 == 0 && W % 4 == 0; }
bool attn_pool_ok(const Block& b, int H, int W) { return b.dim == 112 ? H % 8 == 0 && W % 8 == 0 : H % 4 == 0 && W % 4 == 0; }
bool pooled_gemm_ok(int64_t M, int N) { return M >= 512 && N >= 96 && N % 8 == 0; }
bool fused_mlp_width(int D) { return D == 112 || D == 224; }  // FUSED_MLP_WIDTHS; ln_mlp_img_ok takes both at every row count

int check_config(const lmx_hiera_config_t* c, int* n_blocks) { return lmx_hiera_check_config(c, "lmx_h_hiera_plan", n_blocks); }
void block_table(const lmx_hiera_config_t* c, Block* blocks, int* stage_end) { lmx_hiera_block_table(c, blocks, stage_end); }

int first_global_of(const Block* blocks, int nb) {
  for (int i = 0; i < nb; ++i)
    if (blocks[i].win == 0) return i;
  return -1;
}

// hiera_plan(cfg, n, rows, fused_mlp=True, lowest, proj_ln=True).  per: the rows per block, or NULL: `rows0` stage-1 rows in front of
// the first global block (a band, or the whole grid)
int plan_rows(const lmx_hiera_config_t* c, const Block* blocks, const int* stage_end, int nb, int n, int rows0, const int* per, int lowest,
              lmx_hiera_block_t* out) {
  const int g = c->image / 4;
  const int first_global = first_global_of(blocks, nb);
  int H = per ? per[0] : rows0, W = g, Hf = g;
  bool band = H < g;
  for (int i = 0; i < nb; ++i) {
    const Block& b = blocks[i];
    // one number: the band ends in front of the first global block, where every token sees every other
    const int need = per ? per[i] : band && i == first_global ? Hf : H;
    HP_REQUIRE(H <= need && need <= Hf, "lmx_h_hiera_plan_rows: block %d on %d rows, the block before left %d of %d", i, need, H, Hf);
    const int join = need > H ? H : 0;
    if (join) {
      H = need;
      band = need < Hf;
    }
    lmx_hiera_block_t& P = out[i];
    const int fused = fused_attn(b);
    P.shortcut = LMX_HIERA_SHORTCUT_NONE;
    P.query = LMX_HIERA_QUERY_NONE;
    if (fused == LMX_HIERA_ATTN8 && attn8_ok(b, H, W)) {
      P.attn = i == 0 ? LMX_HIERA_ATTN8_LN : LMX_HIERA_ATTN8;  // attn8_ln_inside(i, fused_mlp = True)
    } else if (fused == LMX_HIERA_ATTN_POOL && attn_pool_ok(b, H, W)) {
      P.attn = LMX_HIERA_ATTN_POOL;
    } else if (fused == LMX_HIERA_ATTN4 && attn4_ok(b, H, W)) {
      P.attn = LMX_HIERA_ATTN4;
    } else {
      // pooled: the GEMM writes the 2 x 2 max-pool of its product (the shortcut's; the q third's, k and v from a second launch)
      const bool pooled = b.qs && pooled_gemm_ok((int64_t)n * H * W, b.D);
      P.attn = LMX_HIERA_LAUNCHES;
      P.shortcut = b.dim == b.D ? LMX_HIERA_SHORTCUT_NONE : pooled ? LMX_HIERA_SHORTCUT_POOLED_GEMM : b.qs ? LMX_HIERA_SHORTCUT_GEMM_MAXPOOL : LMX_HIERA_SHORTCUT_GEMM;
      P.query = pooled ? LMX_HIERA_QUERY_POOLED_Q_KV : b.qs ? LMX_HIERA_QUERY_QKV_MAXPOOL : LMX_HIERA_QUERY_QKV;
    }
    P.ln1 = P.attn == LMX_HIERA_ATTN8_LN ? LMX_HIERA_LN1_KERNEL : LMX_HIERA_LN1_LAUNCH;
    if (i > 0 && out[i - 1].mlp != LMX_HIERA_MLP_LAUNCHES && P.attn != LMX_HIERA_ATTN8_LN) {
      out[i - 1].emit_ln1 = 1;
      if (!join) P.ln1 = LMX_HIERA_LN1_PREV;  // (behind a join those rows are the band's alone: dropped)
    }
    P.H = H, P.W = W, P.Hf = Hf;
    P.Ho = b.qs ? H / 2 : H, P.Wo = b.qs ? W / 2 : W, P.Hfo = b.qs ? Hf / 2 : Hf;
    P.join = join;
    P.window = b.win;
    P.mlp = fused_mlp_width(b.D) ? LMX_HIERA_MLP_IMG : LMX_HIERA_MLP_LAUNCHES;
    // stage 3 of Hiera-B+ after its opening block: the layer's choice, whatever the batch
    P.ln_out = P.attn == LMX_HIERA_LAUNCHES && P.mlp == LMX_HIERA_MLP_LAUNCHES && b.dim == 448 && b.D == 448 && !b.qs;
    P.emit_ln1 = 0;
    P.stage_end = stage_end[i] >= 0;
    P.keep = P.stage_end && stage_end[i] >= lowest;
    P.x16 = P.keep && P.mlp != LMX_HIERA_MLP_LAUNCHES;
    P.join_out = P.keep && band;
    P.clone = P.keep && !band && i + 1 < nb && blocks[i + 1].dim == blocks[i + 1].D;
    H = P.Ho, W = P.Wo, Hf = P.Hfo;
  }
  return LMX_OK;
}

// BlockPlan.choices(): what the band's constant rows depend on besides the weights
bool same_choices(const lmx_hiera_block_t& a, const lmx_hiera_block_t& b) {
  return a.attn == b.attn && a.ln1 == b.ln1 && a.shortcut == b.shortcut && a.query == b.query && a.ln_out == b.ln_out && a.mlp == b.mlp &&
         a.emit_ln1 == b.emit_ln1;
}

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int lmx_h_hiera_blocks(const lmx_hiera_config_t* config, int* n_blocks_host) {
  HP_REQUIRE(n_blocks_host, "lmx_h_hiera_blocks: null pointer");
  return check_config(config, n_blocks_host);
}

extern "C" int lmx_h_hiera_plan_rows(const lmx_hiera_config_t* config, int n, const int* rows_in_host, int lowest, lmx_hiera_block_t* records_host) {
  int nb = 0;
  if (const int rc = check_config(config, &nb)) return rc;
  HP_REQUIRE(rows_in_host && records_host, "lmx_h_hiera_plan_rows: null pointer");
  HP_REQUIRE(n > 0 && n <= 65535 && lowest >= 0, "lmx_h_hiera_plan_rows: n=%d lowest=%d", n, lowest);
  Block blocks[LMX_HIERA_MAX_BLOCKS];
  int stage_end[LMX_HIERA_MAX_BLOCKS];
  block_table(config, blocks, stage_end);
  return plan_rows(config, blocks, stage_end, nb, n, 0, rows_in_host, lowest, records_host);
}

extern "C" int lmx_h_hiera_plan(const lmx_hiera_config_t* config, int n, int nh, int nw, int lowest, lmx_hiera_block_t* records_host, int* rows_host) {
  int nb = 0;
  if (const int rc = check_config(config, &nb)) return rc;
  HP_REQUIRE(records_host && rows_host, "lmx_h_hiera_plan: null pointer");
  const int S = config->image, g = S / 4;
  HP_REQUIRE(n > 0 && n <= 65535 && lowest >= 0 && nh > 0 && nw > 0 && nh <= S && nw <= S, "lmx_h_hiera_plan: n=%d lowest=%d nh=%d nw=%d (image %d)", n,
             lowest, nh, nw, S);
  Block blocks[LMX_HIERA_MAX_BLOCKS];
  int stage_end[LMX_HIERA_MAX_BLOCKS], window[LMX_HIERA_MAX_BLOCKS], q_stride[LMX_HIERA_MAX_BLOCKS];
  block_table(config, blocks, stage_end);
  for (int i = 0; i < nb; ++i) window[i] = blocks[i].win, q_stride[i] = blocks[i].qs;
  lmx_hiera_bands_rows(window, q_stride, nb, g, nh, nw, rows_host);
  if (rows_host[0] == g)  // no band: the whole grid's plan
    return plan_rows(config, blocks, stage_end, nb, n, g, nullptr, lowest, records_host);
  // HieraEncoder._settle: the constant rows come from the whole-grid plan's kernels (one frame), so a block in the band must run
  // the kernel that plan chose: one whose shape check fails on the rule's rows gets rows added until it passes — up to the whole
  // grid, where it needs no constant rows.  (Every round adds rows to a block: it ends at the whole grid at the latest.)
  const int first_global = first_global_of(blocks, nb);  // >= 1: the rule found a band
  lmx_hiera_block_t whole[LMX_HIERA_MAX_BLOCKS];
  if (const int rc = plan_rows(config, blocks, stage_end, nb, 1, g, nullptr, 0, whole)) return rc;
  for (;;) {
    if (const int rc = plan_rows(config, blocks, stage_end, nb, n, 0, rows_host, lowest, records_host)) return rc;
    int bad = -1;
    for (int i = 0; i < first_global && bad < 0; ++i)
      if (records_host[i].H < records_host[i].Hf && !same_choices(records_host[i], whole[i])) bad = i;
    if (bad < 0) return LMX_OK;
    int64_t d = 0;
    for (int i = bad; i < first_global; ++i) {
      const int64_t w = blocks[i].win, two = blocks[i].qs ? 2 : 1, piece = w / gcd64(w, two) * two;
      const int64_t have = i == bad ? rows_host[i] + piece : rows_host[i];
      if (have > d) d = have;
      d = (d + piece - 1) / piece * piece;
      if (d > records_host[i].Hf) d = records_host[i].Hf;
      rows_host[i] = (int)d;
      if (blocks[i].qs) d /= 2;
    }
  }
}
