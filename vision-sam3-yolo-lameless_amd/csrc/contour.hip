// contour.hip — the contour features of services/sam3-pipeline/app/main.py:102-145 (cv2.findContours(RETR_EXTERNAL,
// CHAIN_APPROX_SIMPLE) -> largest contour by cv2.contourArea -> cv2.arcLength / cv2.boundingRect) ON THE DEVICE, for a
// batch of 1080p masks at once: the mask never leaves HBM, 64 bytes per frame do.
//
// host_mask.cpp follows each outer border pixel by pixel (Suzuki-Abe), which is sequential.  The same numbers have a
// parallel form.  Walk the boundary between an 8-connected foreground component C and the OUTSIDE background O (background
// 4-connected to the image frame) crack by crack — a crack = (foreground pixel c, side s) whose neighbour c + s is outside
// — with the foreground on the right.  At the end vertex of a crack, with A = the pixel ahead on the background side and
// B = the pixel straight ahead of c:   A foreground -> turn left,  the next crack belongs to A  (a DIAGONAL step c -> A);
// else B foreground -> go straight, the next crack belongs to B (a UNIT step c -> B);   else turn right around c (no step).
// The pixel sequence of that crack cycle is exactly the border Suzuki-Abe follows (pixels met twice on one-pixel-wide parts
// included), and every step is decided by the 2 x 2 neighbourhood of ONE crack.  So, per component,
//     2 * contourArea = | sum over cracks of (c.x * n.y - n.x * c.y) |,   arcLength = #unit + #diagonal * sqrt(2)
// are plain sums over cracks, exact in integers, in any order.  What is needed besides: labels (which component a pixel
// belongs to; which background is outside) — a union-find connected-component labelling whose root is the component's
// first pixel in raster order, which is also the contour order cv2.findContours' max(..., key=contourArea) breaks ties by.
//
// Kernels.  A SAM mask is a few blobs: connectivity, outside-ness and the crack sums are all decided at the ends of the
// horizontal RUNS of equal type (foreground / background) and where runs of adjacent rows overlap, so union-find nodes,
// labels and accumulators are per run, not per pixel (a 1080p frame has on the order of 10^4 runs on 2 * 10^6 pixels).
//   bit rows  : each row becomes ceil(w / 64) 64-bit words (bit x = pixel x is foreground; bits beyond w are 0).  A run
//               starts at the set bits of B = row ^ (row << 1) (carry across words; bit 0 of a row always set).  Per word
//               the number of runs that start before it in its row, per row the number of runs.
//   scan      : each row's first run id.  Node 0 is OUTSIDE; a frame's run ids start at 2, every row's first id is even.
//               Ids increase in raster order of the runs' first pixels, so "the smaller id wins" still makes a component's
//               root its first pixel in raster order; the runs of a row alternate in type, so id >> 1 is distinct among
//               the foreground runs of a frame: the accumulators are indexed by (id >> 1) - 1.
//   init      : label = own id; a background run on row 0, row h - 1 or at x = 0 is labelled OUTSIDE directly.
//   union     : a thread per word of a row, bit operations against the word above: one union per overlapping pair of runs
//               (foreground 8-connected, background 4-connected), lock-free union-find.  The row's last run, if background,
//               joins OUTSIDE here (the atomic lands on the run's own root, never on node 0).
//   compress  : every run's label becomes its root.
//   sums      : a thread per word; the N and S cracks of a foreground run are the bits of run & outside-above / -below,
//               their left / straight / right decisions are bit masks too, so a word's sums are popcounts; the W and E
//               cracks sit at the run's two ends.  Wave-reduced by root before any atomic.
//   select    : every root run of an EXTERNAL component bids for its frame; final writes the eight numbers.
// Every loop over the runs of a word is bounded by 64; the union-find retry loop is the one loop bounded by content only.
// Checked bit for bit against host_mask.cpp on analytic shapes, random blobs with salt-and-pepper and SAM masks
// (tests/test_gpu_contour.py) and at word edges, odd widths and unaligned masks (tests/test_gpu_contour_runs.py); cv2 itself
// is absent, so like the host version: PARITY UNPINNED against real OpenCV.
#include "common.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int pc(u64 v) { return __builtin_popcountll(v); }  // (HIP's __popcll is unsigned: sums of differences need int)
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* L, int i) {
  int p = ld(L + i);
  while (p != i) {
    i = p;
    p = ld(L + i);
  }
  return i;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + b, a);  // the larger root points to the smaller id
    if (old == b) return;
    b = old;  // somebody re-parented b meanwhile: continue from its new parent
  }
}

// the workspace, every array for all n frames; the 8-byte arrays come first so that none needs padding
struct Ws {
  u64* bits;        // [n][h][wpr] bit rows
  long long* area2; // [n][slots] sum of cross terms of a component, at the slot of its root run
  u64* steps;       // [n][slots] unit steps in the low 32 bits, diagonal steps in the high 32
  u64* best;        // [n] max over external roots of (|area2| << 21 | (0x1fffff - root pixel)): largest area, first in raster
                    //     order among equals
  int* box;         // [n][slots][4] min x, min y, max x, max y of the component's pixels that own a crack
  int* L;           // [n][cap] labels; [0] = OUTSIDE, [1] unused
  int* wpre;        // [n][h][wpr] runs of the row that start before this word
  int* rowbase;     // [n][h] run count of the row (bit rows kernel), then the id of its first run (scan kernel)
  int* count;       // [n] number of external contours
  int h, w, wpr;    // wpr = words per row
  int cap, slots;   // cap = 2 + h * (w rounded up to even) ids per frame, slots = cap / 2 - 1 foreground runs at most
};

// the bits of word k of a row that are pixels
__device__ __forceinline__ u64 valid_bits(int w, int wpr, int k) { return (k == wpr - 1 && (w & 63)) ? (1ull << (w & 63)) - 1 : ~0ull; }

// word k of a bit row with what its neighbours contribute
struct Word {
  u64 C, B;        // pixels; run starts
  unsigned cL, cR; // the pixel before bit 0 and the one after bit 63 (0 outside the frame)
  int first;       // id of the first run that starts in this word (the run of the pixel before bit 0 is first - 1)
};

__device__ __forceinline__ Word load_word(const Ws& ws, int64_t row, int k) {
  const u64* b = ws.bits + row * ws.wpr;
  Word r;
  r.C = b[k];
  r.cL = k > 0 ? (unsigned)(b[k - 1] >> 63) : 0u;
  r.cR = k + 1 < ws.wpr ? (unsigned)(b[k + 1] & 1) : 0u;
  const u64 prev = k > 0 ? (u64)r.cL : (~r.C & 1);
  r.B = (r.C ^ ((r.C << 1) | prev)) & valid_bits(ws.w, ws.wpr, k);
  r.first = ws.rowbase[row] + ws.wpre[row * ws.wpr + k];
  return r;
}

// id of the run pixel j of the word belongs to
__device__ __forceinline__ int run_at(const Word& r, int j) { return r.first + pc(r.B & ((2ull << j) - 1)) - 1; }
// bits j .. (next run start above j) - 1: the rest of j's run inside the word
__device__ __forceinline__ u64 run_rest(u64 B, int j) {
  const u64 nb = B & ~((2ull << j) - 1);
  return (nb ? (1ull << __builtin_ctzll(nb)) - 1 : ~0ull) & ~((1ull << j) - 1);
}

__device__ __forceinline__ void word_of(const Ws& ws, int64_t g, int& img, int& y, int& k) {
  k = (int)(g % ws.wpr);
  const int64_t t = g / ws.wpr;
  y = (int)(t % ws.h);
  img = (int)(t / ws.h);
}

// one workgroup per image row: bit words, runs per word (as a prefix inside the row) and runs of the row.  WORDS (w % 4 == 0,
// mask 4-byte aligned): a lane loads four pixels, 16 lanes OR their nibbles into a word; otherwise a lane loads one pixel and
// the wave's ballot is the word (one vector-memory instruction per 64 pixels instead of per 256).  Same bits either way.
template <bool WORDS>
__global__ __launch_bounds__(256) void run_bits_kernel(const uint8_t* __restrict__ mask, Ws ws, int64_t npix) {
  constexpr int PPT = WORDS ? 4 : 1;  // pixels per thread
  constexpr int LPW = 64 / PPT;       // lanes per word
  constexpr int WPI = 256 / LPW;      // words per iteration of the workgroup
  __shared__ int cnt[WPI];
  const int h = ws.h, w = ws.w, wpr = ws.wpr;
  const int row = blockIdx.x % h, img = blockIdx.x / h;
  const int64_t ri = (int64_t)img * h + row;
  const uint8_t* m = mask + (int64_t)img * npix + (int64_t)row * w;
  const int wi = threadIdx.x / LPW;
  int running = 0;
  for (int x0 = 0; x0 < w; x0 += 256 * PPT) {
    const int x = x0 + threadIdx.x * PPT;
    u64 word;
    if (WORDS) {
      const unsigned v = x < w ? *reinterpret_cast<const unsigned*>(m + x) : 0u;
      const unsigned nib = ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 2u : 0u) | ((v & 0xff0000u) ? 4u : 0u) | ((v & 0xff000000u) ? 8u : 0u);
      word = (u64)nib << (4 * (threadIdx.x & 15));
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) word |= __shfl_xor(word, o, 64);
    } else {
      word = __ballot(x < w && m[x] != 0);
    }
    const int k = x0 / 64 + wi;
    const bool leader = threadIdx.x % LPW == 0;
    if (leader) {
      int c = 0;
      if (k < wpr) {
        const u64 prev = k > 0 ? (u64)(m[64 * k - 1] != 0) : (~word & 1);
        c = pc((word ^ ((word << 1) | prev)) & valid_bits(w, wpr, k));
        ws.bits[ri * wpr + k] = word;
      }
      cnt[wi] = c;
    }
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WPI; ++i) {
      const int c = cnt[i];
      before += i < wi ? c : 0;
      all += c;
    }
    if (leader && k < wpr) ws.wpre[ri * wpr + k] = running + before;
    running += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) ws.rowbase[ri] = running;
}

// one workgroup per frame: rowbase[y] = 2 + sum over the rows above of their run count rounded up to even; per-frame init
__global__ __launch_bounds__(256) void run_scan_kernel(Ws ws) {
  __shared__ int part[256];
  const int img = blockIdx.x;
  int* rb = ws.rowbase + (int64_t)img * ws.h;
  int running = 2;
  for (int y0 = 0; y0 < ws.h; y0 += 256) {
    const int y = y0 + threadIdx.x;
    const int c = y < ws.h ? (rb[y] + 1) & ~1 : 0;
    part[threadIdx.x] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    if (y < ws.h) rb[y] = running + part[threadIdx.x] - c;
    running += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws.L[(int64_t)img * ws.cap] = 0;  // OUTSIDE
    ws.best[img] = 0;
    ws.count[img] = 0;
  }
}

// labels of the runs that start in a word; a foreground run also clears its accumulators
__global__ __launch_bounds__(256) void run_init_kernel(Ws ws, int n) {
  const int64_t total = (int64_t)n * ws.h * ws.wpr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    int img, y, k;
    word_of(ws, g, img, y, k);
    const Word c = load_word(ws, (int64_t)img * ws.h + y, k);
    int* Li = ws.L + (int64_t)img * ws.cap;
    const bool edge_row = y == 0 || y == ws.h - 1;
    int id = c.first;
    for (u64 b = c.B; b; b &= b - 1, ++id) {
      const int j = __builtin_ctzll(b);
      if ((c.C >> j) & 1) {
        Li[id] = id;
        const int64_t s = (int64_t)img * ws.slots + (id >> 1) - 1;
        ws.area2[s] = 0;
        ws.steps[s] = 0;
        ws.box[s * 4 + 0] = 0x7fffffff;
        ws.box[s * 4 + 1] = 0x7fffffff;
        ws.box[s * 4 + 2] = -1;
        ws.box[s * 4 + 3] = -1;
      } else {
        Li[id] = (edge_row || (k == 0 && j == 0)) ? 0 : id;
      }
    }
  }
}

// unions between the runs of a row and those of the row above, where they meet inside this word: same type vertically
// (foreground and background), foreground also diagonally (NW, NE) where that is not already implied
__global__ __launch_bounds__(256) void run_union_kernel(Ws ws, int n) {
  const int64_t total = (int64_t)n * ws.h * ws.wpr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    int img, y, k;
    word_of(ws, g, img, y, k);
    const int64_t ri = (int64_t)img * ws.h + y;
    const Word c = load_word(ws, ri, k);
    int* Li = ws.L + (int64_t)img * ws.cap;
    const u64 V = valid_bits(ws.w, ws.wpr, k);
    if (k == ws.wpr - 1 && y > 0 && y < ws.h - 1) {  // the row's last run ends at x = w - 1
      const int j = (ws.w - 1) & 63;
      if (!((c.C >> j) & 1)) uf_union(Li, run_at(c, j), 0);
    }
    if (y == 0) continue;
    const Word u = load_word(ws, ri - 1, k);
    // runs are already joined horizontally: a vertical union is only new where the pair starts a common stretch
    for (u64 b = ~(c.C ^ u.C) & (c.B | u.B) & V; b; b &= b - 1) {
      const int j = __builtin_ctzll(b);
      uf_union(Li, run_at(c, j), run_at(u, j));
    }
    const u64 Cl = (c.C << 1) | c.cL, Cr = (c.C >> 1) | ((u64)c.cR << 63);
    const u64 Ul = (u.C << 1) | u.cL, Ur = (u.C >> 1) | ((u64)u.cR << 63);
    // (the pixel beside a background pixel of the row above is in the neighbouring run: id -+ 1)
    for (u64 b = c.C & Ul & ~u.C & ~Cl; b; b &= b - 1) {
      const int j = __builtin_ctzll(b);
      uf_union(Li, run_at(c, j), run_at(u, j) - 1);
    }
    for (u64 b = c.C & Ur & ~u.C & ~Cr; b; b &= b - 1) {
      const int j = __builtin_ctzll(b);
      uf_union(Li, run_at(c, j), run_at(u, j) + 1);
    }
  }
}

// path compression over the runs
__global__ __launch_bounds__(256) void run_compress_kernel(Ws ws, int n) {
  const int64_t total = (int64_t)n * ws.h * ws.wpr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    int img, y, k;
    word_of(ws, g, img, y, k);
    const Word c = load_word(ws, (int64_t)img * ws.h + y, k);
    int* Li = ws.L + (int64_t)img * ws.cap;
    int id = c.first;
    for (u64 b = c.B; b; b &= b - 1, ++id) {
      const int r = uf_find(Li, id);
      if (r != id) __hip_atomic_store(Li + id, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // only ever shortens a path
    }
  }
}

// sum of the x coordinates of the set bits of m, bit 0 = pixel x0
__device__ __forceinline__ long long sum_x(u64 m, int x0) {
  const int s = pc(m & 0xaaaaaaaaaaaaaaaaull) + 2 * pc(m & 0xccccccccccccccccull) + 4 * pc(m & 0xf0f0f0f0f0f0f0f0ull) +
                8 * pc(m & 0xff00ff00ff00ff00ull) + 16 * pc(m & 0xffff0000ffff0000ull) + 32 * pc(m & 0xffffffff00000000ull);
  return (long long)x0 * pc(m) + s;
}

// the bits of `need` (background pixels of row r) whose run is labelled OUTSIDE: one label look-up per run
__device__ __forceinline__ u64 outside_bits(const int* __restrict__ Li, const Word& r, u64 need) {
  u64 out = 0;
  while (need) {
    const int j = __builtin_ctzll(need);
    const u64 seg = run_rest(r.B, j);
    if (Li[run_at(r, j)] == 0) out |= seg;
    need &= ~seg;
  }
  return out;
}

// crack sums.  A thread owns one word of a row and goes through its foreground runs; the wave takes them in step so that
// lanes whose runs share a root (the words along the border of one big mask) reduce before the atomic.
// With c = (x, y) and the step of the header comment to n, the cross term x * n.y - n.x * y of a crack is
//   N side (heading E): diagonal to (x+1, y-1): -(x + y)   unit to (x+1, y): -y
//   E side (heading S): diagonal to (x+1, y+1):   x - y    unit to (x, y+1):  x
//   S side (heading W): diagonal to (x-1, y+1):   x + y    unit to (x-1, y):  y
//   W side (heading N): diagonal to (x-1, y-1):   y - x    unit to (x, y-1): -x         and 0 for a turn around c.
__global__ __launch_bounds__(256) void run_sum_kernel(Ws ws, int n) {
  const int64_t total = (int64_t)n * ws.h * ws.wpr;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ll; base < total; base += nthreads) {
    const int64_t g = base + lane;
    Word c;
    c.C = c.B = 0;
    c.cL = c.cR = 0;
    c.first = 0;
    u64 U = 0, D = 0, outN = 0, outS = 0;
    unsigned uL = 0, uR = 0, dL = 0, dR = 0;
    int img = 0, y = 0, k = 0;
    const int* Li = ws.L;
    if (g < total) {
      word_of(ws, g, img, y, k);
      const int64_t ri = (int64_t)img * ws.h + y;
      c = load_word(ws, ri, k);
      Li = ws.L + (int64_t)img * ws.cap;
      if (c.C) {
        outN = outS = ~0ull;  // beyond the frame is outside
        if (y > 0) {
          const Word u = load_word(ws, ri - 1, k);
          U = u.C, uL = u.cL, uR = u.cR;
          outN = outside_bits(Li, u, c.C & ~U);
        }
        if (y < ws.h - 1) {
          const Word d = load_word(ws, ri + 1, k);
          D = d.C, dL = d.cL, dR = d.cR;
          outS = outside_bits(Li, d, c.C & ~D);
        }
      }
    }
    const int x0 = k * 64;
    const u64 Ur = (U >> 1) | ((u64)uR << 63), Cr = (c.C >> 1) | ((u64)c.cR << 63);
    const u64 Dl = (D << 1) | dL, Cl = (c.C << 1) | c.cL;
    u64 rem = c.C;  // foreground pixels of runs not yet taken
    while (__ballot(rem != 0)) {
      long long a2 = 0;
      unsigned long long st = 0;
      int root = -1, mnx = 0, mxx = 0;
      if (rem) {
        const int j = __builtin_ctzll(rem);
        const u64 G = run_rest(c.B, j) & c.C;  // the run inside this word (the last word's bits beyond w are not in C)
        rem &= ~G;
        const int e = 63 - __builtin_clzll(G);
        const int id = run_at(c, j);
        // the W crack sits at the run's first pixel, the E crack at its last: here only if the run starts / ends in this word
        const bool wout = ((c.B >> j) & 1) && (x0 + j == 0 || Li[id - 1] == 0);
        const bool eout = (e < 63 || !c.cR) && (x0 + e == ws.w - 1 || Li[id + 1] == 0);
        const u64 Nc = G & outN, Sc = G & outS;
        const u64 NA = Nc & Ur, NB = Nc & ~Ur & Cr, SA = Sc & Dl, SB = Sc & ~Dl & Cl;
        int unit = pc(NB) + pc(SB), diag = pc(NA) + pc(SA);
        a2 = sum_x(SA, x0) - sum_x(NA, x0) + (long long)y * (pc(SA) + pc(SB) - pc(NA) - pc(NB));
        u64 any = Nc | Sc;
        if (wout) {
          const int x = x0 + j;
          if (j > 0 ? (U >> (j - 1)) & 1 : uL) {
            a2 += y - x;
            ++diag;
          } else if ((U >> j) & 1) {
            a2 -= x;
            ++unit;
          }
          any |= 1ull << j;
        }
        if (eout) {
          const int x = x0 + e;
          if (e < 63 ? (D >> (e + 1)) & 1 : dR) {
            a2 += x - y;
            ++diag;
          } else if ((D >> e) & 1) {
            a2 += x;
            ++unit;
          }
          any |= 1ull << e;
        }
        if (any) {
          root = Li[id];
          st = (unsigned long long)unit | ((unsigned long long)diag << 32);
          mnx = x0 + __builtin_ctzll(any);
          mxx = x0 + 63 - __builtin_clzll(any);
        }
      }
      // most waves have no crack at all; a wave on the border of one big mask has cracks of ONE component: reduce, one atomic
      const bool has = root >= 0;
      const unsigned long long bal = __ballot(has);
      if (bal == 0) continue;
      const int first = __ffsll((long long)bal) - 1;
      const int root0 = __shfl(root, first, 64);
      const int img0 = __shfl(img, first, 64);
      // the lanes that share the first contributor's component reduce together (one atomic pair); the others — runs of
      // isolated noise pixels and small neighbours — add on their own, to addresses of their own
      const bool grp = has && root == root0 && img == img0;
      long long s2 = grp ? a2 : 0;
      unsigned long long ss = grp ? st : 0;
      int gnx = grp ? mnx : 0x7fffffff, gny = grp ? y : 0x7fffffff, gxx = grp ? mxx : -1, gxy = grp ? y : -1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s2 += __shfl_xor(s2, o, 64);
        ss += __shfl_xor(ss, o, 64);
        gnx = min(gnx, __shfl_xor(gnx, o, 64));
        gny = min(gny, __shfl_xor(gny, o, 64));
        gxx = max(gxx, __shfl_xor(gxx, o, 64));
        gxy = max(gxy, __shfl_xor(gxy, o, 64));
      }
      int64_t s = -1;
      if (lane == first) {
        s = (int64_t)img0 * ws.slots + (root0 >> 1) - 1;
      } else if (has && !grp) {
        s = (int64_t)img * ws.slots + (root >> 1) - 1;
        s2 = a2;
        ss = st;
        gnx = mnx;
        gxx = mxx;
        gny = gxy = y;
      }
      if (s >= 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(ws.area2 + s), (unsigned long long)s2);
        atomicAdd(ws.steps + s, ss);
        // the box only grows: an atomic that cannot grow it is skipped after a plain (possibly stale = less grown) look
        int* bb = ws.box + s * 4;
        const volatile int* vb = bb;
        if (gnx < vb[0]) atomicMin(bb + 0, gnx);
        if (gny < vb[1]) atomicMin(bb + 1, gny);
        if (gxx > vb[2]) atomicMax(bb + 2, gxx);
        if (gxy > vb[3]) atomicMax(bb + 3, gxy);
      }
    }
  }
}

// every root run of an EXTERNAL component (its west neighbour is outside background or the frame) bids for its frame
__global__ __launch_bounds__(256) void run_select_kernel(Ws ws, int n) {
  const int64_t total = (int64_t)n * ws.h * ws.wpr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    int img, y, k;
    word_of(ws, g, img, y, k);
    const Word c = load_word(ws, (int64_t)img * ws.h + y, k);
    const int* Li = ws.L + (int64_t)img * ws.cap;
    for (u64 b = c.B & c.C; b; b &= b - 1) {
      const int j = __builtin_ctzll(b);
      const int id = run_at(c, j);
      if (Li[id] != id) continue;  // roots only: the run of the component's first pixel in raster order
      const int x = k * 64 + j;
      if (!(x == 0 || Li[id - 1] == 0)) continue;
      long long a = ws.area2[(int64_t)img * ws.slots + (id >> 1) - 1];
      a = a < 0 ? -a : a;
      atomicMax(ws.best + img, ((unsigned long long)a << 21) | (unsigned long long)(0x1fffff - (y * ws.w + x)));
      atomicAdd(ws.count + img, 1);
    }
  }
}

// out[8] = area2 (>= 0), unit steps, diagonal steps, min x, min y, max x, max y, number of external contours
__global__ void contour_final_kernel(Ws ws, long long* __restrict__ out, int n) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n) return;
  long long* o = out + (int64_t)img * 8;
  if (ws.count[img] == 0) {
    for (int k = 0; k < 8; ++k) o[k] = 0;
    return;
  }
  const unsigned long long key = ws.best[img];
  const int r = 0x1fffff - (int)(key & 0x1fffffull);  // the winner's first pixel -> its run -> its slot
  const int y = r / ws.w, x = r - y * ws.w;
  const Word c = load_word(ws, (int64_t)img * ws.h + y, x >> 6);
  const int64_t s = (int64_t)img * ws.slots + (run_at(c, x & 63) >> 1) - 1;
  const unsigned long long st = ws.steps[s];
  o[0] = (long long)(key >> 21);
  o[1] = (long long)(st & 0xffffffffull);
  o[2] = (long long)(st >> 32);
  const int* bb = ws.box + s * 4;
  o[3] = bb[0];
  o[4] = bb[1];
  o[5] = bb[2];
  o[6] = bb[3];
  o[7] = ws.count[img];
}

inline unsigned grid_for(int64_t items) {
  int64_t b = (items + 255) / 256;
  if (b > 256 * 32) b = 256 * 32;
  return (unsigned)(b < 1 ? 1 : b);
}

// lays the arrays of Ws out from `base` on; returns the bytes used
inline int64_t ws_layout(Ws& ws, char* base, int n, int h, int w) {
  ws.h = h;
  ws.w = w;
  ws.wpr = (w + 63) / 64;
  ws.cap = 2 + h * ((w + 1) & ~1);
  ws.slots = ws.cap / 2 - 1;
  const int64_t words = (int64_t)n * h * ws.wpr, slots = (int64_t)n * ws.slots;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base + off;
    off += bytes;
    return p;
  };
  ws.bits = reinterpret_cast<u64*>(take(words * 8));
  ws.area2 = reinterpret_cast<long long*>(take(slots * 8));
  ws.steps = reinterpret_cast<u64*>(take(slots * 8));
  ws.best = reinterpret_cast<u64*>(take((int64_t)n * 8));
  ws.box = reinterpret_cast<int*>(take(slots * 16));
  ws.L = reinterpret_cast<int*>(take((int64_t)n * ws.cap * 4));
  ws.wpre = reinterpret_cast<int*>(take(words * 4));
  ws.rowbase = reinterpret_cast<int*>(take((int64_t)n * h * 4));
  ws.count = reinterpret_cast<int*>(take((int64_t)n * 4));
  return off;
}

}  // namespace

// Sized for ANY mask of the shape: a one-pixel checkerboard row has w runs.  Per frame and row: 12 bytes per 64-pixel word
// (bit row, run prefix), 4 for the row's first id, and per possible run (w rounded up to even) a 4-byte label and half a
// 32-byte accumulator; + 20 bytes per frame.  That is at most 36 bytes per pixel + 4 per frame for every h, w > 1; a mask of
// a few blobs touches only the front of the label and accumulator arrays.
extern "C" int64_t lmx_contour_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  Ws ws;
  return ws_layout(ws, nullptr, n, h, w);
}

extern "C" int lmx_k_contour_features(const uint8_t* mask, int n, int h, int w, int64_t* out, void* workspace, lmx_stream_t stream) {
  LMX_REQUIRE(mask && out && workspace, "lmx_k_contour_features: null pointer");
  // (the selection key packs the root pixel into 21 bits: 1080p = 2 073 600 pixels < 2^21)
  LMX_REQUIRE(n > 0 && h > 1 && w > 1 && (int64_t)h * w <= 0x1fffff && (int64_t)n * h < 0x7fffffffll && n <= 65535,
              "lmx_k_contour_features: n=%d h=%d w=%d (at most 2^21 - 1 pixels per mask)", n, h, w);
  LMX_REQUIRE(aligned16(workspace), "lmx_k_contour_features: workspace alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t npix = (int64_t)h * w;
  Ws ws;
  ws_layout(ws, reinterpret_cast<char*>(workspace), n, h, w);
  const unsigned rows = (unsigned)((int64_t)n * h), words = grid_for((int64_t)n * h * ws.wpr);
  // (which form reads the mask depends on the shape and the pointer only, and both write the same bits: a frame's result
  // does not depend on the batch it rides in)
  if (w % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0)  // rows then start on word boundaries
    hipLaunchKernelGGL(run_bits_kernel<true>, dim3(rows), dim3(256), 0, st, mask, ws, npix);
  else
    hipLaunchKernelGGL(run_bits_kernel<false>, dim3(rows), dim3(256), 0, st, mask, ws, npix);
  hipLaunchKernelGGL(run_scan_kernel, dim3(n), dim3(256), 0, st, ws);
  hipLaunchKernelGGL(run_init_kernel, dim3(words), dim3(256), 0, st, ws, n);
  hipLaunchKernelGGL(run_union_kernel, dim3(words), dim3(256), 0, st, ws, n);
  hipLaunchKernelGGL(run_compress_kernel, dim3(words), dim3(256), 0, st, ws, n);
  hipLaunchKernelGGL(run_sum_kernel, dim3(words), dim3(256), 0, st, ws, n);
  hipLaunchKernelGGL(run_select_kernel, dim3(words), dim3(256), 0, st, ws, n);
  hipLaunchKernelGGL(contour_final_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ws, reinterpret_cast<long long*>(out), n);
  return lmx_launch_check("contour_final_kernel");
}
