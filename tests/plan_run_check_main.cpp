// plan_run_check_main.cpp — csrc/plan_run.h, the walker under every native model's workspace, on a toy plan: a stand-alone program for
// tests/test_plan_run_sanitized.py, which builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it on the CPU.  The
// launching walk writes every buffer it is handed, end to end, into a heap block of exactly the counted size, so a wrong offset is
// a report.  Exit 0 and "ok" if every check holds; otherwise the failed checks on stderr and exit 1.
#include "check_main.h"

#include "../vision-sam3-yolo-lameless_amd/csrc/plan_run.h"

static int g_failed = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_error);  \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

struct Toy : LmxPlanRun {
  LmxArena keep, tmp, one;
  std::vector<size_t> offs;  // where each buffer lies in its arena, in the plan's order
  std::vector<int64_t> shared;  // the requests to `one`
};

// a buffer of the plan: its offset is noted, and a launching run fills it
static int buffer(Toy& R, LmxArena* a, const char* what, int64_t bytes, bool share) {
  char* p;
  R.offs.push_back(a->at);
  const int rc = share ? R.share(a, what, bytes, &p) : R.take(a, what, bytes, &p);
  if (rc != LMX_OK) return rc;
  if (share) R.shared.push_back(bytes);
  if (R.launch != (p != nullptr)) return LMX_EINVAL;
  if (p) memset(p, 0x5a, (size_t)bytes);
  return LMX_OK;
}

static const int64_t ROWS[3] = {2 * 333, 9 * 333, 333}, HIDDEN[3] = {777, 2 * 777, 3 * 777};  // per frame: the middle block is the largest

// three blocks: what a block keeps outlives it, what it takes from `tmp` dies with it (rewind), `one` serves three requests
static int plan(Toy& R, int n) {
  const int64_t shared[3] = {700, 5000, 1200};
  int rc = buffer(R, &R.keep, "stream", (int64_t)n * 1000, false);
  for (int i = 0; i < 3 && rc == LMX_OK; ++i) {
    R.rewind_to(&R.tmp, 0);
    rc = buffer(R, &R.tmp, "rows", n * ROWS[i], false);
    if (rc == LMX_OK) rc = buffer(R, &R.tmp, "hidden", n * HIDDEN[i], false);
    if (rc == LMX_OK) rc = buffer(R, &R.one, "operand", shared[i] * n, true);
    if (rc == LMX_OK) rc = buffer(R, &R.keep, "kept", (int64_t)n * 100 + i, false);
  }
  return rc;
}

int main() {
  const int n = 3;
  Toy count;
  count.fn = "toy_prepare", count.model = "the toy";
  CHECK(plan(count, n) == LMX_OK);
  // the peak across the rewinds: the largest block, not the last one and not the sum
  size_t want_tmp = 0;
  for (int i = 0; i < 3; ++i) {
    const size_t block = up256((size_t)(n * ROWS[i])) + up256((size_t)(n * HIDDEN[i]));
    if (block > want_tmp) want_tmp = block;
  }
  CHECK(count.tmp.peak == want_tmp && count.tmp.at < count.tmp.peak);
  CHECK(count.keep.peak == count.keep.at);
  // the largest-request region is the maximum of its requests
  CHECK(count.one.peak == up256((size_t)5000 * n) && count.one.at == 0 && count.shared.size() == 3);
  for (size_t o : count.offs) CHECK(o % 256 == 0);

  // the launching walk: the same offsets, and it ends exactly at the counted peak
  Toy run;
  run.launch = true, run.fn = "toy_run", run.model = "the toy";
  LmxArena* counted[3] = {&count.keep, &count.tmp, &count.one};
  LmxArena* mine[3] = {&run.keep, &run.tmp, &run.one};
  std::vector<std::vector<char>> heap(3);
  for (int i = 0; i < 3; ++i) {
    heap[i].resize(counted[i]->peak);  // exactly: one byte more in a take is a heap overflow
    mine[i]->base = heap[i].data(), mine[i]->cap = counted[i]->peak;
  }
  CHECK(plan(run, n) == LMX_OK);
  CHECK(run.offs == count.offs);
  for (int i = 0; i < 3; ++i) CHECK(mine[i]->peak == counted[i]->peak);
  CHECK(run.keep.at == count.keep.peak);
  // a smaller chunk fits what the full one counted
  Toy small = run;
  small.offs.clear();
  for (LmxArena* a : {&small.keep, &small.tmp, &small.one}) a->at = 0;
  CHECK(plan(small, 1) == LMX_OK);

  // refusals: nothing is handed out and `at` stays
  char* p = reinterpret_cast<char*>(&run);
  const size_t at = run.keep.at;
  for (int64_t bad : {(int64_t)0, (int64_t)-5, (int64_t)0x7fffffff, (int64_t)0x80000000ll, (int64_t)1 << 40}) {
    g_error[0] = 0;
    CHECK(count.take(&count.keep, "the big one", bad, &p) == LMX_EINVAL && p == nullptr);
    CHECK(strstr(g_error, "toy_prepare: buffer 'the big one' of the toy") && strstr(g_error, "index below 2 GB"));
  }
  CHECK(count.take(&count.keep, "just below", 0x7ffffffell, &p) == LMX_OK);
  g_error[0] = 0;
  CHECK(run.take(&run.keep, "one more", 1, &p) == LMX_EINVAL && p == nullptr && run.keep.at == at);
  CHECK(strstr(g_error, "toy_run: buffer 'one more' of the toy does not fit the prepared workspace"));
  run.rewind_to(&run.tmp, 0);
  CHECK(run.take(&run.tmp, "too large", (int64_t)run.tmp.cap + 1, &p) == LMX_EINVAL && p == nullptr && run.tmp.at == 0);
  CHECK(run.take(&run.tmp, "all of it", (int64_t)run.tmp.cap, &p) == LMX_OK && p == run.tmp.base && run.tmp.at == run.tmp.cap);
  CHECK(run.share(&run.one, "too large", (int64_t)run.one.cap + 1, &p) == LMX_EINVAL && p == nullptr && run.one.at == 0);
  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}
