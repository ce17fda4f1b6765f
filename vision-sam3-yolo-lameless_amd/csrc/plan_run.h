// plan_run.h — how every native model (dino_model.hip, yolo_model.hip, sam_model.hip with sam_hiera_model.h) obtains the device memory
// of its launch plan.  The plan is host code written ONCE over a run: a counting run (prepare / open) walks it only to learn what it
// asks for — no kernel runs, every pointer it hands out is null — and a launching run walks the same code over the same offsets
// inside the workspace that count sized, so allocation order and launch order are one piece of code and cannot drift apart.
// A buffer is taken where the plan first writes it, with the size that launch uses; one of 2 GB or more is refused by name (the
// kernels walk an operand with 32-bit byte offsets, and for most launches nothing in the launcher checks it), and a launching run
// refuses what does not fit the prepared capacity.  HOST code only, and no HIP: a stream travels as lmx_stream_t, so a plain g++
// program can include this header (tests/plan_run_check_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lmx.h"

void lmx_set_error(const char* fmt, ...);  // api.hip

#define PLAN_REQUIRE(cond, ...)   \
  do {                            \
    if (!(cond)) {                \
      lmx_set_error(__VA_ARGS__); \
      return LMX_EINVAL;          \
    }                             \
  } while (0)

const int64_t LMX_MAX_BUFFER_BYTES = 0x7fffffffll;  // a buffer stays below this: the kernels index below 2 GB

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// a region of a workspace that hands out buffers front to back, each on a 256-byte boundary.  peak: the most that was ever taken,
// which is what a counting run is for; cap: what the launching run may take
struct LmxArena {
  char* base = nullptr;
  size_t at = 0, peak = 0, cap = 0;
};

// one walk of a plan: counting (launch false) or launching
struct LmxPlanRun {
  bool launch = false;
  const char* fn = "";                // the calling entry point, which opens every message
  const char* model = "";             // "the Hiera encoder": whose buffer a message names
  const char* kernels = "kernels";    // who indexes below 2 GB
  lmx_stream_t st = nullptr;

  // `bytes` of `a`: *out is null in a counting run
  int take(LmxArena* a, const char* what, int64_t bytes, void** out) const {
    *out = nullptr;
    PLAN_REQUIRE(bytes > 0 && bytes < LMX_MAX_BUFFER_BYTES, "%s: buffer '%s' of %s has %lld bytes, the %s index below 2 GB", fn, what, model,
                 (long long)bytes, kernels);
    const size_t need = up256((size_t)bytes);
    if (launch) {
      PLAN_REQUIRE(need <= a->cap && a->at <= a->cap - need, "%s: buffer '%s' of %s does not fit the prepared workspace", fn, what, model);
      *out = a->base + a->at;
    }
    a->at += need;
    if (a->at > a->peak) a->peak = a->at;
    return LMX_OK;
  }
  template <class T>
  int take(LmxArena* a, const char* what, int64_t bytes, T** out) const {
    return take(a, what, bytes, reinterpret_cast<void**>(out));
  }
  // an arena of its own as ONE region sized to the largest request and handed to every requester: for a buffer that a launch writes
  // and the launch right behind it consumes, so that one region serves them all in stream order
  template <class T>
  int share(LmxArena* a, const char* what, int64_t bytes, T** out) const {
    const int rc = take(a, what, bytes, out);
    rewind_to(a, 0);
    return rc;
  }
  // what was taken behind `mark` (an earlier a->at) is dead: the next take starts there.  The peak stays
  static void rewind_to(LmxArena* a, size_t mark) { a->at = mark; }
};

// a launch of the plan: enqueued by a launching run, skipped by a counting one
#define LMX_LAUNCH(R, call)                       \
  do {                                            \
    const int rc_ = (R).launch ? (call) : LMX_OK; \
    if (rc_ != LMX_OK) return rc_;                \
  } while (0)
