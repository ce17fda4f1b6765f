// sam_lanes.h — a SAM handle's workspace LANES: what csrc/fused_model.hip needs of csrc/sam_model.hip beyond the public lmx_sam_* calls.
// A lmx_sam handle owns one workspace per prepared (frame size, plan), which is why the public calls allow ONE stream in flight per
// handle.  The fused step keeps several SAM passes in flight (lmx/pipeline.py: a HIP stream per pass), so a handle can hold further
// workspaces — lanes 1 .. — over the SAME weight upload.  The public calls keep lane 0 and their rule.  A lane is only ever used on one
// stream, so a later pass on it is ordered behind the earlier one by the stream itself, without events.
// A pass is split where the fused step waits for YOLO: the encoder (into the lane's embedding buffer) needs no box, the decoder does,
// and it reads the top box of each frame straight from YOLO's boxes [n][max_det][4] through the row stride ldb (floats), as
// MaskDecoder.predict reads boxes[i:i + chunk, 0, :].
// HOST functions with C++ linkage, internal to the library (not in include/lmx.h); errors as everywhere (LMX_EINVAL / LMX_EHIP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmx.h"

const int LMX_SAM_MAX_LANES = 16;

// SYNCHRONOUS: lane 0 as lmx_sam_prepare builds it (same checks, same messages) and lanes 1 .. lanes - 1 beside it; lanes already there are kept
int lmx_sam_lanes_prepare(lmx_sam* m, int h, int w, int precision, int lanes);
// 1 if `lanes` lanes of (h, w, precision) are prepared, else 0; no allocation, no error text
int lmx_sam_lanes_ready(const lmx_sam* m, int h, int w, int precision, int lanes);
// enqueue-only, on a prepared lane: lmx_sam_encode of n <= max_batch frames into the lane's embedding buffer
int lmx_sam_lane_encode(lmx_sam* m, int lane, const uint8_t* frames, int n, int h, int w, int precision, hipStream_t st);
// enqueue-only: lmx_sam_decode of the lane's embedding with frame i's box at boxes + i * ldb; mask_bits and contour may be NULL
int lmx_sam_lane_decode(lmx_sam* m, int lane, int n, int h, int w, const float* boxes, int64_t ldb, int precision, uint8_t* mask_bits, int64_t* stats,
                        int64_t* contour, float* iou, hipStream_t st);
