"""Pose series: the detector's outputs to tleap's pose records, the 125 x 44 series and the key-padding mask (services/tleap-pipeline
app/main.py:173-313 and :479-486) in ONE launch for a batch of clips (csrc/tleap.hip; include/lmx.h "Pose series" has the arithmetic).
``PoseSeries`` binds the kernel, or with ``backend="host"`` its plain C++ twin ``lmx_h_tleap_series`` without a GPU.  The series and the
mask stay on the device for ``TcnScorer`` / ``XfmScorer``; ``records`` downloads the pose records once.  There is no torch arithmetic
here.  The kernel is small and is not where a clip's time goes (the pose model is): what it buys is a frames-to-scores path without host
arithmetic, pinned bit for bit, usable from C and one launch per stage for a backlog of clips."""
import numpy as np
import torch

from . import kernels as K

# services/tleap-pipeline/app/main.py:210-263 — the names estimate_pose_from_bbox gives its 20 keypoints, in slot order
HEURISTIC_NAMES = [
    "left_eye", "right_eye", "nose", "left_ear", "right_ear", "left_front_elbow", "right_front_elbow", "left_back_elbow",
    "right_back_elbow", "left_front_knee", "right_front_knee", "left_back_knee", "right_back_knee", "left_front_paw", "right_front_paw",
    "left_back_paw", "right_back_paw", "throat", "withers", "tailbase",
]
RECORD = K.tleap_record_dtype()


class PoseSeries:
    """mode "trained" (keypoints of a pose model) or "heuristic" (boxes of a detector filtered by `cow_classes`)."""

    def __init__(self, mode, cow_classes=(19,), target=125, backend="device"):
        if mode not in ("trained", "heuristic") or backend not in ("device", "host"):
            raise ValueError(f"PoseSeries: mode {mode!r}, backend {backend!r}")
        self.mode, self.cow_classes, self.target, self.backend = mode, tuple(int(c) for c in cow_classes), int(target), backend

    def __call__(self, boxes, scores, cls, counts, kpts, hw, clip_first):
        """The detector's tensors for the frames of n clips (clip c: frames clip_first[c] .. clip_first[c + 1]) ->
        (rows i32 [n], records, series f32 [n, target, 44], mask uint8 [n, target]) where the operands are."""
        if (kpts is not None) != (self.mode == "trained"):
            raise K.LmxError(f"PoseSeries: mode {self.mode} {'needs' if kpts is None else 'takes no'} kpts")
        return K.tleap_series(boxes, scores, cls, counts, kpts, hw, clip_first, self.target, self.cow_classes, host=self.backend == "host")

    @staticmethod
    def records(rows, records, clip_first, max_det):
        """ONE download: per clip a numpy array of its rows[c] records (dtype RECORD)."""
        rec = records.cpu().numpy().view(RECORD).reshape(-1)
        counts = rows.cpu().numpy()
        return [rec[int(clip_first[c]) * max_det:int(clip_first[c]) * max_det + int(counts[c])] for c in range(len(counts))]
