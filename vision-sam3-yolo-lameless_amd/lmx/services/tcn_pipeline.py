"""TCNPipeline — mirror of services/tcn-pipeline/app/main.py: the first consumer of `pipeline.tleap`.  The pose series of
`{id}_tleap.json` becomes 44 features per frame (20 keypoints relative to the bounding box, centroid, box area, centroid velocity),
centre-cropped or centre-padded to 125 steps; the TCN turns it into a severity score and an MC-dropout uncertainty, written to
`{id}_tcn.json` and published on `pipeline.tcn`.  `model.predict_with_uncertainty(x, n_samples=10)` (main.py:361: ten train-mode
forwards of about 45 launches each) is ONE launch of ``lmx.tcn.TcnScorer.score``, and ``process_videos`` scores a whole backlog of clips
in one launch.  The dropout bits are the library's (include/lmx.h), seeded per clip by ``lmx.tcn.clip_seed(video_id)`` — the first 8
bytes of the id's SHA-256, little-endian — so scoring a clip again gives the same bytes; parity with torch's generator is statistical."""
import numpy as np
import torch

from .. import tcn
from .gait_pipeline import GaitPipeline


class TCNPipeline(GaitPipeline):
    NAME, LABEL = "tcn", "TCN"

    def extract_features_from_tleap(self, tleap_data):
        """main.py:255-314: float32 [frames, 44], or None without pose_sequences.  The arithmetic is Python's (doubles) up to the cast;
        the velocity is the difference of the float32 centroid-x column."""
        pose_sequences = tleap_data.get("pose_sequences", [])
        return self._feature_matrix(pose_sequences) if pose_sequences else None

    def pad_or_truncate(self, features, target_length=125):
        """main.py:316-328: centre crop, or zero padding on both sides with the shorter half in front."""
        return self._centre(features, target_length, 0)

    def _clip(self, tleap_data):
        """(the padded series,) or None"""
        features = self.extract_features_from_tleap(tleap_data)
        if features is None or len(features) == 0:
            return None
        return (self.pad_or_truncate(features, target_length=self.TARGET_LENGTH),)

    def _score(self, video_ids, series):
        """(severity, uncertainty) per clip from ONE launch over the stacked series."""
        x = torch.from_numpy(np.ascontiguousarray(np.stack(series, 0), np.float32)).to(self.model.device)
        mean, std, _ = self.model.score(x, [tcn.clip_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        return mean.cpu().numpy(), std.cpu().numpy()

    def _results(self, video_id, features, severity_score, uncertainty):
        return {"video_id": video_id, "pipeline": "tcn", "severity_score": severity_score, "uncertainty": uncertainty,
                "prediction": int(severity_score > 0.5), "confidence": 1.0 - uncertainty, "input_frames": features.shape[0],
                "input_features": features.shape[1], "model_receptive_field": self.model.cfg.receptive_field}
