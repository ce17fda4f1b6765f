"""TransformerPipeline — mirror of services/transformer-pipeline/app/main.py:240-508, the TCN's twin on `pipeline.tleap`.  The pose
series of `{id}_tleap.json` becomes the TCN's 44 features per frame and a key-padding mask (a frame whose mean keypoint confidence times
its detection confidence is below 0.3 is masked), centre-cropped or centre-padded to 125 steps (padding is masked); the gait transformer
turns it into a severity score, an MC-dropout uncertainty and a temporal saliency, written to `{id}_transformer.json` and published on
`pipeline.transformer`.  `model.predict_with_uncertainty(x, mask, n_samples=10)` and `model.get_attention_weights(x)` (main.py:426-441:
eleven forwards of a few hundred launches each) are TWO launches of ``lmx.xfm.XfmScorer`` — S = 10 with the mask, eval mode without it
for the saliency, as main.py:435 passes none — and ``process_videos`` scores a whole backlog of clips in the same two launches.  The
dropout bits are the library's (include/lmx.h), seeded per clip by ``lmx.xfm.clip_seed(video_id)``; parity with torch's generator is
statistical.  A clip whose every step is masked has no defined score (torch gives NaN): it is refused and nothing is written."""
import numpy as np
import torch

from .. import xfm
from .gait_pipeline import GaitPipeline


class TransformerPipeline(GaitPipeline):
    NAME, LABEL = "transformer", "Transformer"
    MASK_BELOW = 0.3            # mean keypoint confidence x detection confidence
    SALIENCY_SHOWN = 20
    USES_MASK = True

    def extract_features_from_tleap(self, tleap_data):
        """main.py:303-372: (float32 [frames, 44], bool [frames], True = masked), or (None, None) without pose_sequences.  The
        features are the TCN's; the confidence of a frame is np.mean over its 20 keypoint confidences (0.5 where a keypoint has none, 0
        for a missing keypoint) times the detection confidence, cast to float32."""
        pose_sequences = tleap_data.get("pose_sequences", [])
        if not pose_sequences:
            return None, None
        confidences = []
        for frame in pose_sequences:
            conf = [kp.get("confidence", 0.5) for kp in frame.get("keypoints", [])[:self.NUM_KEYPOINTS]]
            conf += [0.0] * (self.NUM_KEYPOINTS - len(conf))
            confidences.append(np.mean(conf) * frame.get("detection_confidence", 1.0))
        return self._feature_matrix(pose_sequences), np.array(confidences, dtype=np.float32) < np.float32(self.MASK_BELOW)

    def pad_or_truncate(self, features, mask, target_length=125):
        """main.py:374-392: centre crop, or padding on both sides with the shorter half in front: zeros for the features, True for the mask."""
        return self._centre(features, target_length, 0), self._centre(mask, target_length, True)

    def _clip(self, tleap_data):
        """(padded series, padded mask) or None"""
        features, mask = self.extract_features_from_tleap(tleap_data)
        if features is None or len(features) == 0:
            return None
        return self.pad_or_truncate(features, mask, target_length=self.TARGET_LENGTH)

    def _features(self, video_id):
        """As the base, and None where every step is masked"""
        clip = super()._features(video_id)
        if clip is not None and clip[1].all():
            print(f"  Every step of {video_id} is masked (low confidence): no score")
            return None
        return clip

    def _accept(self, video_id, clip):
        """As the base, with the refusal of _features"""
        if clip[1].all():
            print(f"  Every step of {video_id} is masked (low confidence): no score")
            return None
        return super()._accept(video_id, clip)

    def _score(self, video_ids, series, masks):
        """(severity, uncertainty, saliency) per clip from TWO launches over the stacked series"""
        x = torch.from_numpy(np.ascontiguousarray(np.stack(series, 0), np.float32)).to(self.model.device)
        m = torch.from_numpy(np.ascontiguousarray(np.stack(masks, 0)).astype(np.uint8)).to(self.model.device)
        mean, std, _ = self.model.score(x, m, [xfm.clip_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        return mean.cpu().numpy(), std.cpu().numpy(), self.model.saliency(x).cpu().numpy()

    def _results(self, video_id, features, mask, severity_score, uncertainty, saliency):
        temporal_saliency = [float(v) for v in saliency]
        cfg = self.model.cfg
        return {"video_id": video_id, "pipeline": "transformer", "severity_score": severity_score, "uncertainty": uncertainty,
                "prediction": int(severity_score > 0.5), "confidence": 1.0 - uncertainty, "input_frames": features.shape[0],
                "input_features": features.shape[1], "masked_frames": int(mask.sum()),
                "temporal_saliency": temporal_saliency[:self.SALIENCY_SHOWN] if len(temporal_saliency) > self.SALIENCY_SHOWN else temporal_saliency,
                "model_info": {"d_model": cfg.d_model, "num_layers": cfg.n_layers, "nhead": cfg.n_heads}}
