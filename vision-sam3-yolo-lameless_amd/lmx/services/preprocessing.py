"""VideoPreprocessor — mirror of services/video-preprocessing/app/main.py:39-149, the step in front of all three pipelines: YOLO on
the first 10 frames, the median box of the large detections, 50 px of padding, the crop of every frame, and the `video.preprocessed`
message.  The reference cuts the window out with moviepy, re-encodes it with libx264 and lets every consumer decode that file again;
here the crop is a WINDOW of the original decode:

  * on the ingest side `lmx.kernels.yuv420_to_bgr_roi` / `NativeFused.step_yuv_roi` convert only the window of the decoder's NV12 / I420
    frames, at any parity of the box, so the pipelines can run on the original decode and skip the re-encode and the second decode;
  * on the egress side `lmx.kernels.bgr_to_yuv420` turns the window of BGR frames (a strided view: no copy) into the NV12 / I420 planes
    an encoder takes — `cropped()` is what the caller would hand to libx264 or a hardware encoder.

Decoding, mp4 writing and NATS stay with the caller, as in curation.

One documented departure: libx264 refuses odd yuv420p sizes, so for a box with an odd side the reference's write fails and it publishes
nothing (main.py:151-154).  `encoder_box` shrinks x2 / y2 by one where a side is odd, and `cropped()` encodes that box."""
import numpy as np

SAMPLE_FRAMES = 10  # main.py:67
MODEL_CONF = 0.25  # self.yolo_model(frame, verbose=False): the model's default confidence (main.py:75)
BOX_CONF = 0.5  # box.conf[0] > 0.5 (main.py:83)
AREA_FRACTION = 0.1  # w * h > width * height * 0.1 (main.py:87)
PADDING = 50  # main.py:106


def crop_box_of(boxes, width, height, pad=PADDING):
    """main.py:85-110 on the boxes that passed the confidence rule, [k, 4] xyxy float32 in frame pixels, every class: kept are the boxes
    whose float32 area is STRICTLY above width * height * 0.1 (compared as doubles); per column np.median over the float32 values (an
    even count averages the two middle values, in float32), int() truncation, the padding, the clamp to the frame; the full frame when
    nothing is kept.  lmx_h_crop_box (csrc/host_crop.cpp) is the same arithmetic in C."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    kept = []
    for x1, y1, x2, y2 in b:
        w, h = x2 - x1, y2 - y1  # float32, as box.xyxy[0].cpu().numpy()'s scalars
        if float(w * h) > (width * height * AREA_FRACTION):
            kept.append([x1, y1, x2, y2])
    if not kept:
        return [0, 0, int(width), int(height)]
    k = np.array(kept)  # float32 [m, 4]
    box = [int(np.median(k[:, i])) for i in range(4)]
    return [max(0, box[0] - pad), max(0, box[1] - pad), min(int(width), box[2] + pad), min(int(height), box[3] + pad)]


def confident_boxes(boxes, scores, counts, conf=BOX_CONF):
    """the detector's tables ([n, max_det, 4], [n, max_det], [n]) -> float32 [k, 4]: the boxes of main.py:79-83 in its order (frame by
    frame, detection by detection) whose confidence is above `conf`"""
    boxes, scores, counts = (np.asarray(t) for t in (boxes, scores, counts))
    out = [boxes[i, j] for i in range(boxes.shape[0]) for j in range(int(counts[i])) if scores[i, j] > conf]
    return np.asarray(out, dtype=np.float32).reshape(-1, 4)


def encoder_box(crop_box):
    """the box an encoder can take: x2 / y2 lowered by one where a side is odd (4:2:0 frames have even sizes).  A documented departure:
    for such a box the reference's libx264 write fails and nothing is published."""
    x1, y1, x2, y2 = (int(v) for v in crop_box)
    return [x1, y1, x2 - ((x2 - x1) & 1), y2 - ((y2 - y1) & 1)]


def message(video_id, input_path, output_path, crop_box, fps, total_frames):
    """the `video.preprocessed` payload of main.py:135-144, key for key (pass encoder_box(crop_box) where the file was written from
    cropped(): width and height are then the file's)"""
    return {
        "video_id": video_id,
        "original_path": str(input_path),
        "processed_path": str(output_path),
        "crop_box": crop_box,
        "fps": fps,
        "width": crop_box[2] - crop_box[0],
        "height": crop_box[3] - crop_box[1],
        "total_frames": total_frames,
    }


class VideoPreprocessor:
    """process_video of the reference (main.py:39-149) from frames in HBM to the crop box, the cropped frames as an encoder takes them
    and the message; the caller owns decode, encode and I/O."""

    def __init__(self, detector, model_conf=MODEL_CONF, box_conf=BOX_CONF):
        """model_conf, box_conf: the reference's two thresholds (the model's default 0.25, then `conf > 0.5`); a custom-trained detector
        may want others"""
        self.detector, self.model_conf, self.box_conf = detector, model_conf, box_conf

    def detections(self, frames):
        """the detector's (boxes, scores, counts) numpy tables on the first min(10, n) frames at the model's confidence"""
        boxes, scores, _, _, counts = self.detector.detect(frames[:SAMPLE_FRAMES], conf=self.model_conf)
        return boxes.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()

    def crop_box(self, frames, width, height):
        """frames: u8 BGR [n,h,w,3] on the detector's device; width, height: the clip's (cap.get's integers) -> [x1, y1, x2, y2]
        (main.py:65-110): one batched detect over the sampled frames, three small tables to the host, crop_box_of on them"""
        if frames.shape[0] == 0:  # total_frames = 0: no frame is read, nothing is detected
            return [0, 0, int(width), int(height)]
        return crop_box_of(confident_boxes(*self.detections(frames), conf=self.box_conf), width, height)

    encoder_box = staticmethod(encoder_box)
    message = staticmethod(message)

    def cropped(self, frames_or_yuv, crop_box, layout="nv12", matrix="bt601"):
        """what an encoder takes for the clip cropped to encoder_box(crop_box): (y, c) for nv12 or (y, u, v) for i420, uint8 device
        tensors (lmx.kernels.bgr_to_yuv420).  frames_or_yuv: BGR u8 [n,h,w,3] on the device — its window is converted where it lies,
        without a copy — or the decoder's planes as a tuple, (y, c) for nv12 or (y, u, v) for i420, each sliced to the frame's size
        ([n,h,w] and [n,h/2,w] or [n,h/2,w/2]; pitches are the strides), in the layout and matrix given — then the window is converted to
        BGR first (lmx.kernels.yuv420_to_bgr_roi: the box has any parity, a 4:2:0 plane cannot be cut at an odd pixel) and back."""
        from .. import kernels as K

        x1, y1, x2, y2 = encoder_box(crop_box)
        if isinstance(frames_or_yuv, (tuple, list)):
            y, c = frames_or_yuv[0], frames_or_yuv[1]
            v = frames_or_yuv[2] if len(frames_or_yuv) > 2 else None
            h, w = int(y.shape[-2]), int(y.shape[-1])
            bgr = K.yuv420_to_bgr_roi(y, c, h, w, (x1, y1, x2 - x1, y2 - y1), layout=layout, matrix=matrix, v=v)
        else:
            bgr = frames_or_yuv[:, y1:y2, x1:x2]
        return K.bgr_to_yuv420(bgr, layout=layout, matrix=matrix)
