"""segment_anything's SamAutomaticMaskGenerator on liblmx (automatic_mask_generator.py and utils/amg.py of the public
segment_anything package): every mask of an image from a grid of single-point prompts.

Per crop (the whole image, plus the crops of `crop_n_layers`): set_image on the crop, then per batch of `points_per_batch`
points one decode of all three masks (MaskDecoder.decode_lowres: one image embedding, B prompt sets) and one
lmx_k_mask_score launch, which gives the stability counts, the area and the box of every candidate straight from its 256x256
low-res logits.  No full-resolution logit is materialised: `segment_anything` post-processes all 3B candidates to the frame
size first.  The filters run on the device, order-preserving (element-wise masks, no compaction).  lmx_k_nms_boxes then
keeps the crop's survivors.  The host syncs once per crop, when it reads the kept candidates.  Full-size masks (lmx_k_mask_post)
are made only for the records returned.  The generator's own launches run eagerly and it captures no HIP graph; the encoder
runs as LmxSamPredictor.set_image runs it (replayed from the predictor's graph cache once a crop shape repeats).

Where lmx pins a choice that segment_anything leaves to its libraries:
  * prompt coordinates: the crop's grid points are scaled to the resized input frame in float64
    (ResizeLongestSide.apply_coords) and handed to the decoder as f32; segment_anything keeps them in float64 up to the
    positional encoding (a difference below one f32 ulp of the coordinate);
  * stability score: count(v > thr + off) / count(v > thr - off) as the correctly rounded f32 quotient (0 / 0 = NaN);
  * NMS (box and crop stage): ties in the score go to the earlier candidate (a stable sort; torchvision leaves it open),
    IoU in f32 as torchvision's CPU kernel, compared in double;
  * order: candidates point-major with masks 1..3, batches in grid order, crops in generate_crop_boxes' order.
Not supported (both need libraries segment_anything imports for them): min_mask_region_area > 0 (cv2) and
output_mode="coco_rle" (pycocotools); both raise at construction."""
import itertools
import math

import numpy as np
import torch

from . import kernels as K

_OUTPUT_MODES = ("binary_mask", "uncompressed_rle", "coco_rle")


def build_point_grid(n_per_side):
    """segment_anything.utils.amg.build_point_grid: n x n points in [0,1]^2, offsets 1/(2n), x fastest (float64)."""
    offset = 1 / (2 * n_per_side)
    points_one_side = np.linspace(offset, 1 - offset, n_per_side)
    points_x = np.tile(points_one_side[None, :], (n_per_side, 1))
    points_y = np.tile(points_one_side[:, None], (1, n_per_side))
    return np.stack([points_x, points_y], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    """One grid per crop layer: int(n_per_side / scale_per_layer**i) points per side in layer i."""
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
    """segment_anything.utils.amg.generate_crop_boxes: ([x0, y0, x1, y1] ints, layer index) — the image, then per layer i
    (2^(i+1))^2 overlapping crops in product(x0s, y0s) order."""
    crop_boxes, layer_idxs = [[0, 0, im_size[1], im_size[0]]], [0]
    im_h, im_w = im_size
    short_side = min(im_h, im_w)

    def crop_len(orig_len, n_crops, overlap):
        return int(math.ceil((overlap * (n_crops - 1) + orig_len) / n_crops))

    for i_layer in range(n_layers):
        n_crops_per_side = 2 ** (i_layer + 1)
        overlap = int(overlap_ratio * short_side * (2 / n_crops_per_side))
        crop_w = crop_len(im_w, n_crops_per_side, overlap)
        crop_h = crop_len(im_h, n_crops_per_side, overlap)
        crop_box_x0 = [int((crop_w - overlap) * i) for i in range(n_crops_per_side)]
        crop_box_y0 = [int((crop_h - overlap) * i) for i in range(n_crops_per_side)]
        for x0, y0 in itertools.product(crop_box_x0, crop_box_y0):
            crop_boxes.append([x0, y0, min(x0 + crop_w, im_w), min(y0 + crop_h, im_h)])
            layer_idxs.append(i_layer + 1)
    return crop_boxes, layer_idxs


def mask_to_rle(mask):
    """segment_anything.utils.amg.mask_to_rle_pytorch for one bool [H,W] mask: uncompressed RLE in column-major order,
    starting with the run of zeros (0 when the first pixel is set)."""
    h, w = mask.shape
    flat = np.asarray(mask, bool).T.ravel()
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    idx = np.concatenate([[0], change, [h * w]])
    counts = [] if not flat[0] else [0]
    counts.extend(np.diff(idx).tolist())
    return {"size": [h, w], "counts": counts}


def rle_to_mask(rle):
    """segment_anything.utils.amg.rle_to_mask: uncompressed RLE -> bool [H,W]."""
    h, w = rle["size"]
    mask = np.empty(h * w, dtype=bool)
    idx, parity = 0, False
    for count in rle["counts"]:
        mask[idx:idx + count] = parity
        idx += count
        parity ^= True
    return mask.reshape(w, h).transpose()


def _near_crop_edge(boxes, crop_box, orig_box, atol=20.0):
    """is_box_near_crop_edge on the device: boxes int64 [n,4] in crop coordinates -> bool [n]."""
    crop_t = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)
    orig_t = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)
    x0, y0 = crop_box[0], crop_box[1]
    b = (boxes + torch.tensor([[x0, y0, x0, y0]], device=boxes.device)).float()
    near_crop = torch.isclose(b, crop_t[None, :], atol=atol, rtol=0)
    near_image = torch.isclose(b, orig_t[None, :], atol=atol, rtol=0)
    return torch.any(torch.logical_and(near_crop, ~near_image), dim=1)


def nms_any(boxes, scores, iou):
    """torchvision NMS (ties to the lower index) over any number of candidates: boxes f32 [n,4] on the device, scores f32 [n] on
    the host -> kept indices (host int64, in suppression order).  Up to K.NMS_BOXES_MAX candidates take one lmx_k_nms_boxes
    launch.  More are taken in their stable order of descending score, in chunks: each launch holds the boxes kept so far,
    ranked first, then as many next candidates as fit.  Kept boxes never suppress each other, so this is the greedy NMS over
    the whole set.  One host sync per launch."""
    scores = np.asarray(scores, np.float32)
    n = len(scores)
    if n == 0:
        return np.zeros((0,), np.int64)
    if n <= K.NMS_BOXES_MAX:
        keep, count = K.nms_boxes(boxes, torch.from_numpy(scores).to(boxes.device), iou)
        return keep[:int(count.cpu()[0])].cpu().numpy().astype(np.int64)
    order = np.argsort(-scores, kind="stable")
    kept = np.zeros((0,), np.int64)
    pos = 0
    while pos < n:
        room = K.NMS_BOXES_MAX - len(kept)
        if room <= 0:
            raise ValueError(f"NMS keeps more than {K.NMS_BOXES_MAX} boxes: lmx_k_nms_boxes cannot hold them with the next candidates")
        cand = np.concatenate([kept, order[pos:pos + room]])
        rank = -np.arange(len(cand), dtype=np.float32)                      # exact below 2^24: the order of `cand`
        idx = torch.from_numpy(cand).to(boxes.device)
        keep, count = K.nms_boxes(boxes[idx].contiguous(), torch.from_numpy(rank).to(boxes.device), iou)
        kept = cand[keep[:int(count.cpu()[0])].cpu().numpy().astype(np.int64)]
        pos += room
    return kept


class SamAutomaticMaskGenerator:
    """`segment_anything.SamAutomaticMaskGenerator(model, ...)`.  model: an LmxSam (what sam_model_registry returns) or an
    LmxSamPredictor (e.g. LmxSamPredictor.from_parts with a Hiera encoder).  generate(image HWC uint8 RGB) -> list of
    records {segmentation, area, bbox, predicted_iou, point_coords, stability_score, crop_box}, in NMS order."""

    def __init__(self, model, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                 stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0, crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500,
                 crop_n_points_downscale_factor=1, point_grids=None, min_mask_region_area=0, output_mode="binary_mask"):
        from .adapters import LmxSamPredictor

        if (points_per_side is None) == (point_grids is None):
            raise ValueError("Exactly one of points_per_side or point_grid must be provided.")
        if points_per_side is not None:
            grids = build_all_layer_point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
        else:
            grids = [np.asarray(g, np.float64) for g in point_grids]
            if len(grids) != crop_n_layers + 1:
                raise ValueError(f"point_grids holds {len(grids)} grids: crop_n_layers={crop_n_layers} needs {crop_n_layers + 1}")
            if any(g.ndim != 2 or g.shape[1] != 2 or g.shape[0] == 0 for g in grids):
                raise ValueError("each point grid must be a non-empty [N,2] array of (x, y) in [0,1]")
        if output_mode not in _OUTPUT_MODES:
            raise ValueError(f"Unknown output_mode {output_mode}.")
        if output_mode == "coco_rle":
            raise ValueError("output_mode='coco_rle' needs pycocotools, which lmx does not use: take 'uncompressed_rle' and "
                             "encode it with pycocotools.mask.frPyObjects")
        if min_mask_region_area > 0:
            raise ValueError("min_mask_region_area > 0 needs cv2's hole and island removal (segment_anything imports cv2 for it), "
                             "which lmx does not provide")
        if points_per_batch < 1:
            raise ValueError(f"points_per_batch must be >= 1, is {points_per_batch}")
        cap = max(g.shape[0] for g in grids) * 3
        if cap > K.NMS_BOXES_MAX:
            raise ValueError(f"{cap} candidate masks per crop: at most {K.NMS_BOXES_MAX} (points_per_side <= 73)")
        self.predictor = model if isinstance(model, LmxSamPredictor) else LmxSamPredictor(model)
        self.point_grids = grids
        self.points_per_batch = int(points_per_batch)
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode

    @property
    def mask_threshold(self):
        return getattr(self.predictor.model, "mask_threshold", 0.0)

    # ---- one crop ------------------------------------------------------------------------------------------------
    def _process_crop(self, image, crop_box, layer_idx, orig_size):
        """-> dict of host arrays for the crop's NMS survivors (in NMS order) and the device low-res logits they come from."""
        pr = self.predictor
        dec = pr.decoder
        x0, y0, x1, y1 = crop_box
        pr.set_image(np.ascontiguousarray(image[y0:y1, x0:x1, :]))
        ch, cw = pr.original_size
        nh, nw = pr.input_size
        points = self.point_grids[layer_idx] * np.array([[cw, ch]])                     # float64, crop pixels
        in_pts = torch.from_numpy(pr.transform.apply_coords(points, (ch, cw)).astype(np.float32)).to(pr.device)
        n_pts = points.shape[0]
        labels = torch.ones((n_pts, 1), dtype=torch.int32, device=pr.device)
        lowres, ious, stats = [], [], []
        for b0 in range(0, n_pts, self.points_per_batch):
            b1 = min(b0 + self.points_per_batch, n_pts)
            lr, iou = dec.decode_lowres(pr.features, (ch, cw), (nh, nw), points=in_pts[b0:b1, None].contiguous(),
                                        labels=labels[b0:b1], multimask=True, input_frame=True)
            flat = lr.view(-1, lr.shape[-2], lr.shape[-1])
            stats.append(K.mask_score(flat, dec.S, nh, nw, ch, cw, self.mask_threshold, self.stability_score_offset))
            lowres.append(flat)
            ious.append(iou.reshape(-1))
        iou = torch.cat(ious)
        st = torch.cat(stats)
        # stability score: the f64 quotient of two integers < 2^24 rounded to f32 is the correctly rounded f32 quotient
        stab = (st[:, 0].double() / st[:, 1].double()).float()
        boxes = st[:, 3:7]
        keep = torch.ones_like(iou, dtype=torch.bool)
        if self.pred_iou_thresh > 0.0:
            keep &= iou > self.pred_iou_thresh
        if self.stability_score_thresh > 0.0:
            keep &= stab >= self.stability_score_thresh
        keep &= ~_near_crop_edge(boxes, crop_box, [0, 0, orig_size[1], orig_size[0]])
        order, count = K.nms_boxes(boxes.float(), iou, self.box_nms_thresh, valid=keep)
        sel = order.long().clamp_min(0)
        packed = torch.cat([sel[:, None].double(), boxes[sel].double(), iou[sel].double()[:, None], stab[sel].double()[:, None],
                            count.double().expand(sel.shape[0])[:, None]], 1).cpu().numpy()      # the crop's one host sync
        k = int(packed[0, -1]) if packed.shape[0] else 0
        idx = packed[:k, 0].astype(np.int64)
        pb = self.points_per_batch * 3
        # keep the survivors' low-res logits only (the full-size masks of the records are made from them)
        kept = torch.stack([lowres[i // pb][i % pb] for i in idx.tolist()]) if k else None
        off = np.array([x0, y0, x0, y0], np.int64)
        return dict(idx=idx, boxes=packed[:k, 1:5].astype(np.int64) + off,
                    iou=packed[:k, 5].astype(np.float32), stab=packed[:k, 6].astype(np.float32),
                    points=points[idx // 3] + np.array([[x0, y0]], np.float64),
                    crop_box=crop_box, hw=(ch, cw), resized=(nh, nw), lowres=kept)

    def _masks(self, crop, sel, orig_size):
        """(full-size masks u8 [k,H,W] on the device, areas int64 [k]) of the crop's candidates `sel` (positions in its NMS
        order): lmx_k_mask_post on their low-res logits, placed at the crop's offset."""
        H, W = orig_size
        x0, y0, x1, y1 = crop["crop_box"]
        ch, cw = crop["hw"]
        nh, nw = crop["resized"]
        lr = crop["lowres"][torch.from_numpy(sel).to(crop["lowres"].device)].contiguous()
        m, stats = K.mask_post(lr, self.predictor.decoder.S, nh, nw, ch, cw)
        if (ch, cw) != (H, W):
            full = torch.zeros((m.shape[0], H, W), dtype=torch.uint8, device=m.device)
            full[:, y0:y1, x0:x1] = m
            m = full
        return m, stats[:, 0]

    # ---- the image -----------------------------------------------------------------------------------------------
    def generate(self, image):
        """image: HWC uint8 RGB -> list of record dicts (segment_anything's keys and types)."""
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"generate expects an HWC uint8 image, got {a.dtype} {a.shape}")
        orig_size = a.shape[:2]
        crop_boxes, layer_idxs = generate_crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        crops = [self._process_crop(a, cb, li, orig_size) for cb, li in zip(crop_boxes, layer_idxs)]
        self.predictor.reset_image()
        owner = np.concatenate([np.full(len(c["idx"]), j, np.int64) for j, c in enumerate(crops)])
        pos = np.concatenate([np.arange(len(c["idx"]), dtype=np.int64) for c in crops])
        boxes = np.concatenate([c["boxes"] for c in crops], 0)
        if len(crop_boxes) > 1 and len(owner):
            # scores = 1 / box_area(crop_boxes): the int64 area, reciprocal in f32 (torch's `1 / tensor`)
            cb = torch.tensor([crops[j]["crop_box"] for j in owner.tolist()])
            scores = (1 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))).to(torch.float32)
            dev = self.predictor.device
            keep = nms_any(torch.from_numpy(boxes.astype(np.float32)).to(dev), scores.numpy(), self.crop_nms_thresh)
            owner, pos, boxes = owner[keep], pos[keep], boxes[keep]
        # full-size masks, one mask_post launch per crop, in record order
        masks, areas = [None] * len(owner), np.zeros(len(owner), np.int64)
        for j, c in enumerate(crops):
            r = np.flatnonzero(owner == j)
            if len(r) == 0:
                continue
            m, a_ = self._masks(c, pos[r], orig_size)
            m, a_ = m.cpu().numpy().astype(bool), a_.cpu().numpy()
            for t, ri in enumerate(r.tolist()):
                masks[ri], areas[ri] = m[t], a_[t]
        records = []
        for i in range(len(owner)):
            c, p = crops[owner[i]], pos[i]
            bx = boxes[i]
            cb = c["crop_box"]
            records.append({
                "segmentation": masks[i] if self.output_mode == "binary_mask" else mask_to_rle(masks[i]),
                "area": int(areas[i]),
                "bbox": [int(bx[0]), int(bx[1]), int(bx[2] - bx[0]), int(bx[3] - bx[1])],
                "predicted_iou": float(c["iou"][p]),
                "point_coords": [c["points"][p].tolist()],
                "stability_score": float(c["stab"][p]),
                "crop_box": [int(cb[0]), int(cb[1]), int(cb[2] - cb[0]), int(cb[3] - cb[1])],
            })
        return records
