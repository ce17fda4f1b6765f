"""Host restatement of segment_anything's SamAutomaticMaskGenerator (automatic_mask_generator.py + utils/amg.py), in its
order of operations: full-resolution logits per batch, IoU filter, stability score, stability filter, threshold, box, edge
filter, per-crop NMS, uncrop, cross-crop NMS, records.  The helpers are transformers' restatements of segment_anything's
(models/sam/image_processing_pil_sam.py) where they are the same function; NMS is oracle.nms.torchvision_nms (stable ties).

decode_fn(points [B,2] float64 in crop pixels) -> (logits f32 [B,3,h,w] at crop resolution, iou f32 [B,3]) is the model
(or [B,4,..] / [B,4]: all four decoder masks, of which the generator takes 1..3):
authored analytic logits on the CPU, or the device decoder's lmx_k_mask_logits output on the GPU (the counts below are
integer reductions, exact on any device).  set_crop(crop_image) is called before a crop's batches (the crop encoder hook)."""
import numpy as np
import torch
from transformers.models.sam import image_processing_pil_sam as T

from oracle.nms import torchvision_nms


def point_grids(n_per_side, n_layers, scale):
    return [T._build_point_grid(int(n_per_side / (scale ** i))) for i in range(n_layers + 1)]


def crop_boxes(hw, n_layers, overlap_ratio):
    return T._generate_per_layer_crops(n_layers, overlap_ratio, hw)


def generate(image, decode_fn, set_crop=None, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88,
             stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0, crop_nms_thresh=0.7,
             crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1, point_grids_=None, mask_threshold=0.0,
             output_mode="binary_mask", defect=None, trace=None):
    """-> records as SamAutomaticMaskGenerator.generate.  defect (tests only): a named deviation from the reference.
    trace: optional dict filled with the candidate counts before / after each filter and the cross-crop NMS."""
    H, W = image.shape[:2]
    grids = point_grids_ if point_grids_ is not None else point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
    boxes_c, layers = crop_boxes((H, W), crop_n_layers, crop_overlap_ratio)
    all_ = dict(masks=[], boxes=[], iou=[], stab=[], points=[], crop=[])
    tr = trace if trace is not None else {}
    for k in ("cand", "after_iou", "after_stab", "after_edge", "after_nms", "before_cross", "after_cross"):
        tr.setdefault(k, 0)
    for crop_box, li in zip(boxes_c, layers):
        x0, y0, x1, y1 = crop_box
        crop = image[y0:y1, x0:x1]
        ch, cw = crop.shape[:2]
        if set_crop is not None:
            set_crop(crop)
        pts = grids[li] * np.array([[cw, ch]])
        cm, cb, ci, cs, cp = [], [], [], [], []
        for b0 in range(0, len(pts), points_per_batch):
            p = pts[b0:b0 + points_per_batch]
            logits, iou = decode_fn(p)
            logits = torch.as_tensor(logits)
            iou = torch.as_tensor(iou)
            if logits.shape[1] == 4:  # all four decoder masks: the generator takes 1..3 (multimask_output=True)
                sel = slice(0, 3) if defect == "masks_0_2" else slice(1, 4)
                logits, iou = logits[:, sel], iou[:, sel]
            masks = logits.flatten(0, 1)
            ious = iou.flatten(0, 1).to(torch.float32)
            points = torch.as_tensor(np.repeat(p, logits.shape[1], axis=0))
            tr["cand"] += masks.shape[0]
            if pred_iou_thresh > 0.0:
                keep = ious > pred_iou_thresh
                masks, ious, points = masks[keep], ious[keep], points[keep]
            tr["after_iou"] += masks.shape[0]
            if defect == "stability_ge":
                inter = (masks >= mask_threshold + stability_score_offset).sum((-1, -2), dtype=torch.int32)
                union = (masks >= mask_threshold - stability_score_offset).sum((-1, -2), dtype=torch.int32)
                stab = inter / union
            else:
                stab = T._compute_stability_score(masks, mask_threshold, stability_score_offset)
            if stability_score_thresh > 0.0:
                keep = stab >= stability_score_thresh
                masks, ious, points, stab = masks[keep], ious[keep], points[keep], stab[keep]
            tr["after_stab"] += masks.shape[0]
            masks = masks > mask_threshold
            boxes = T._batched_mask_to_box(masks)
            if defect == "exclusive_box_max":
                boxes = boxes + torch.tensor([0, 0, 1, 1]) * (masks.flatten(1).any(1)[:, None])
            if defect != "no_edge_filter":
                keep = ~T._is_box_near_crop_edge(boxes, crop_box, [0, 0, W, H])
                masks, ious, points, stab, boxes = masks[keep], ious[keep], points[keep], stab[keep], boxes[keep]
            tr["after_edge"] += masks.shape[0]
            cm.append(masks), cb.append(boxes), ci.append(ious), cs.append(stab), cp.append(points)
        masks, boxes, ious, stab, points = (torch.cat(v) for v in (cm, cb, ci, cs, cp))
        keep = _nms(boxes.float().numpy(), ious.numpy(), box_nms_thresh, defect)
        tr["after_nms"] += len(keep)
        masks, boxes, ious, stab, points = masks[keep], boxes[keep], ious[keep], stab[keep], points[keep]
        full = torch.zeros((masks.shape[0], H, W), dtype=torch.bool)
        full[:, y0:y1, x0:x1] = masks
        all_["masks"].append(full)
        all_["boxes"].append(boxes + torch.tensor([[x0, y0, x0, y0]]))
        all_["iou"].append(ious)
        all_["stab"].append(stab)
        all_["points"].append(points + torch.tensor([[x0, y0]]))
        all_["crop"].append(torch.tensor([crop_box] * masks.shape[0], dtype=torch.int64).reshape(-1, 4))
    d = {k: torch.cat(v) for k, v in all_.items()}
    tr["before_cross"] += len(d["boxes"])
    if len(boxes_c) > 1 and defect != "no_cross_crop_nms":
        cbx = d["crop"]
        scores = 1 / ((cbx[:, 2] - cbx[:, 0]) * (cbx[:, 3] - cbx[:, 1]))
        keep = _nms(d["boxes"].float().numpy(), scores.float().numpy(), crop_nms_thresh, defect)
        d = {k: v[keep] for k, v in d.items()}
    tr["after_cross"] += len(d["boxes"])
    rles = T._mask_to_rle(d["masks"]) if len(d["masks"]) else []
    out = []
    for i in range(len(rles)):
        b, c = d["boxes"][i], d["crop"][i]
        out.append({
            "segmentation": d["masks"][i].numpy() if output_mode == "binary_mask" else rles[i],
            "area": int(sum(rles[i]["counts"][1::2])),
            "bbox": [int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])],
            "predicted_iou": d["iou"][i].item(),
            "point_coords": [d["points"][i].tolist()],
            "stability_score": d["stab"][i].item(),
            "crop_box": [int(c[0]), int(c[1]), int(c[2] - c[0]), int(c[3] - c[1])],
        })
    return out


def _nms(boxes, scores, thr, defect):
    scores = np.asarray(scores, np.float32)
    if defect == "unstable_ties":  # ties to the LATER candidate
        n = len(scores)
        rev = torchvision_nms(boxes[::-1].copy(), scores[::-1].copy(), thr)
        return torch.as_tensor(n - 1 - rev, dtype=torch.long)
    if defect == "unsigned_score_bits":  # sort by the raw f32 bits as unsigned integers (negative scores above positive)
        key = scores.view(np.uint32).astype(np.float64)
        return torch.as_tensor(torchvision_nms(boxes, key.astype(np.float32), thr), dtype=torch.long)
    return torch.as_tensor(torchvision_nms(boxes, scores, thr), dtype=torch.long)


def records_equal(a, b):
    """Field-by-field equality of two record lists (order included); f32 scores compared as bits.  -> (ok, message)."""
    if len(a) != len(b):
        return False, f"{len(a)} records vs {len(b)}"
    for i, (r, s) in enumerate(zip(a, b)):
        for k in ("area", "bbox", "point_coords", "crop_box"):
            if r[k] != s[k]:
                return False, f"record {i} {k}: {r[k]} vs {s[k]}"
        for k in ("predicted_iou", "stability_score"):
            x, y = np.float32(r[k]), np.float32(s[k])
            if x.view(np.uint32) != y.view(np.uint32):
                return False, f"record {i} {k}: {r[k]!r} vs {s[k]!r}"
        sa, sb = r["segmentation"], s["segmentation"]
        if isinstance(sa, dict):
            if sa != sb:
                return False, f"record {i} rle differs"
        elif not np.array_equal(np.asarray(sa, bool), np.asarray(sb, bool)):
            return False, f"record {i} mask differs ({int(np.sum(np.asarray(sa) != np.asarray(sb)))} pixels)"
    return True, ""
