"""tests/amgref.py and lmx.amg's host helpers on the CPU: the helpers agree with transformers' restatements of
segment_anything's, an authored end-to-end case gives its hand-derived records, and each modelled defect changes them."""
import numpy as np
import pytest
import torch
from transformers.models.sam import image_processing_pil_sam as T

import amgref
from lmx import amg
from lmx.adapters import ResizeLongestSide

H, W = 64, 96
# authored objects (inclusive pixel rectangles or discs), each with the IoU score its masks are given
OBJECTS = [
    dict(kind="rect", x=(6, 20), y=(2, 28), iou=0.9),      # holds grid points 0 and 4: a score tie NMS must resolve
    dict(kind="disc", c=(60, 40), r=9, iou=0.95),
    dict(kind="rect", x=(76, 95), y=(48, 63), iou=0.8),    # touches the right and bottom image edges
    dict(kind="rect", x=(30, 44), y=(18, 30), iou=0.85),
]


def _inside(o, xs, ys):
    if o["kind"] == "rect":
        return (xs >= o["x"][0]) & (xs <= o["x"][1]) & (ys >= o["y"][0]) & (ys <= o["y"][1])
    return (xs - o["c"][0]) ** 2 + (ys - o["c"][1]) ** 2 <= o["r"] ** 2


def _erode(m):
    e = m.copy()
    e[1:, :] &= m[:-1, :]
    e[:-1, :] &= m[1:, :]
    e[:, 1:] &= m[:, :-1]
    e[:, :-1] &= m[:, 1:]
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = False
    return e


def _image():
    """An image whose pixels carry their own coordinates (channel 0 = x, 1 = y): the crop hook reads a crop's offset."""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys, np.zeros_like(xs)], -1).astype(np.uint8)


class Authored:
    """decode_fn: masks 0..3 for a point inside object O: 0 the whole frame (+4, score 0.99), 1 O with its interior at +4, its
    one-pixel border exactly at 1.0 (the stability offset) and -4 outside (score O), 2 O at +0.5 (stability 0, score O),
    3 O eroded by one pixel (score O - 0.3).  A point outside every object: empty masks (stability 0 / 0), score 0.99.
    shift: added to every score (negative scores)."""

    def __init__(self, shift=0.0):
        self.off = (0, 0)
        self.shift = shift

    def set_crop(self, crop):
        self.off = (int(crop[0, 0, 0]), int(crop[0, 0, 1]))
        self.hw = crop.shape[:2]

    def __call__(self, points):
        h, w = self.hw
        ys, xs = np.mgrid[0:h, 0:w]
        xs, ys = xs + self.off[0], ys + self.off[1]
        B = len(points)
        lg = np.full((B, 4, h, w), -4.0, np.float32)
        iou = np.full((B, 4), 0.99, np.float32)
        lg[:, 0] = 4.0
        for b, (px, py) in enumerate(points):
            gx, gy = px + self.off[0], py + self.off[1]
            hit = [o for o in OBJECTS if _inside(o, np.array(gx), np.array(gy))]
            if not hit:
                continue
            o = hit[0]
            m = _inside(o, xs, ys)
            e = _erode(_inside(o, *np.mgrid[0:H, 0:W][::-1]))[ys, xs]
            lg[b, 1][m] = 1.0
            lg[b, 1][e] = 4.0
            lg[b, 2][m] = 0.5
            lg[b, 3][e] = 4.0
            iou[b, 1:] = [o["iou"], o["iou"], o["iou"] - 0.3]
        return torch.from_numpy(lg), torch.from_numpy(iou + np.float32(self.shift))


BASE = dict(points_per_side=4, pred_iou_thresh=0.7, stability_score_thresh=0.6, box_nms_thresh=0.7)
CROPS = dict(BASE, crop_n_layers=1)
NEG = dict(BASE, pred_iou_thresh=0.0)


def _run(kw, defect=None, shift=0.0, output_mode="binary_mask"):
    m = Authored(shift)
    return amgref.generate(_image(), m, set_crop=m.set_crop, defect=defect, output_mode=output_mode, **kw)


def test_helpers_agree_with_transformers():
    for n in (1, 4, 7, 32):
        assert np.array_equal(amg.build_point_grid(n), T._build_point_grid(n))
    for hw in ((1080, 1920), (1920, 1080), (333, 517), (64, 96)):
        for layers in (0, 1, 2):
            for ratio in (512 / 1500, 0.25):
                assert amg.generate_crop_boxes(hw, layers, ratio) == T._generate_per_layer_crops(layers, ratio, hw)
    rng = np.random.default_rng(0)
    masks = torch.from_numpy(rng.random((6, 13, 17)) < 0.5)
    masks[0] = False
    masks[1] = True
    masks[2, :, :] = False
    masks[2, 0, 0] = True
    for i, r in enumerate(T._mask_to_rle(masks)):
        assert amg.mask_to_rle(masks[i].numpy()) == r
        assert np.array_equal(amg.rle_to_mask(r), masks[i].numpy()) and np.array_equal(T._rle_to_mask(r), masks[i].numpy())
    # the transform: get_preprocess_shape, float64 numpy and f32 torch coordinates
    tr = ResizeLongestSide(1024)
    for h, w in ((1080, 1920), (1920, 1080), (333, 517)):
        s = 1024 * 1.0 / max(h, w)
        nh, nw = int(h * s + 0.5), int(w * s + 0.5)
        assert tr.get_preprocess_shape(h, w, 1024) == (nh, nw)
        c = rng.uniform(0, 2000, (5, 2))
        assert np.array_equal(tr.apply_coords(c, (h, w)), np.stack([c[:, 0] * (nw / w), c[:, 1] * (nh / h)], 1))
        ct = torch.from_numpy(c).float()
        assert torch.equal(tr.apply_coords_torch(ct, (h, w)), torch.stack([ct[:, 0] * (nw / w), ct[:, 1] * (nh / h)], 1))
        b = rng.uniform(0, 900, (3, 4))
        assert np.array_equal(tr.apply_boxes(b, (h, w)), tr.apply_coords(b.reshape(-1, 2, 2), (h, w)).reshape(-1, 4))
        assert tr.apply_image(np.zeros((h // 8, w // 8, 3), np.uint8)).shape[:2] == tr.get_preprocess_shape(h // 8, w // 8, 1024)


def test_authored_case_gives_hand_derived_records():
    recs = _run(BASE)
    ys, xs = np.mgrid[0:H, 0:W]
    grid = amg.build_point_grid(4) * [W, H]
    want = []
    for o in sorted(OBJECTS, key=lambda o: -o["iou"]):      # NMS order: descending score
        m = _inside(o, xs, ys)
        e = _erode(m)
        first = next(p for p in grid if _inside(o, np.array(p[0]), np.array(p[1])))  # ties go to the earlier point
        yy, xx = np.nonzero(m)
        want.append(dict(area=int(m.sum()), bbox=[int(xx.min()), int(yy.min()), int(xx.max() - xx.min()), int(yy.max() - yy.min())],
                         predicted_iou=float(np.float32(o["iou"])), point_coords=[first.tolist()],
                         stability_score=float(np.float32(e.sum()) / np.float32(m.sum())), crop_box=[0, 0, W, H], segmentation=m))
    ok, msg = amgref.records_equal(recs, want)
    assert ok, msg


DEFECTS = [("stability_ge", BASE, 0.0), ("exclusive_box_max", BASE, 0.0), ("masks_0_2", BASE, 0.0), ("no_edge_filter", CROPS, 0.0),
           ("no_cross_crop_nms", CROPS, 0.0), ("unstable_ties", BASE, 0.0), ("unsigned_score_bits", NEG, -1.5)]


@pytest.mark.parametrize("defect,kw,shift", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_each_defect_changes_the_records(defect, kw, shift):
    good = _run(kw, shift=shift)
    bad = _run(kw, defect=defect, shift=shift)
    assert len(good) > 0
    ok, msg = amgref.records_equal(good, bad)
    assert not ok, f"defect {defect} left the records unchanged"


def test_crop_layer_and_negative_scores_run_through():
    recs = _run(CROPS)
    assert len(recs) >= len(OBJECTS) and {tuple(r["crop_box"]) for r in recs} != {(0, 0, W, H)}
    neg = _run(NEG, shift=-1.5)
    assert len(neg) == len(OBJECTS) and all(r["predicted_iou"] < 0 for r in neg)
    rle = _run(BASE, output_mode="uncompressed_rle")
    for r, s in zip(_run(BASE), rle):
        assert np.array_equal(amg.rle_to_mask(s["segmentation"]), r["segmentation"])
