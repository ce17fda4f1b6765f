"""SamAutomaticMaskGenerator and SamPredictor.predict_torch on the MI355X: lmx_k_mask_score against counts and boxes taken from
lmx_k_mask_logits' output, lmx_k_nms_boxes against oracle.nms.torchvision_nms, the shared-embedding decode, predict_torch and
the transform, and generate() record for record against the host restatement tests/amgref.py fed by the device decoder."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amgref
import samprompt as SP
from oracle.nms import torchvision_nms

pytestmark = pytest.mark.gpu

# (frame h, w): landscape / portrait 1080p and 1030x1031 (the staged kernel, the last with w % 4 != 0 and a partial tile),
# odd, crop-sized with w % 4 != 0, small (the direct kernel: frame smaller than the input frame)
GEOMS = [(1080, 1920), (1920, 1080), (1030, 1031), (333, 517), (541, 962), (97, 130)]


def _resized(h, w):
    from lmx import sam

    return sam.resize_longest_side(h, w, 1024)


def _score_fixture(n, thr, off, seed):
    """Low-res logits [n,256,256]: piecewise-constant 32x32 blocks valued thr - off, thr, thr + off or random, plus an empty
    mask, a full mask and a frame touching every border."""
    rng = np.random.default_rng(seed)
    vals = np.array([thr - off, thr, thr + off], np.float32)
    pick = rng.integers(0, 4, (n, 8, 8))
    blocks = np.where(pick < 3, vals[np.minimum(pick, 2)], rng.standard_normal((n, 8, 8)).astype(np.float32) * 3)
    lg = np.repeat(np.repeat(blocks, 32, 1), 32, 2).astype(np.float32)
    lg[0] = -10.0
    lg[1] = 10.0
    lg[2] = -10.0
    lg[2, :3, :] = lg[2, -3:, :] = lg[2, :, :3] = lg[2, :, -3:] = 5.0
    return torch.from_numpy(lg)


def _ref_score(v, thr, off):
    t_hi, t_lo, t = (torch.tensor(x, dtype=torch.float32).item() for x in (thr + off, thr - off, thr))
    c_hi = (v > t_hi).sum((1, 2))
    c_lo = (v > t_lo).sum((1, 2))
    m = v > t
    boxes = torch.zeros((v.shape[0], 4), dtype=torch.int64, device=v.device)
    for i in range(v.shape[0]):
        if m[i].any():
            ys, xs = torch.nonzero(m[i], as_tuple=True)
            boxes[i] = torch.stack([xs.min(), ys.min(), xs.max(), ys.max()])
    out = torch.zeros((v.shape[0], 8), dtype=torch.int64, device=v.device)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3:7] = c_hi, c_lo, m.sum((1, 2)), boxes
    return out, (v == t_hi).sum(), (v == t_lo).sum(), (v == t).sum()


@pytest.mark.parametrize("thr,off", [(0.0, 1.0), (0.25, 0.5)])
@pytest.mark.parametrize("geom", GEOMS, ids=[f"{h}x{w}" for h, w in GEOMS])
def test_mask_score_equals_mask_logits_counts(cuda, geom, thr, off):
    from lmx import kernels as K

    h, w = geom
    nh, nw = _resized(h, w)
    lg = _score_fixture(12, thr, off, seed=h * 7 + w).to(cuda)
    got = K.mask_score(lg, 1024, nh, nw, h, w, thr, off)
    v = K.mask_logits(lg, 1024, nh, nw, h, w)
    ref, e_hi, e_lo, e_t = _ref_score(v, thr, off)
    # the fixture puts >= 1000 output pixels exactly on each threshold (where > and >= part)
    assert min(int(e_hi), int(e_lo), int(e_t)) >= 1000, (int(e_hi), int(e_lo), int(e_t))
    assert torch.equal(got, ref), (got - ref).abs().max()
    assert int(got[0, 2]) == 0 and got[0, 3:7].tolist() == [0, 0, 0, 0]
    assert int(got[1, 2]) == h * w and got[1, 3:7].tolist() == [0, 0, w - 1, h - 1]
    assert got[2, 3:7].tolist() == [0, 0, w - 1, h - 1]
    if thr == 0.0:
        _, stats = K.mask_post(lg, 1024, nh, nw, h, w)
        ne = got[:, 2] > 0
        assert torch.equal(got[:, 2], stats[:, 0]) and torch.equal(got[ne, 3:7], stats[ne, 3:7])


def test_mask_score_index_list_beyond_one_launch(cuda):
    """65 541 rows through an index list (two launches of <= 65 535) on a small frame: every row equals its mask's own score."""
    from lmx import kernels as K

    h, w = 41, 66
    nh, nw = _resized(h, w)
    lg = _score_fixture(8, 0.0, 1.0, seed=5).to(cuda)
    own = K.mask_score(lg, 1024, nh, nw, h, w)
    idx = torch.arange(65541, dtype=torch.int32, device=cuda) % 8
    idx = idx[torch.randperm(65541, generator=torch.Generator().manual_seed(3)).to(cuda)].contiguous()
    got = K.mask_score(lg, 1024, nh, nw, h, w, idx=idx)
    assert torch.equal(got, own[idx.long()])


def _nms_case(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 500, (n, 2)).astype(np.float32)
    wh = rng.uniform(0, 120, (n, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    if n >= 8:
        boxes[n // 4: n // 4 + n // 8] = boxes[: n // 8]                 # duplicates
        boxes[-(n // 16) - 1:, 2] = boxes[-(n // 16) - 1:, 0]           # zero area
    scores = np.round(rng.standard_normal(n).astype(np.float32) * 4) / 4  # many ties, half negative
    scores[: n // 10] = -0.0
    return boxes, scores.astype(np.float32)


@pytest.mark.parametrize("thr", [0.7, 0.5])
@pytest.mark.parametrize("n", [1, 64, 3072, 16384])
def test_nms_boxes_equals_torchvision_nms(cuda, n, thr):
    from lmx import kernels as K

    boxes, scores = _nms_case(n, seed=n)
    keep, count = K.nms_boxes(torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), thr)
    k = int(count.cpu()[0])
    ref = torchvision_nms(boxes, scores, thr)
    assert k == len(ref) and np.array_equal(keep.cpu().numpy()[:k], ref)
    assert (keep.cpu().numpy()[k:] == -1).all()
    if n >= 64:  # a validity mask: the same as NMS over the valid subset
        valid = np.random.default_rng(n + 1).random(n) < 0.6
        keep, count = K.nms_boxes(torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), thr,
                                  valid=torch.from_numpy(valid).to(cuda))
        sub = np.flatnonzero(valid)
        ref = sub[torchvision_nms(boxes[sub], scores[sub], thr)]
        k = int(count.cpu()[0])
        assert k == len(ref) and np.array_equal(keep.cpu().numpy()[:k], ref)


def _clustered_case(n, bases, seed):
    """n boxes in `bases` clusters of near-duplicates (IoU > 0.7 inside a cluster), scores from a few values (ties), as the
    cross-crop NMS sees them: the same mask found in several crops, scored 1 / crop area."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 4000, (bases, 2)).astype(np.float32)
    wh = rng.uniform(20, 200, (bases, 2)).astype(np.float32)
    b = rng.integers(0, bases, n)
    jit = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    boxes = (np.concatenate([xy[b], xy[b] + wh[b]], 1) + jit).astype(np.float32)
    scores = np.float32(1) / rng.choice(np.array([1080 * 1920, 700 * 1200, 540 * 960], np.float32), n)
    return boxes, scores.astype(np.float32)


@pytest.mark.parametrize("cap", [None, 1000], ids=["cap16384", "cap1000"])
def test_nms_any_beyond_one_launch_equals_torchvision_nms(cuda, cap, monkeypatch):
    """More candidates than one lmx_k_nms_boxes launch holds (the cross-crop NMS of many crops): the chunked greedy NMS of
    lmx.amg.nms_any equals the one-pass oracle.  cap1000 lowers the launch size so that many chunks carry kept boxes."""
    from lmx import amg
    from lmx import kernels as K

    if cap:
        monkeypatch.setattr(K, "NMS_BOXES_MAX", cap)
    n, bases = (40000, 3000) if cap is None else (3500, 400)
    boxes, scores = _clustered_case(n, bases, seed=7)
    keep = amg.nms_any(torch.from_numpy(boxes).to(cuda), scores, 0.7)
    ref = torchvision_nms(boxes, scores, 0.7)
    assert len(ref) > (0 if cap is None else cap // 4) and np.array_equal(keep, ref)
    # a kept set larger than one launch cannot be carried: a clear error, not a wrong answer
    monkeypatch.setattr(K, "NMS_BOXES_MAX", 100)
    with pytest.raises(ValueError, match="keeps more than 100"):
        amg.nms_any(torch.from_numpy(boxes[:1000]).to(cuda), scores[:1000], 0.7)


# ---------------------------------------------------------------------------------------------------- decoder / predictor
def _dec_state(seed=62, iou_shift=0.0):
    """Synthetic decoder weights; iou_shift moves the IoU head's output (its last bias) so that a positive pred_iou_thresh can
    bite (segment_anything applies the IoU filter only for thresholds > 0)."""
    from lmx import sam_decoder, weights

    sd = sam_decoder.synthetic_state_dict(seed)
    sd.update(weights.synth_state_dict(sam_decoder.mask_embed_param_spec(), seed + 1))
    b = "mask_decoder.iou_prediction_head.proj_out.bias"
    sd[b] = (sd[b] + np.float32(iou_shift)).astype(np.float32)
    return sd


@pytest.mark.parametrize("precision", ["exact", "f16"])
def test_shared_embedding_prompt_alone_equals_prompt_in_batch(cuda, precision):
    from lmx import sam_decoder

    dec = sam_decoder.MaskDecoder(_dec_state(), cuda)
    rng = np.random.default_rng(4)
    base = torch.from_numpy(rng.standard_normal((1, 256, 8, 8)).astype(np.float32))
    emb = F.interpolate(base, size=(64, 64), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).reshape(-1, 256).contiguous()
    emb = emb.to(cuda) if precision == "exact" else emb.to(cuda).half()
    n = 9
    pts = torch.from_numpy(rng.uniform(0, 1000, (n, 2, 2)).astype(np.float32)).to(cuda)
    lab = torch.from_numpy(rng.integers(0, 2, (n, 2)).astype(np.int32)).to(cuda)
    for input_frame in (False, True):
        lr, iou = dec.decode_lowres(emb, (1080, 1920), (576, 1024), points=pts, labels=lab, multimask=True, precision=precision,
                                    input_frame=input_frame)
        for i in (0, 4, 8):
            lr1, iou1 = dec.decode_lowres(emb, (1080, 1920), (576, 1024), points=pts[i:i + 1], labels=lab[i:i + 1], multimask=True,
                                          precision=precision, input_frame=input_frame)
            assert torch.equal(lr[i:i + 1], lr1) and torch.equal(iou[i:i + 1], iou1), (i, input_frame)
    # frame pixels and the same points pre-scaled to the input frame in float64 give the same tokens
    a = dec.decode(emb, (1080, 1920), (576, 1024), points=pts[:2], labels=lab[:2], multimask=False, precision=precision)
    sc = torch.tensor([1024 / 1920, 576 / 1080], dtype=torch.float64, device=cuda)
    b = dec.decode(emb, (1080, 1920), (576, 1024), points=(pts[:2].double() * sc).float(), labels=lab[:2], multimask=False,
                   precision=precision, input_frame=True)
    assert torch.equal(a["lowres"], b["lowres"]) and torch.equal(a["mask"], b["mask"])


def _vit_sam(cuda):
    from lmx import adapters, sam, weights

    cfg = sam.SamVitConfig(hidden=128, layers=3, heads=2, mlp=256, global_idx=(1,), window=14, image=1024)
    sd = weights.synth_state_dict(sam.vit_param_spec(cfg), 61)
    sd.update(_dec_state(62, iou_shift=1.0))
    return adapters.LmxSam(cfg, sd, cuda), sd


def _hiera_predictor(cuda):
    from lmx import adapters, sam, sam_decoder, weights

    cfg = sam.HieraConfig(hidden=16, blocks=(1, 1, 1, 1), dims=(16, 32, 64, 128), heads=(1, 2, 4, 8), global_blocks=(),
                          pos_bkg=(7, 7), fpn_dim=256, image=1024)
    enc = sam.HieraEncoder(cfg, weights.synth_state_dict(sam.param_spec(cfg), 11), cuda)
    return adapters.LmxSamPredictor.from_parts(enc, sam_decoder.MaskDecoder(_dec_state(63), cuda))


@pytest.fixture(scope="module")
def vit(cuda):
    return _vit_sam(cuda)


def test_predict_torch_matches_float64(vit, cuda):
    from lmx import adapters, synth

    model, sd = vit
    pred = adapters.SamPredictor(model)
    frame = synth.synth_frame(6, 20)
    pred.set_image(frame)
    H, W = pred.original_size
    pts = np.array([[[600.0, 500.0]], [[1300.0, 300.0]], [[200.0, 900.0]]])
    tp = pred.transform.apply_coords_torch(torch.from_numpy(pts), (H, W)).to(cuda)
    lab = torch.ones((3, 1), dtype=torch.int32, device=cuda)
    masks, iou, low = pred.predict_torch(tp, lab, multimask_output=True)
    assert masks.shape == (3, 3, H, W) and masks.dtype == torch.bool and iou.shape == (3, 3) and low.shape == (3, 3, 256, 256)
    logits, iou2, low2 = pred.predict_torch(tp, lab, multimask_output=True, return_logits=True)
    assert torch.equal(logits > 0, masks) and torch.equal(iou2, iou) and torch.equal(low2, low)
    emb = pred.get_image_embedding().cpu().double()
    for b in range(3):
        with torch.no_grad():
            lr, ir, _, _ = SP.predict(SP.sd_as(sd, torch.float64), emb, (H, W), pred.input_size, points=pts[b].astype(np.float32)[None],
                                      labels=np.ones((1, 1), np.int32), multimask=True)
        for c in range(3):
            rel = float((low[b, c].cpu().double() - lr[0, c]).norm() / lr[0, c].norm())
            assert rel <= 1e-4, (b, c, rel)
        assert float((iou[b].cpu().double() - ir[0]).abs().max()) <= 2e-4
    # box prompts in the input frame
    bx = pred.transform.apply_boxes_torch(torch.tensor([[420.0, 360.0, 1010.0, 850.0]]), (H, W)).to(cuda)
    m_b, i_b, _ = pred.predict_torch(None, None, boxes=bx, multimask_output=False)
    assert m_b.shape == (1, 1, H, W)


def test_transform_follows_segment_anything_arithmetic(vit):
    from lmx import adapters

    tr = adapters.SamPredictor(vit[0]).transform
    for (h, w) in [(1080, 1920), (1920, 1080), (333, 517)]:
        nh, nw = tr.get_preprocess_shape(h, w, 1024)
        s = 1024 * 1.0 / max(h, w)
        assert (nh, nw) == (int(h * s + 0.5), int(w * s + 0.5))
        c = np.random.default_rng(h).uniform(0, 2000, (5, 2))
        assert np.array_equal(tr.apply_coords(c, (h, w)), np.stack([c[:, 0] * (nw / w), c[:, 1] * (nh / h)], 1))
        ct = torch.from_numpy(c).float()
        ref = torch.stack([ct[:, 0] * (nw / w), ct[:, 1] * (nh / h)], 1)
        assert torch.equal(tr.apply_coords_torch(ct, (h, w)), ref)
        assert np.array_equal(tr.apply_boxes(c[:4].reshape(1, 8)[:, :4], (h, w)).ravel(), tr.apply_coords(c[:2], (h, w)).ravel())


# ---------------------------------------------------------------------------------------------------------------- generate()
def _image(h, w, seed):
    """Smooth colour blobs: an image the synthetic encoders turn into varied masks."""
    rng = np.random.default_rng(seed)
    base = torch.from_numpy(rng.uniform(0, 255, (1, 3, 6, 6)).astype(np.float32))
    img = F.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.ascontiguousarray(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))


def _device_decode_fn(pred, precision=None):
    """amgref's model: the device decoder on the predictor's current crop, full-size logits from lmx_k_mask_logits."""
    from lmx import kernels as K

    def decode(points):
        H, W = pred.original_size
        tp = torch.from_numpy(pred.transform.apply_coords(points, (H, W)).astype(np.float32)).to(pred.device)[:, None].contiguous()
        lab = torch.ones((len(points), 1), dtype=torch.int32, device=pred.device)
        lr, iou = pred.decoder.decode_lowres(pred.features, (H, W), pred.input_size, points=tp, labels=lab, multimask=True,
                                             precision=precision, input_frame=True)
        nh, nw = pred.input_size
        v = K.mask_logits(lr.reshape(-1, 256, 256).contiguous(), pred.decoder.S, nh, nw, H, W).view(len(points), 3, H, W)
        return v.cpu(), iou.cpu()

    return decode


def _thresholds(pred, image, pps):
    """(pred_iou_thresh, stability_score_thresh) at the medians of the whole-image candidates (so each filter bites), and
    the lowest IoU score among them."""
    pred.set_image(image)
    H, W = image.shape[:2]
    logits, iou = _device_decode_fn(pred)(amgref.point_grids(pps, 0, 1)[0] * np.array([[W, H]]))
    m = logits.flatten(0, 1)
    stab = ((m > 1.0).sum((1, 2)).double() / (m > -1.0).sum((1, 2)).double()).float()
    stab = stab[~torch.isnan(stab)]
    return float(iou.flatten().median()), float(stab.median()), float(iou.min())


CASES = [
    # id, frame (h, w), kwargs
    ("landscape-8", (90, 160), dict(points_per_side=8)),
    ("portrait-12", (150, 100), dict(points_per_side=12, points_per_batch=20)),
    ("crops-ds2", (120, 176), dict(points_per_side=8, crop_n_layers=1, crop_n_points_downscale_factor=2)),
    ("grids", (100, 130), dict(points_per_side=None, point_grids=[np.random.default_rng(1).uniform(0.05, 0.95, (40, 2))])),
    ("iou-off", (96, 128), dict(points_per_side=10, pred_iou_thresh=0.0)),
]


def _run_both(pred, model, image, kw, precision=None):
    from lmx import adapters

    kw = dict(kw)
    pps = kw.get("points_per_side") or 8
    it, st, min_iou = _thresholds(pred, image, pps)
    kw.setdefault("pred_iou_thresh", it)
    kw.setdefault("stability_score_thresh", st)
    if precision:
        pred.decoder.precision = precision
    gen = adapters.SamAutomaticMaskGenerator(model, **kw)
    recs = gen.generate(image)
    trace = {}
    rkw = {k: v for k, v in kw.items() if k != "point_grids"}
    if "point_grids" in kw:
        rkw["point_grids_"] = kw["point_grids"]
        rkw["points_per_side"] = None
    ref = amgref.generate(image, _device_decode_fn(pred), set_crop=pred.set_image, trace=trace, **rkw)
    return recs, ref, trace, min_iou


@pytest.mark.parametrize("precision", ["exact", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_generate_equals_reference(vit, cuda, case, precision):
    from lmx import adapters

    model, _ = vit
    pred = adapters.SamPredictor(model)
    name, (h, w), kw = case
    try:
        recs, ref, tr, _ = _run_both(pred, pred, _image(h, w, seed=h + w), kw, precision)
    finally:
        pred.decoder.precision = "exact"
    ok, msg = amgref.records_equal(recs, ref)
    assert ok, msg
    if kw.get("pred_iou_thresh", 1) > 0:  # the cases with both filters on: each filter rejects and keeps candidates
        assert tr["cand"] > tr["after_iou"] > tr["after_stab"] > 0, tr
    assert tr["after_stab"] > 0 and tr["after_edge"] > tr["after_nms"] > 0, tr
    print(f"generate [{name}] {precision}: {len(recs)} records, trace {tr}")


class _DiscPredictor:
    """A stand-in for LmxSamPredictor's model half with authored low-res logits (the generator's kernels, filters and NMS are
    the real ones): a point inside one of DISCS gets that disc as masks 1..3 (+4 inside, -4 outside on the 256x256 grid, scores
    s, s - 0.1, s - 0.2); any other point gets empty masks.  The image's pixels carry their coordinates, so a crop knows its
    offset."""
    DISCS = [(150.0, 100.0, 12.0, 0.9), (180.0, 40.0, 12.0, 0.8), (60.0, 150.0, 14.0, 0.85), (250.0, 160.0, 10.0, 0.7)]

    def __init__(self, cuda):
        self.S = 1024
        self.device = cuda

    def decode_lowres(self, feats, hw, resized, points=None, labels=None, multimask=True, precision=None, input_frame=True, **_):
        ch, cw = hw
        nh, nw = resized
        ox, oy = self.off
        p = points[:, 0].double()
        px, py = p[:, 0] / (nw / cw) + ox, p[:, 1] / (nh / ch) + oy
        u = torch.arange(256, device=self.device, dtype=torch.float64) * 4 + 2
        gx, gy = u / (nw / cw) + ox, u / (nh / ch) + oy
        B = p.shape[0]
        lr = torch.full((B, 3, 256, 256), -4.0, device=self.device)
        iou = torch.full((B, 3), 0.5, device=self.device)
        done = torch.zeros(B, dtype=torch.bool, device=self.device)
        for cx, cy, r, sc in self.DISCS:
            pin = ((px - cx) ** 2 + (py - cy) ** 2 <= r * r) & ~done
            grid = ((gx[None, :] - cx) ** 2 + (gy[:, None] - cy) ** 2 <= r * r).float() * 8 - 4
            lr[pin] = grid[None, None].expand(int(pin.sum()), 3, 256, 256)
            iou[pin] = torch.tensor([sc, sc - 0.1, sc - 0.2], device=self.device)
            done |= pin
        return lr.contiguous(), iou


def test_generate_crops_edge_filter_and_cross_crop_nms(cuda):
    """crop_n_layers=1 on authored discs, some inside every crop, one across a crop's inner edge: lmx.amg equals amgref, and
    the edge filter and the cross-crop NMS each remove candidates."""
    from lmx import adapters

    H, W = 200, 300
    ys, xs = np.mgrid[0:H, 0:W]
    image = np.stack([xs % 256, ys, xs // 256], -1).astype(np.uint8)
    pred = adapters.LmxSamPredictor.__new__(adapters.LmxSamPredictor)
    pred.decoder = _DiscPredictor(cuda)
    pred.device = cuda
    pred.transform = adapters.ResizeLongestSide(1024)
    pred.model = type("M", (), {"mask_threshold": 0.0})()

    def set_image(crop):
        pred.decoder.off = (int(crop[0, 0, 0]) + 256 * int(crop[0, 0, 2]), int(crop[0, 0, 1]))
        pred.original_size = crop.shape[:2]
        pred.input_size = pred.transform.get_preprocess_shape(crop.shape[0], crop.shape[1], 1024)
        pred.features = None

    pred.set_image = set_image
    pred.reset_image = lambda: None
    kw = dict(points_per_side=8, crop_n_layers=1, pred_iou_thresh=0.0, stability_score_thresh=0.5)
    recs = adapters.SamAutomaticMaskGenerator(pred, **kw).generate(image)
    trace = {}
    ref = amgref.generate(image, _device_decode_fn(pred), set_crop=pred.set_image, trace=trace, **kw)
    ok, msg = amgref.records_equal(recs, ref)
    assert ok, msg
    assert trace["after_stab"] > trace["after_edge"] and trace["before_cross"] > trace["after_cross"] > 0, trace
    assert len({tuple(r["crop_box"]) for r in recs}) > 1, [r["crop_box"] for r in recs]


def test_generate_hiera_equals_reference(cuda):
    """Hiera encoder through from_parts, the IoU filter off (pred_iou_thresh=0): the unshifted IoU head's negative scores
    reach NMS."""
    pred = _hiera_predictor(cuda)
    recs, ref, tr, min_iou = _run_both(pred, pred, _image(110, 150, seed=9), dict(points_per_side=8, pred_iou_thresh=0.0))
    ok, msg = amgref.records_equal(recs, ref)
    assert ok, msg
    assert min_iou < 0 and tr["after_stab"] > 0 and tr["after_nms"] > 0, (min_iou, tr)
    print(f"generate [hiera] {len(recs)} records, min IoU score {min_iou:.4f}, trace {tr}")


def test_generate_is_batch_invariant(vit, cuda):
    from lmx import adapters

    model, _ = vit
    pred = adapters.SamPredictor(model)
    image = _image(100, 140, seed=2)
    it, st, _ = _thresholds(pred, image, 9)
    runs = [adapters.SamAutomaticMaskGenerator(pred, points_per_side=9, points_per_batch=b, pred_iou_thresh=it, stability_score_thresh=st)
            .generate(image) for b in (1, 7, 64, 81)]
    assert len(runs[0]) > 0
    for r in runs[1:]:
        ok, msg = amgref.records_equal(runs[0], r)
        assert ok, msg


def test_generate_1080p_writes_no_full_size_logits(vit, cuda, monkeypatch):
    """Default parameters at 1080p (and the same grid with both score filters off, so that records exist) with
    lmx.kernels.mask_logits disabled: each record equals predict_torch on its own point."""
    from lmx import adapters
    from lmx import kernels as K

    model, _ = vit
    pred = adapters.SamPredictor(model)
    image = _image(1080, 1920, seed=7)

    def forbidden(*a, **k):
        raise AssertionError("generate() materialised full-size logits")

    with monkeypatch.context() as m:
        m.setattr(K, "mask_logits", forbidden)
        adapters.SamAutomaticMaskGenerator(model).generate(image)
        recs = adapters.SamAutomaticMaskGenerator(pred, pred_iou_thresh=0.0, stability_score_thresh=0.0).generate(image)
    assert len(recs) > 0
    pred.set_image(image)
    for r in recs[:12]:
        p = np.asarray(r["point_coords"], np.float64)
        tp = torch.from_numpy(pred.transform.apply_coords(p, (1080, 1920)).astype(np.float32)).to(cuda)[:, None]
        logits, iou, _ = pred.predict_torch(tp, torch.ones((1, 1), dtype=torch.int32, device=cuda), return_logits=True)
        c = [j for j in range(3) if np.float32(iou[0, j].item()).view(np.uint32) == np.float32(r["predicted_iou"]).view(np.uint32)]
        assert len(c) >= 1
        v = logits[0, c[0]]
        mask = (v > 0).cpu().numpy()
        assert np.array_equal(mask, r["segmentation"])
        stab = np.float32(float((v > 1.0).sum()) / float((v > -1.0).sum())) if int((v > -1.0).sum()) else np.float32(np.nan)
        assert np.float32(r["stability_score"]).view(np.uint32) == stab.view(np.uint32) or (np.isnan(stab) and np.isnan(r["stability_score"]))
        assert r["area"] == int(mask.sum())
        if r["area"]:
            ys, xs = np.nonzero(mask)
            assert r["bbox"] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def test_output_modes_and_argument_errors(vit, cuda):
    from lmx import adapters, amg

    model, _ = vit
    image = _image(80, 120, seed=4)
    kw = dict(points_per_side=6, pred_iou_thresh=0.0, stability_score_thresh=0.0)
    a = adapters.SamAutomaticMaskGenerator(model, **kw).generate(image)
    b = adapters.SamAutomaticMaskGenerator(model, output_mode="uncompressed_rle", **kw).generate(image)
    assert len(a) == len(b) > 0
    for r, s in zip(a, b):
        assert np.array_equal(amg.rle_to_mask(s["segmentation"]), r["segmentation"])
        assert s["segmentation"]["size"] == [80, 120] and sum(s["segmentation"]["counts"]) == 80 * 120
    G = adapters.SamAutomaticMaskGenerator
    with pytest.raises(ValueError):
        G(model, points_per_side=None)
    with pytest.raises(ValueError):
        G(model, points_per_side=8, point_grids=[np.zeros((4, 2))])
    with pytest.raises(ValueError):
        G(model, points_per_side=None, point_grids=[np.zeros((4, 2))], crop_n_layers=1)
    with pytest.raises(ValueError, match="pycocotools"):
        G(model, output_mode="coco_rle")
    with pytest.raises(ValueError, match="cv2"):
        G(model, min_mask_region_area=10)
    with pytest.raises(ValueError):
        G(model, output_mode="polygons")
