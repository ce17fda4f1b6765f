"""The SAM prompt paths beyond the box on the MI355X (csrc/prompt.hip, MaskDecoder.decode, LmxSamPredictor.predict): each new
kernel against float64 (tests/samprompt.py) or bit for bit against the kernel it generalises, every decoder case of
tests/test_sam_prompt_ref_host.py on both plans against the float64 reference, decode == predict, batch invariance, and the
segment_anything idioms through the adapter.  A landscape 1080x1920 and a portrait 1920x1080 frame throughout."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import samprompt as SP

pytestmark = pytest.mark.gpu

FRAMES = [((1080, 1920), (576, 1024)), ((1920, 1080), (1024, 576))]


def _state(seed=41):
    from lmx import sam_decoder, weights

    sd = sam_decoder.synthetic_state_dict(seed)
    sd.update(weights.synth_state_dict(sam_decoder.mask_embed_param_spec(), seed + 1))
    return sd


def _emb(seed, n=1):
    rng = np.random.default_rng(seed)
    base = torch.from_numpy(rng.standard_normal((n, 256, 8, 8)).astype(np.float32))
    emb = F.interpolate(base, size=(64, 64), mode="bilinear", align_corners=False) * 2.0
    return (emb + 0.1 * torch.from_numpy(rng.standard_normal(emb.shape).astype(np.float32))).half().float()  # exact in f16 too


def _rows(emb):
    return emb.permute(0, 2, 3, 1).reshape(-1, 256).contiguous()


def _mask_input(seed, n=1):
    rng = np.random.default_rng(seed)
    m = F.interpolate(torch.from_numpy(rng.standard_normal((n, 1, 16, 16)).astype(np.float32)) * 8, size=(256, 256), mode="bilinear",
                      align_corners=False)
    return m[:, 0].contiguous()


def _lg(r):
    return f"2^{np.log2(max(r, 1e-300)):.2f}"


# ---------------------------------------------------------------------------------------------------------- prompt_points
@pytest.mark.parametrize("frame", FRAMES, ids=["landscape", "portrait"])
def test_prompt_points_matches_float64(cuda, frame):
    from lmx import kernels as K
    from lmx import sam_decoder

    (h, w), (nh, nw) = frame
    sd = _state()
    dec = sam_decoder.MaskDecoder(sd, cuda)
    sd64 = SP.sd_as(sd, torch.float64)
    pts = np.array([[[0.0, 0.0], [w - 1.0, h - 1.0], [w / 3 + 0.25, h / 2 - 0.75], [-30.0, h + 50.0], [17.0, 5.0]],
                    [[w - 1.0, 0.0], [0.0, h - 1.0], [w / 2, h / 2], [w + 10.0, -8.0], [500.5, 300.25]]], np.float32)
    lab = np.array([[1, 0, -1, 1, 0], [-1, -1, 1, 0, 1]], np.int32)
    box = np.array([[10.0, 20.0, w - 1.0, h - 1.0], [w / 4, h / 4, w / 2, h / 2]], np.float32)
    d = dict(points=torch.from_numpy(pts).to(cuda), labels=torch.from_numpy(lab).to(cuda), boxes=torch.from_numpy(box).to(cuda))
    args = (nw / w, nh / h, 1024.0, dec.gauss, dec.point_embed, dec.not_a_point, dec.corner)
    worst = 0.0
    for with_box in (False, True):
        got = K.prompt_points(d["points"], d["labels"], d["boxes"] if with_box else None, *args).cpu()
        ref = SP.encode_prompts(sd64, SP.scale_coords(pts, (h, w), (nh, nw)), lab,
                                SP.scale_coords(box.reshape(-1, 2, 2), (h, w), (nh, nw)).reshape(-1, 4) if with_box else None)
        assert got.shape == ref.shape == (2, 5 + (2 if with_box else 1), 256)
        err = float((got.double() - ref).abs().max())
        worst = max(worst, err / 2e-4)
        assert err <= 2e-4, err
        nap = torch.from_numpy(sd["prompt_encoder.not_a_point_embed.weight"][0])
        for b in range(2):
            for t in range(5):
                if lab[b, t] == -1:
                    assert torch.equal(got[b, t], nap)
            if not with_box:
                assert torch.equal(got[b, 5], nap)  # the pad token
    # box only: the bits of lmx_k_prompt_box
    a = K.prompt_points(None, None, d["boxes"], *args)
    b = K.prompt_box(d["boxes"], nw / w, nh / h, 1024.0, dec.gauss, dec.corner)
    assert torch.equal(a, b)
    # a label outside {-1, 0, 1} poisons its token only
    bad = d["labels"].clone()
    bad[0, 2] = 2
    p = K.prompt_points(d["points"], bad, None, *args).cpu()
    assert torch.isnan(p[0, 2]).all() and not torch.isnan(p[0, :2]).any() and not torch.isnan(p[1]).any()
    print(f"prompt_points {h}x{w}: worst ratio to the 2e-4 bound {_lg(worst)}")


# ---------------------------------------------------------------------------------------------------------- mask_embed
MASKS = ["random", "pm20", "constant", "constant, equal conv1 channels (variance 0 -> eps)"]


def _mask_case(kind):
    if kind == "random":
        return _mask_input(3, 2)
    if kind == "pm20":
        return torch.where(_mask_input(4, 2) > 0, 20.0, -20.0)
    return torch.full((2, 256, 256), 0.75)


@pytest.mark.parametrize("emb_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", MASKS)
def test_mask_embed_matches_float64(cuda, kind, emb_dtype):
    """lmx_k_mask_embed within SP.mask_embed_bound (C = 4, u = 2^-24) of float64, per element; the same launch's output misses
    the bound of a reference without either LayerNorm by >= 30x.  With equal conv1 channels the first LayerNorm sees variance
    0 and outputs its bias alone; the bound carries 1/sqrt(eps) = 1000 times the conv1 magnitude forward there, so that input
    checks the kernel against the bound only (2^-17 measured) and the 30x is asked of the other three."""
    from lmx import kernels as K
    from lmx import sam_decoder

    sd = _state()
    if kind.startswith("constant, equal"):
        w = sd["prompt_encoder.mask_embed.conv1.weight"]
        sd["prompt_encoder.mask_embed.conv1.weight"] = np.repeat(w[:1], 4, 0)
        sd["prompt_encoder.mask_embed.conv1.bias"] = np.full(4, 0.3, np.float32)
    dec = sam_decoder.MaskDecoder(sd, cuda)
    mk = _mask_case(kind)
    emb = _rows(_emb(6, 2)).to(emb_dtype)
    got = K.mask_embed(mk.to(cuda), emb.to(cuda), dec.mask_params).cpu().double()
    sd64 = SP.sd_as(sd, torch.float64)
    ref, bound = SP.mask_embed_bound(sd64, mk.double(), emb.double())
    r = float(((got - ref).abs() / bound).max())
    print(f"mask_embed [{kind}] emb {emb_dtype}: max ratio {_lg(r)}")
    assert r <= 1.0
    for defect in () if kind.startswith("constant, equal") else ("no_ln1", "no_ln2"):
        bad = emb.double() + SP.mask_embed(sd64, mk.double(), defect=defect).permute(0, 2, 3, 1).reshape(-1, 256)
        rb = float(((got - bad).abs() / bound).max())
        print(f"  without {defect}: min miss {_lg(rb)}")
        assert rb >= 30, (defect, rb)


# ---------------------------------------------------------------------------------------------------------- hyper_mask_multi
@pytest.mark.parametrize("M", [1, 3, 4])
def test_hyper_mask_multi_slices_equal_single_kernels(cuda, M):
    from lmx import kernels as K

    n, G, C = 2, 64, 32
    g = torch.Generator().manual_seed(M)
    up16 = (torch.randn(n * G * G * 16, C, generator=g) * 0.7).half().to(cuda)
    up32 = (torch.randn(n * G * G * 16, C, generator=g) * 0.7).to(cuda)
    hyper = torch.randn(n, M, C, generator=g).to(cuda)
    multi = K.hyper_mask_multi(up16, hyper, n, G, C)
    for act in (K.ACT_NONE, K.ACT_GELU):
        multi32 = K.hyper_mask_multi_f32(up32, hyper, n, G, C, act=act)
        for m in range(M):
            h = hyper[:, m].contiguous()
            assert torch.equal(multi32[:, m], K.hyper_mask_f32(up32, h, n, G, C, act=act)), (m, act)
    for m in range(M):
        assert torch.equal(multi[:, m], K.hyper_mask(up16, hyper[:, m].contiguous(), n, G, C)), m


# ---------------------------------------------------------------------------------------------------------- mask_logits
@pytest.mark.parametrize("frame", FRAMES, ids=["landscape", "portrait"])
def test_mask_logits_threshold_is_mask_post(cuda, frame):
    """(mask_logits > 0) == mask_post's mask bit for bit; the logits within 2^-20 max|low-res| of torch's f32 interpolate and
    within 2^-18 max|low-res| of float64 interpolation (whose source coordinates are not rounded to f32)."""
    from lmx import kernels as K

    (h, w), (nh, nw) = frame
    g = torch.Generator().manual_seed(11)
    low = F.interpolate(torch.randn(3, 1, 12, 12, generator=g) * 10, size=(256, 256), mode="bilinear", align_corners=False)[:, 0].contiguous()
    d = low.to(cuda)
    lg = K.mask_logits(d, 1024, nh, nw, h, w)
    mask, _ = K.mask_post(d, 1024, nh, nw, h, w)
    assert torch.equal((lg > 0).to(torch.uint8), mask)
    lg = lg.cpu().double()
    top = float(low.abs().max())
    for name, ref, bound in (("torch f32", SP.postprocess_logits(d[:, None], (nh, nw), (h, w))[:, 0].cpu().double(), 2.0 ** -20 * top),
                             ("float64", SP.postprocess_logits(low.double()[:, None], (nh, nw), (h, w))[:, 0], 2.0 ** -18 * top)):
        r = float((lg - ref).abs().max()) / bound
        print(f"mask_logits {h}x{w} vs {name}: max ratio {_lg(r)}")
        assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------- decoder cases
# (name, points as fractions of (w, h), labels, box as fractions, mask_input seed, multimask)
CASES = [
    ("one positive point", [[0.4, 0.4]], [1], None, None, False),
    ("pos + neg + ignored", [[0.4, 0.4], [0.65, 0.6], [0.02, 0.85]], [1, 0, -1], None, None, True),
    ("2 points + box", [[0.3, 0.3], [0.47, 0.55]], [1, 0], [0.15, 0.14, 0.62, 0.83], None, False),
    ("box only, multimask", None, None, [0.15, 0.14, 0.62, 0.83], None, True),
    ("points + mask_input", [[0.4, 0.4], [0.7, 0.75]], [1, 1], None, 7, True),
    ("14 points, no box (T=20)", [[0.05 + 0.065 * i, 0.07 + 0.06 * i] for i in range(14)], [1, 0, -1, 1, 1, 0, 0, 1, -1, 1, 0, 1, 1, 0], None,
     None, True),
]
EMB_SEED = (5, 20)  # per frame: every reference mask of every case non-degenerate
_REF = {}


def _case_inputs(case, frame):
    name, fp, lab, fb, mseed, multimask = case
    (h, w), _ = frame
    pts = None if fp is None else (np.asarray(fp, np.float64) * [w, h]).astype(np.float32)[None]
    labels = None if lab is None else np.asarray(lab, np.int32)[None]
    box = None if fb is None else (np.asarray(fb, np.float64) * [w, h, w, h]).astype(np.float32)[None]
    mk = None if mseed is None else _mask_input(mseed)
    return pts, labels, box, mk, multimask


def _reference(ci, fi):
    key = (ci, fi)
    if key not in _REF:
        frame = FRAMES[fi]
        pts, labels, box, mk, multimask = _case_inputs(CASES[ci], frame)
        sd64 = SP.sd_as(_state(), torch.float64)
        with torch.no_grad():
            low, iou, _, _ = SP.predict(sd64, _emb(EMB_SEED[fi]).double(), frame[0], frame[1], pts, labels, box,
                                        None if mk is None else mk.double(), multimask)
            mask = SP.postprocess_logits(low, frame[1], frame[0]) > 0
        _REF[key] = (low, iou, mask)
    return _REF[key]


def _decode(dec, frame, case, cuda, precision, emb=None, fi=0):
    pts, labels, box, mk, multimask = _case_inputs(case, frame)
    e = _rows(_emb(EMB_SEED[fi]) if emb is None else emb).to(cuda)
    t = lambda a: None if a is None else torch.as_tensor(a).to(cuda)  # noqa: E731
    return dec.decode(e if precision == "exact" else e.half(), frame[0], frame[1], points=t(pts), labels=t(labels), boxes=t(box),
                      mask_input=t(mk), multimask=multimask, precision=precision)


def _mask_iou(a, b):
    u = float((a | b).sum())
    return float((a & b).sum()) / u if u else 1.0


@pytest.mark.parametrize("precision", ["exact", "f16"])
@pytest.mark.parametrize("fi", [0, 1], ids=["landscape", "portrait"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c[0] for c in CASES])
def test_decode_case_matches_float64(cuda, ci, fi, precision):
    """exact plan: low-res rel <= 1e-4 per mask, IoU-score abs <= 2e-4, mask IoU >= 0.9999; f16 plan: rel <= 2e-2, IoU >= 0.999."""
    from lmx import sam_decoder

    frame = FRAMES[fi]
    dec = sam_decoder.MaskDecoder(_state(), cuda)
    out = _decode(dec, frame, CASES[ci], cuda, precision, fi=fi)
    low_ref, iou_ref, mask_ref = _reference(ci, fi)
    low, iou, mask = out["lowres"].cpu().double(), out["iou"].cpu().double(), out["mask"].cpu().bool()
    C = 3 if CASES[ci][5] else 1
    assert low.shape == (1, C, 256, 256) and iou.shape == (1, C) and mask.shape == (1, C) + frame[0] and out["stats"].shape == (1, C, 8)
    rel_bar, iou_bar = (1e-4, 0.9999) if precision == "exact" else (2e-2, 0.999)
    worst = []
    for c in range(C):
        cov = float(mask_ref[0, c].float().mean())
        assert 0.02 < cov < 0.98, f"degenerate reference mask {c} (coverage {cov:.3f}): the test would not measure anything"
        rel = float((low[0, c] - low_ref[0, c]).norm() / low_ref[0, c].norm())
        miou = _mask_iou(mask[0, c], mask_ref[0, c])
        score = float((iou[0, c] - iou_ref[0, c]).abs())
        worst.append((rel / rel_bar, (1 - miou) / (1 - iou_bar), score / 2e-4))
        assert rel <= rel_bar and miou >= iou_bar, (c, rel, miou)
        if precision == "exact":
            assert score <= 2e-4, (c, score)
    w = np.max(np.asarray(worst), 0)
    print(f"decode [{CASES[ci][0]}] {frame[0]} {precision}: worst ratio rel {w[0]:.3g}, mask IoU {w[1]:.3g}, score {w[2]:.3g}")


@pytest.mark.parametrize("precision", ["exact", "f16"])
def test_decode_box_single_equals_predict(cuda, precision):
    from lmx import sam_decoder

    (h, w), rhw = FRAMES[0]
    dec = sam_decoder.MaskDecoder(_state(), cuda)
    e = _rows(_emb(8, 2)).to(cuda)
    e = e if precision == "exact" else e.half()
    boxes = torch.tensor([[300.0, 150.0, 1200.0, 900.0], [800.5, 400.25, 1000.0, 700.0]], device=cuda)
    a = dec.decode(e, (h, w), rhw, boxes=boxes, multimask=False, precision=precision)
    b = dec.predict(e, boxes, (h, w), rhw, precision=precision)
    assert torch.equal(a["lowres"][:, 0], b["lowres"]) and torch.equal(a["iou"][:, 0], b["iou"])
    assert torch.equal(a["mask"][:, 0], b["mask"]) and torch.equal(a["stats"][:, 0], b["stats"])


@pytest.mark.parametrize("precision", ["exact", "f16"])
def test_decode_is_batch_invariant(cuda, precision):
    """3 frames with different points (and mask inputs) in one call give the bits of each frame alone."""
    from lmx import sam_decoder

    frame = FRAMES[0]
    (h, w), rhw = frame
    dec = sam_decoder.MaskDecoder(_state(), cuda)
    e = _rows(_emb(9, 3)).to(cuda)
    e = e if precision == "exact" else e.half()
    pts = torch.tensor([[[700.0, 400.0], [1200.0, 650.0]], [[300.0, 200.0], [900.0, 800.0]], [[1500.0, 500.0], [10.0, 10.0]]], device=cuda)
    lab = torch.tensor([[1, 0], [1, 1], [1, -1]], dtype=torch.int32, device=cuda)
    mk = _mask_input(12, 3).to(cuda)
    whole = dec.decode(e, (h, w), rhw, points=pts, labels=lab, mask_input=mk, multimask=True, precision=precision)
    whole = {k: v.clone() for k, v in whole.items()}
    for j in range(3):
        alone = dec.decode(e[j * 4096:(j + 1) * 4096].contiguous(), (h, w), rhw, points=pts[j:j + 1].contiguous(),
                           labels=lab[j:j + 1].contiguous(), mask_input=mk[j:j + 1].contiguous(), multimask=True, precision=precision)
        for k in ("lowres", "iou", "mask", "stats"):
            assert torch.equal(whole[k][j:j + 1], alone[k]), (j, k)


# ---------------------------------------------------------------------------------------------------------- adapter idioms
@pytest.fixture(scope="module")
def predictor(cuda):
    from lmx import adapters, sam, synth, weights

    cfg = sam.SamVitConfig(hidden=128, layers=3, heads=2, mlp=256, global_idx=(1,), window=14, image=1024)
    sd = weights.synth_state_dict(sam.vit_param_spec(cfg), 61)
    sd.update(_state(62))
    pred = adapters.SamPredictor(adapters.LmxSam(cfg, sd, cuda))
    pred.set_image(synth.synth_frame(6, 20))
    return pred, sd


def _ref_from_adapter(pred, sd, **kw):
    emb = pred.get_image_embedding().cpu().double()
    with torch.no_grad():
        low, iou, _, _ = SP.predict(SP.sd_as(sd, torch.float64), emb, pred.original_size, pred.input_size, **kw)
        return low[0], iou[0], (SP.postprocess_logits(low, pred.input_size, pred.original_size) > 0)[0]


def test_adapter_box_defaults_to_three_masks(predictor):
    pred, sd = predictor
    emb = pred.get_image_embedding()
    assert emb.shape == (1, 256, 64, 64) and emb.dtype == torch.float32
    b = np.array([420.0, 360.0, 1010.0, 850.0])
    masks, scores, low = pred.predict(box=b)
    assert masks.shape == (3, 1080, 1920) and masks.dtype == bool and scores.shape == (3,) and low.shape == (3, 256, 256)
    low_ref, iou_ref, mask_ref = _ref_from_adapter(pred, sd, box=b[None], multimask=True)
    for c in range(3):
        assert _mask_iou(torch.from_numpy(masks[c]), mask_ref[c]) >= 0.9999
    assert np.abs(scores - iou_ref.numpy()).max() <= 2e-4


def test_adapter_points_and_refinement_loop(predictor):
    pred, sd = predictor
    pc, pl = np.array([[700.0, 500.0], [1100.0, 700.0]]), np.array([1, 0])
    masks, scores, low = pred.predict(point_coords=pc, point_labels=pl)
    assert masks.shape == (3, 1080, 1920) and scores.shape == (3,)
    _, iou_ref, mask_ref = _ref_from_adapter(pred, sd, points=pc[None], labels=pl[None], multimask=True)
    assert min(_mask_iou(torch.from_numpy(masks[c]), mask_ref[c]) for c in range(3)) >= 0.9999
    # segment_anything's refinement idiom: the best low-res mask fed back with the prompt, single-mask output
    mi = low[np.argmax(scores)][None]
    m2, s2, l2 = pred.predict(point_coords=pc, point_labels=pl, mask_input=mi, multimask_output=False)
    assert m2.shape == (1, 1080, 1920) and s2.shape == (1,) and l2.shape == (1, 256, 256)
    low_ref, iou_ref, mask_ref = _ref_from_adapter(pred, sd, points=pc[None], labels=pl[None], mask_input=torch.from_numpy(mi).double())
    assert _mask_iou(torch.from_numpy(m2[0]), mask_ref[0]) >= 0.9999
    assert float((torch.from_numpy(l2).double() - low_ref).norm() / low_ref.norm()) <= 1e-4
    # return_logits: the same call un-thresholded
    lg, s3, l3 = pred.predict(point_coords=pc, point_labels=pl, mask_input=mi, multimask_output=False, return_logits=True)
    assert lg.dtype == np.float32 and lg.shape == (1, 1080, 1920)
    assert np.array_equal(lg > 0, m2) and np.array_equal(s3, s2) and np.array_equal(l3, l2)


def test_adapter_rejects_malformed_prompts(predictor):
    pred, _ = predictor
    pc, pl = np.array([[700.0, 500.0]]), np.array([1])
    bad = [dict(point_coords=pc), dict(point_labels=pl), dict(point_coords=pc, point_labels=np.array([1, 0])),
           dict(point_coords=np.zeros((2, 3)), point_labels=np.array([1, 0])), dict(point_coords=pc, point_labels=np.array([2])),
           dict(point_coords=pc, point_labels=pl, mask_input=np.zeros((256, 256), np.float32)),
           dict(point_coords=pc, point_labels=pl, mask_input=np.zeros((1, 128, 128), np.float32)), dict(box=np.zeros(3)), dict()]
    for kw in bad:
        with pytest.raises(ValueError):
            pred.predict(**kw)
