"""The model-level C API for SAM on the GPU (include/lmx.h "MODEL level: SAM", csrc/sam_model.hip): lmx_sam_encode / lmx_sam_decode /
lmx_sam_segment are the launch sequences of SamVitEncoder.encode and MaskDecoder.predict written in C++ — the same lmx_k_* entry points
with the same descriptors — so the bar everywhere is EQUALITY with the Python plan (torch.equal / np.array_equal) on both precision
plans; tests/test_gpu_sam.py in turn holds the Python plans to the fp32 oracle.  Synthetic weights, synthetic frames.
Reduced encoders (image / patch / window stay 1024 / 16 / 14, the decoder's grid 64):
  S64  hidden 192, 3 heads (head dim 64), one windowed then one global layer; image with both plans
  S80  hidden 320, 4 heads (head dim 80: the attention kernels' 96-wide class ViT-H uses), global first, then windowed; f16 plan only"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# padding rows (nh < 1024), padding columns (nw < 1024), no padding
# 139x157: w % 4 == 1 and w % 8 == 5 (mask rows at every byte residue, a partial last byte per row of mask_bits)
SIZES = {"96x160": (96, 160), "150x100": (150, 100), "64x64": (64, 64), "139x157": (139, 157)}
IMAGE_PLANS = {"S64": ("f16", "exact"), "S80": ("f16",)}
GRID = [(name, plan) for name, plans in IMAGE_PLANS.items() for plan in plans]
OUT = ("mask", "stats", "iou", "lowres", "mask_bits", "contour")


def _config(name):
    from lmx import sam

    if name == "S64":
        return sam.SamVitConfig(hidden=192, heads=3, layers=2, mlp=384, global_idx=(1,))
    if name == "S80":
        return sam.SamVitConfig(hidden=320, heads=4, layers=2, mlp=640, global_idx=(0,))
    return sam.sam_vit_b()


def make_frames(h, w, n, seed=0):
    """u8 [n,h,w,3]: seeded noise with a few bright rectangles per frame"""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    f = rng.integers(0, 96, (n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        for _ in range(3):
            rh, rw = int(rng.integers(max(h // 6, 2), max(h // 2, 3))), int(rng.integers(max(w // 6, 2), max(w // 2, 3)))
            y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
            f[i, y0:y0 + rh, x0:x0 + rw] = rng.integers(180, 256, (3,), dtype=np.uint8)
    return f


def make_boxes(h, w, n):
    """f32 [n,4] xyxy in frame pixels, cycling through: inside the frame, touching two borders, all-zero (the "no detection" box of
    lmx/pipeline.py)"""
    kinds = [(0.25 * w, 0.25 * h, 0.75 * w, 0.7 * h), (0.0, 0.0, 0.6 * w, 0.5 * h), (0.0, 0.0, 0.0, 0.0)]
    return np.array([kinds[i % 3] for i in range(n)], np.float32)


class _Models:
    """Per model, built once: the Python encoder and decoder, their weight image and (per max_batch) an open handle; the Python plan's
    results per (model, plan, size, n), computed once and left unchanged."""

    def __init__(self, dev, tmp):
        self.dev, self.tmp, self._m, self._h, self._frames, self._ref = dev, tmp, {}, {}, {}, {}

    def model(self, name):
        from lmx import native, sam, sam_decoder, weights

        if name not in self._m:
            cfg = _config(name)
            enc = sam.SamVitEncoder(cfg, weights.synth_state_dict(sam.vit_param_spec(cfg), 5), self.dev)
            dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), self.dev)
            path = self.tmp / f"{name}.lmx"
            native.write_sam_image(enc, dec, path, IMAGE_PLANS[name])
            self._m[name] = (enc, dec, path)
        return self._m[name]

    def handle(self, name, max_batch=3):
        from lmx import native

        if (name, max_batch) not in self._h:
            self._h[name, max_batch] = native.NativeSam(self.model(name)[2], max_batch, self.dev)
        return self._h[name, max_batch]

    def frames(self, h, w, n=3):
        if (h, w, n) not in self._frames:
            self._frames[h, w, n] = (torch.from_numpy(make_frames(h, w, n)).to(self.dev), torch.from_numpy(make_boxes(h, w, n)).to(self.dev))
        return self._frames[h, w, n]

    def ref(self, name, plan, h, w, n=3):
        """the Python plan: dict(emb, mask, stats, iou, lowres, mask_bits, contour)"""
        key = (name, plan, h, w, n)
        if key not in self._ref:
            self._ref[key] = py_segment(self.model(name), *self.frames(h, w, n), plan)
        return self._ref[key]

    def close(self):
        for nd in self._h.values():
            nd.close()


def py_segment(model, frames, boxes, plan):
    from lmx import kernels as K
    from lmx import sam

    enc, dec, _ = model
    n, h, w, _ = frames.shape
    emb = enc.encode(frames, plan)["fpn"][2]
    d = dec.predict(emb.view(-1, 256), boxes, (h, w), sam.resize_longest_side(h, w, enc.cfg.image), plan)
    return dict(emb=emb, mask=d["mask"], stats=d["stats"], iou=d["iou"].contiguous(), lowres=d["lowres"].contiguous(), mask_bits=K.pack_bits(d["mask"]),
                contour=K.contour_features(d["mask"]))


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_sam"))
    yield m
    m.close()


def _assert_same(got, want, keys=OUT, what=""):
    assert set(got) == set(keys), (what, sorted(got))
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), f"{what} {k}: {g.dtype} {tuple(g.shape)} against {w.dtype} {tuple(w.shape)}"
        assert torch.equal(g, w), f"{what} {k}: {int((g != w).sum())} of {g.numel()} elements differ"


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name,plan", GRID)
def test_encode_equals_python_plan(models, name, plan, size):
    h, w = SIZES[size]
    frames = models.frames(h, w)[0][:2].contiguous()
    want = models.model(name)[0].encode(frames, plan)["fpn"][2]
    ns = models.handle(name)
    got = ns.encode(frames, plan)
    assert got.dtype == want.dtype == (torch.float32 if plan == "exact" else torch.float16) and tuple(got.shape) == tuple(want.shape) == (2, 64, 64, 256)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} elements differ"
    from lmx import sam

    assert ns.resized(h, w) == sam.resize_longest_side(h, w, 1024)


def test_resized_equals_resize_longest_side(models):
    """lmx_sam_resized against ResizeLongestSide.get_preprocess_shape (it takes a handle, so it is held here and not in the host tests)"""
    from lmx import sam

    ns = models.handle("S64")
    sizes = [(1080, 1920), (1920, 1080), (64, 64), (1, 1024), (683, 1024)]
    assert [ns.resized(h, w) for h, w in sizes] == [sam.resize_longest_side(h, w, 1024) for h, w in sizes]
    assert ns.resized(1080, 1920) == (576, 1024)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name,plan", GRID)
def test_decode_equals_python_plan(models, name, plan, size):
    h, w = SIZES[size]
    _, boxes = models.frames(h, w)
    want = models.ref(name, plan, h, w)
    got = models.handle(name).decode(want["emb"], boxes, (h, w), plan)
    _assert_same(got, want, what=f"{name} {plan} {size}")
    areas = want["stats"][:, 0].tolist()
    print(f"{name} {plan} {size}: mask areas {areas} iou {want['iou'].tolist()}")
    info = models.handle(name).info
    cfg = models.model(name)[0].cfg
    assert (info.encoder, info.hidden, info.heads, info.layers, info.mlp, info.window, info.patch, info.image, info.plans, info.max_batch) == \
        (0, cfg.hidden, cfg.heads, cfg.layers, cfg.mlp, 14, 16, 1024, 3 if name == "S64" else 1, 3)


@pytest.mark.parametrize("name,plan", GRID)
def test_segment_equals_encode_then_decode(models, name, plan):
    h, w = SIZES["96x160"]
    frames, boxes = models.frames(h, w)
    want = models.ref(name, plan, h, w)
    ns = models.handle(name)
    _assert_same(ns.segment(frames, boxes, plan), want, what=f"{name} {plan}")
    two_step = ns.decode(ns.encode(frames, plan), boxes, (h, w), plan)
    _assert_same(two_step, want, what=f"{name} {plan} encode + decode")


@pytest.mark.parametrize("plan", ["f16", "exact"])
def test_segment_at_an_odd_width(models, plan):
    """139 x 157: the handle carves mask, mask_bits and contour space out of one workspace, here with w % 4 != 0 and w % 8 != 0;
    besides equality with the Python plan, mask_bits is numpy.packbits of the mask that came back with it."""
    h, w = SIZES["139x157"]
    frames, boxes = models.frames(h, w)
    want = models.ref("S64", plan, h, w)
    got = models.handle("S64").segment(frames, boxes, plan)
    _assert_same(got, want, what=f"S64 {plan} 139x157")
    mask = got["mask"].cpu().numpy()
    assert mask.shape == (3, h, w) and set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(got["mask_bits"].cpu().numpy(), np.packbits(mask, axis=-1))
    areas = want["stats"][:, 0].tolist()
    print(f"S64 {plan} 139x157: mask areas {areas}")
    assert any(0 < a < h * w for a in areas), "every reference mask is empty or full: the bits say nothing"


def test_an_output_left_out_corrupts_nothing(models):
    """every optional output NULL except one in turn, and all of them NULL: what goes to the workspace instead leaves the rest right"""
    h, w = SIZES["150x100"]
    frames, boxes = models.frames(h, w)
    want = models.ref("S64", "exact", h, w)
    ns = models.handle("S64")
    for only in (("mask",), ("mask_bits",), ("contour",), ("lowres",), ()):
        got = ns.segment(frames, boxes, "exact", outputs=only)
        _assert_same(got, want, keys=("stats", "iou") + only, what=f"outputs {only}")
    _assert_same(ns.segment(frames, boxes, "exact"), want)


def test_the_services_frame_size(models):
    """one 1080 x 1920 frame under the services' plan"""
    frames, boxes = models.frames(1080, 1920, 1)
    want = models.ref("S64", "exact", 1080, 1920, 1)
    got = models.handle("S64").segment(frames, boxes, "exact")
    _assert_same(got, want)
    assert int(want["stats"][0, 0]) > 0 and int(want["contour"][0, 7]) > 0, "the reference mask is empty: nothing was compared"


@pytest.mark.parametrize("plan", ["f16", "exact"])
def test_real_size_vit_b(cuda, tmp_path, plan):
    """sam_vit_b() (768 wide, 12 layers, mlp 3072): workspace sizes, leading dimensions and the 2 GB guard scale with the real N and K"""
    from lmx import native, sam, sam_decoder, weights

    cfg = sam.sam_vit_b()
    enc = sam.SamVitEncoder(cfg, weights.synth_state_dict(sam.vit_param_spec(cfg), 5), cuda)
    dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), cuda)
    path = tmp_path / "vit_b.lmx"
    try:
        native.write_sam_image(enc, dec, path, (plan,))
        frames, boxes = (torch.from_numpy(a).to(cuda) for a in (make_frames(96, 160, 1), make_boxes(96, 160, 1)))
        want = py_segment((enc, dec, path), frames, boxes, plan)
        with native.NativeSam(path, 1, cuda) as ns:
            assert (ns.info.hidden, ns.info.layers, ns.info.plans) == (768, 12, 1 << native.PLANS[plan])
            got = ns.segment(frames, boxes, plan)
            _assert_same(got, want)
            assert torch.equal(ns.encode(frames, plan), want["emb"])
        # a workspace beyond what the kernels' index arithmetic accepts: refused at prepare, with the buffer named, before anything is allocated
        with native.NativeSam(path, 200, cuda) as big:
            with pytest.raises(native.LmxError, match="buffer '.*the kernels index below 2 GB"):
                big.prepare(96, 160, plan)
    finally:
        path.unlink(missing_ok=True)


@pytest.mark.parametrize("plan", ["f16", "exact"])
def test_chunks(models, plan):
    """n = 5 with max_batch 2 (chunks of 2, 2, 1) equals n = 5 with max_batch 5, and both equal the Python plan on the 5 frames"""
    h, w = SIZES["150x100"]
    frames, boxes = models.frames(h, w, 5)
    want = models.ref("S64", plan, h, w, 5)
    in_chunks = models.handle("S64", 2).segment(frames, boxes, plan)
    at_once = models.handle("S64", 5).segment(frames, boxes, plan)
    _assert_same(in_chunks, at_once, what="max_batch 2 against max_batch 5")
    _assert_same(at_once, want, what="max_batch 5 against Python")
    assert torch.equal(models.handle("S64", 2).encode(frames, plan), want["emb"])


@pytest.mark.parametrize("plan", ["f16", "exact"])
def test_a_call_leaves_nothing_behind_for_the_next(models, cuda, plan):
    """n = 3, then 1, then 3 frames of 64 x 96 on ONE handle with max_batch = 3.  A call's buffers lie where its own walk of the plan
    puts them, so the smaller call lays them over what the larger one left and the larger one over that again: each result equals,
    bit for bit, that of a fresh handle given the same call alone."""
    from lmx import native

    frames, boxes = models.frames(64, 96, 3)
    path = models.model("S64")[2]
    with native.NativeSam(path, 3, cuda) as ns:
        for n in (3, 1, 3):
            f, b = frames[:n].contiguous(), boxes[:n].contiguous()
            got = ns.segment(f, b, plan)
            with native.NativeSam(path, 3, cuda) as fresh:
                want = fresh.segment(f, b, plan)
            _assert_same(got, want, what=f"{plan}, n = {n}")
            assert bool(torch.isfinite(want["lowres"]).all()) and float(want["lowres"].std()) > 0


def test_two_sizes_alternate_on_one_handle(models):
    ns = models.handle("S64")
    (fa, ba), (fb, bb) = models.frames(*SIZES["96x160"]), models.frames(*SIZES["150x100"])
    wa, wb = models.ref("S64", "exact", *SIZES["96x160"]), models.ref("S64", "exact", *SIZES["150x100"])
    ga1, gb, ga2 = ns.segment(fa, ba, "exact"), ns.segment(fb, bb, "exact"), ns.segment(fa, ba, "exact")
    _assert_same(ga1, wa)
    _assert_same(gb, wb)
    _assert_same(ga2, wa)


def test_two_plans_alternate_on_one_handle(models):
    ns = models.handle("S64")
    h, w = SIZES["64x64"]
    f, b = models.frames(h, w)
    wf, wx = models.ref("S64", "f16", h, w), models.ref("S64", "exact", h, w)
    g1, g2, g3 = ns.segment(f, b, "f16"), ns.segment(f, b, "exact"), ns.segment(f, b, "f16")
    _assert_same(g1, wf)
    _assert_same(g2, wx)
    _assert_same(g3, wf)
    assert not torch.equal(wf["lowres"], wx["lowres"]), "the two plans give the same bits: nothing alternated"


def test_two_handles_are_independent(models, cuda):
    from lmx import native

    h, w = SIZES["96x160"]
    f, b = models.frames(h, w)
    w1, w2 = models.ref("S64", "f16", h, w), models.ref("S80", "f16", h, w)
    h1, h2 = native.NativeSam(models.model("S64")[2], 3, cuda), native.NativeSam(models.model("S80")[2], 3, cuda)
    try:
        _assert_same(h1.segment(f, b, "f16"), w1)
        _assert_same(h2.segment(f, b, "f16"), w2)
        _assert_same(h1.segment(f, b, "f16"), w1)
        h1.close()
        with pytest.raises(native.LmxError, match="closed"):
            h1.segment(f, b, "f16")
        _assert_same(h2.segment(f, b, "f16"), w2)
    finally:
        h1.close()
        h2.close()
    assert not torch.equal(w1["lowres"], w2["lowres"])


def test_a_handle_keeps_16_prepared_pairs(models, cuda):
    """16 (frame size, plan) pairs are kept, the 17th is refused by prepare and by segment alike, and the first sixteen still serve"""
    from lmx import native

    h, w = SIZES["64x64"]
    f, b = models.frames(h, w, 1)
    with native.NativeSam(models.model("S64")[2], 1, cuda) as ns:
        ns.prepare(h, w, "f16")
        for i in range(15):
            ns.prepare(33 + i, 40, "f16")
        with pytest.raises(native.LmxError, match="already holds 16"):
            ns.prepare(33 + 15, 40, "f16")
        with pytest.raises(native.LmxError, match="already holds 16"):
            ns.prepare(h, w, "exact")  # a held size under the other plan is another pair
        f2, b2 = models.frames(*SIZES["96x160"], 1)
        with pytest.raises(native.LmxError, match="already holds 16"):
            ns.segment(f2, b2, "f16")
        _assert_same(ns.segment(f, b, "f16"), models.ref("S64", "f16", h, w, 1))
        small = torch.from_numpy(make_frames(33 + 14, 40, 1)).to(cuda)
        sb = torch.from_numpy(make_boxes(33 + 14, 40, 1)).to(cuda)
        _assert_same(ns.segment(small, sb, "f16"), py_segment(models.model("S64"), small, sb, "f16"))


def test_segment_only_enqueues_on_the_callers_stream(models, cuda):
    """After lmx_sam_prepare, segment on a side stream with work queued ahead of it: the call returns while that work is still running
    (it neither synchronises nor allocates through a synchronising call), and a consumer on the same stream reads the right outputs."""
    h, w = SIZES["96x160"]
    frames, boxes = models.frames(h, w)
    want = models.ref("S64", "exact", h, w)
    ns = models.handle("S64")
    ns.prepare(h, w, "exact")
    ns.segment(frames, boxes, "exact")  # every kernel's code object is on the device after this
    a = torch.randn((8192, 8192), device=cuda)
    c = torch.empty_like(a)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    ahead = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(24):  # some hundred milliseconds of f32 GEMM in front of the call
            torch.matmul(a, a, out=c)
        ahead.record(side)
        got = ns.segment(frames, boxes, "exact")
        returned_early = not ahead.query()
        z = got["stats"].float().sum(1) + got["iou"] + got["lowres"].sum((1, 2))
    side.synchronize()
    assert returned_early, "lmx_sam_segment returned only after the work queued ahead of it had finished: it synchronised"
    _assert_same(got, want)
    assert torch.equal(z, want["stats"].float().sum(1) + want["iou"] + want["lowres"].sum((1, 2)))


@pytest.mark.parametrize("plan", ["f16", "exact"])
def test_host_entry_equals_device_entry(models, plan):
    h, w = SIZES["150x100"]
    frames, boxes = models.frames(h, w, 5)
    ns = models.handle("S64", 2)
    dev_out = ns.segment(frames, boxes, plan)
    host_out = ns.segment_host(frames.cpu().numpy(), boxes.cpu().numpy(), plan)
    assert set(host_out) == set(dev_out) == set(OUT)
    for k in OUT:
        d = dev_out[k].cpu().numpy()
        assert host_out[k].dtype == d.dtype and host_out[k].shape == d.shape and np.array_equal(host_out[k], d), k
    few = ns.segment_host(frames.cpu().numpy(), boxes.cpu().numpy(), plan, outputs=("mask_bits",))
    assert set(few) == {"mask_bits", "stats", "iou"} and all(np.array_equal(few[k], host_out[k]) for k in few)


def test_errors_are_returned_not_faults(models, cuda):
    """every refused call is refused on the host, before any launch, with the argument named; the handles still segment afterwards"""
    from lmx import native

    lib = native._lib.load()
    err = lambda: lib.lmx_last_error().decode()
    h, w = SIZES["96x160"]
    frames, boxes = models.frames(h, w)
    ns, n80 = models.handle("S64"), models.handle("S80")
    out = dict(mask=torch.empty((3, h, w), dtype=torch.uint8, device=cuda), bits=torch.empty((3, h, (w + 7) // 8), dtype=torch.uint8, device=cuda),
               stats=torch.empty((3, 8), dtype=torch.int64, device=cuda), contour=torch.empty((3, 8), dtype=torch.int64, device=cuda),
               iou=torch.empty((3,), dtype=torch.float32, device=cuda), lowres=torch.empty((3, 256, 256), dtype=torch.float32, device=cuda))
    emb = torch.empty((3, 64, 64, 256), dtype=torch.float16, device=cuda)

    def seg(handle=ns._h, f=frames.data_ptr(), n=3, hh=h, ww=w, b=boxes.data_ptr(), prec=0, fn=lib.lmx_sam_segment, **over):
        p = {k: t.data_ptr() for k, t in out.items()}
        p.update(over)
        return fn(handle, f, n, hh, ww, b, prec, p["mask"], p["bits"], p["stats"], p["contour"], p["iou"], p["lowres"], None)

    with torch.cuda.device(cuda):
        assert seg(handle=None) == -1 and "null handle" in err()
        assert seg(f=None) == -1 and "null pointer (frames)" in err()
        assert seg(b=None) == -1 and "null pointer (boxes)" in err()
        assert seg(stats=None) == -1 and "null pointer (stats" in err()
        assert seg(iou=None) == -1 and "null pointer (iou" in err()
        assert seg(n=0) == -1 and "n = 0" in err()
        assert seg(n=-2) == -1 and "n = -2" in err()
        assert seg(hh=0) == -1 and "frame size 0 x 160" in err()
        assert seg(ww=-1) == -1 and "frame size 96 x -1" in err()
        assert seg(prec=7) == -1 and "precision 7" in err()
        assert seg(handle=n80._h, prec=1) == -1 and "does not hold the exact plan" in err()
        # the same checks guard decode and encode
        assert seg(fn=lib.lmx_sam_decode, f=None) == -1 and "null pointer (emb)" in err()
        assert seg(fn=lib.lmx_sam_decode, f=emb.data_ptr(), iou=None) == -1 and "null pointer (iou" in err()
        assert seg(fn=lib.lmx_sam_decode, f=emb.data_ptr(), prec=7) == -1 and "precision 7" in err()
        assert lib.lmx_sam_encode(ns._h, None, 3, h, w, 0, emb.data_ptr(), None) == -1 and "null pointer (frames)" in err()
        assert lib.lmx_sam_encode(ns._h, frames.data_ptr(), 3, h, w, 0, None, None) == -1 and "null pointer (emb)" in err()
        assert lib.lmx_sam_encode(None, frames.data_ptr(), 3, h, w, 0, emb.data_ptr(), None) == -1 and "null handle" in err()
        assert lib.lmx_sam_prepare(ns._h, h, w, 7) == -1 and "precision 7" in err()
        assert lib.lmx_sam_prepare(ns._h, 0, w, 0) == -1 and "frame size" in err()
        assert lib.lmx_sam_resized(ns._h, h, w, None, None) == -1 and "null" in err()
        # contour features outside lmx_k_contour_features' range are refused, not launched: a frame of one row
        assert seg(hh=1) == -1 and "contour" in err()
    with pytest.raises(native.LmxError, match="does not hold the exact plan"):
        n80.prepare(h, w, "exact")
    for mb in (0, -3):
        with pytest.raises(native.LmxError, match="max_batch"):
            native.NativeSam(models.model("S64")[2], mb, cuda)
    with pytest.raises(native.LmxError, match="cannot open"):
        native.NativeSam(str(models.model("S64")[2]) + ".absent", 2, cuda)
    if torch.cuda.device_count() >= 2:  # another device's stream, and another current device
        other = torch.device("cuda", 1)
        s1 = torch.cuda.Stream(device=other)
        with torch.cuda.device(cuda):
            p = {k: t.data_ptr() for k, t in out.items()}
            rc = lib.lmx_sam_segment(ns._h, frames.data_ptr(), 3, h, w, boxes.data_ptr(), 0, p["mask"], p["bits"], p["stats"], p["contour"], p["iou"],
                                     p["lowres"], s1.cuda_stream)
            assert rc == -1 and "the stream belongs to device 1" in err()
        with torch.cuda.device(other):
            assert seg() == -1 and "the current device is 1" in err()
    # the handles that saw the errors still give the right answer
    _assert_same(ns.segment(frames, boxes, "f16"), models.ref("S64", "f16", h, w))
    _assert_same(ns.segment(frames, boxes, "exact"), models.ref("S64", "exact", h, w))
    _assert_same(n80.segment(frames, boxes, "f16"), models.ref("S80", "f16", h, w))


def test_c_example_gives_the_python_masks(models, tmp_path):
    """examples/sam_segment.c, compiled with cc against liblmx.so and run as a child process on the exported S64 image: its output file
    holds the Python plan's bytes (exact plan, chunks of 2).  The child's loader is pointed at the HIP runtime this process loaded."""
    from lmx import _lib

    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    h, w = SIZES["150x100"]
    frames, boxes = models.frames(h, w, 5)
    want = models.ref("S64", "exact", h, w, 5)
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(np.array([5, h, w], np.int32).tobytes())
        f.write(frames.cpu().numpy().tobytes())
        f.write(boxes.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "sam_segment"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sam_segment.c"),
                    "-o", str(exe), "-L", libdir, "-llmx", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], check=True, timeout=120)
    # the HIP runtime torch loaded, first on the child's search path; where its file does not carry the soname liblmx.so asks for,
    # a link of that name in a directory behind it
    hip = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(hip) == 1, hip
    hipdir = os.path.dirname(hip[0])
    soname = "libamdhip64.so.7"
    search = [hipdir]
    if not os.path.exists(os.path.join(hipdir, soname)):
        rt = tmp_path / "rt"
        rt.mkdir()
        os.symlink(hip[0], rt / soname)
        search.append(str(rt))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(search + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
    out = tmp_path / "masks.bin"
    r = subprocess.run([str(exe), str(models.model("S64")[2]), str(raw), str(out), "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == b"".join(want[k].cpu().numpy().tobytes() for k in ("mask_bits", "stats", "iou"))
