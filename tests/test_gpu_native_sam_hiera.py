"""The model-level C API for SAM on a weight image whose encoder is Hiera (csrc/sam_hiera_model.h under csrc/sam_model.hip):
lmx_sam_encode is the launch sequence of HieraEncoder(band="blocks").encode(frames, outputs="embedding")["fpn"][2] written in C++ over
the plan lmx_h_hiera_plan computes — the same lmx_k_* entry points with the same descriptors — followed by the decoder path the ViT
images use, so the bar everywhere is EQUALITY with the Python plan (torch.equal / np.array_equal) on both decoder plans.  The C band
table is built from an all-zero frame; Python's from a real one, and band=False builds none: equality with both proves the table.
R8 is Hiera-B+ cut to eight blocks, one of every kind (tests/test_hiera_plan_c_host.py holds its plan and the frame sizes' properties:
(90, 160) a join inside the band, (139, 160) none before the global block's, (150, 100) and (64, 64) no band).  Synthetic weights."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_native_sam import OUT, ROOT, _assert_same, make_boxes, make_frames

pytestmark = pytest.mark.gpu
SIZES = {"90x160": (90, 160), "139x160": (139, 160), "150x100": (150, 100), "64x64": (64, 64)}
PLANS = ("f16", "exact")


def _r8():
    from lmx import sam

    return sam.HieraConfig(blocks=(2, 2, 3, 1), global_blocks=(6,))


class _Models:
    """Built once: the Python encoders (band="blocks" and band=False) and decoder with one set of weights, their weight image and (per
    max_batch) an open handle; the Python plan's results per (plan, size, n), computed once and left unchanged."""

    def __init__(self, dev, tmp, cfg, name):
        from lmx import native, sam, sam_decoder, weights

        self.dev, self._h, self._frames, self._ref = dev, {}, {}, {}
        sd = weights.synth_state_dict(sam.param_spec(cfg), 5)
        self.enc = sam.HieraEncoder(cfg, sd, dev, band="blocks")
        self.whole = sam.HieraEncoder(cfg, sd, dev, band=False)
        self.dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), dev)
        self.path = tmp / f"{name}.lmx"
        native.write_sam_image(self.enc, self.dec, self.path, PLANS)

    def handle(self, max_batch=3):
        from lmx import native

        if max_batch not in self._h:
            self._h[max_batch] = native.NativeSam(self.path, max_batch, self.dev)
        return self._h[max_batch]

    def frames(self, h, w, n=3):
        if (h, w, n) not in self._frames:
            self._frames[h, w, n] = (torch.from_numpy(make_frames(h, w, n)).to(self.dev), torch.from_numpy(make_boxes(h, w, n)).to(self.dev))
        return self._frames[h, w, n]

    def ref(self, plan, h, w, n=3):
        """the Python plan: dict(emb, mask, stats, iou, lowres, mask_bits, contour)"""
        from lmx import kernels as K
        from lmx import sam

        key = (plan, h, w, n)
        if key not in self._ref:
            frames, boxes = self.frames(h, w, n)
            emb = self.enc.encode(frames, outputs="embedding")["fpn"][2]
            d = self.dec.predict(emb.view(-1, 256), boxes, (h, w), sam.resize_longest_side(h, w, self.enc.cfg.image), plan)
            self._ref[key] = dict(emb=emb, mask=d["mask"], stats=d["stats"], iou=d["iou"].contiguous(), lowres=d["lowres"].contiguous(),
                                  mask_bits=K.pack_bits(d["mask"]), contour=K.contour_features(d["mask"]))
        return self._ref[key]

    def close(self):
        for nd in self._h.values():
            nd.close()


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_sam_hiera"), _r8(), "r8")
    yield m
    m.close()


@pytest.mark.parametrize("size", list(SIZES))
def test_encode_equals_python_plan(models, size):
    h, w = SIZES[size]
    frames, _ = models.frames(h, w)
    ns = models.handle()
    assert (ns.info.encoder, ns.info.hidden, ns.info.heads, ns.info.layers, ns.info.mlp, ns.info.window, ns.info.patch, ns.info.image, ns.info.plans,
            ns.info.max_batch) == (2, 112, 2, 8, 0, 8, 16, 1024, 3, 3) and ns.grid == 64
    want = models.ref("f16", h, w)["emb"]
    assert want.dtype == torch.float16 and tuple(want.shape) == (3, 64, 64, 256)
    for plan in PLANS:  # the trunk has one plan: f16 [n][64][64][256] whatever `precision` says
        got = ns.encode(frames, plan)
        assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got, want), f"{plan}: {int((got != want).sum())} of {got.numel()} elements differ from band='blocks'"
    whole = models.whole.encode(frames, outputs="embedding")["fpn"][2]
    assert torch.equal(got, whole), f"{int((got != whole).sum())} of {got.numel()} elements differ from band=False"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("size", ["90x160", "150x100"])
def test_decode_and_segment_equal_python_plan(models, plan, size):
    h, w = SIZES[size]
    frames, boxes = models.frames(h, w)
    want = models.ref(plan, h, w)
    ns = models.handle()
    _assert_same(ns.decode(want["emb"], boxes, (h, w), plan), want, what=f"decode {plan} {size}")
    got = ns.segment(frames, boxes, plan)
    _assert_same(got, want, what=f"segment {plan} {size}")
    _assert_same(ns.decode(ns.encode(frames, plan), boxes, (h, w), plan), got, what="encode then decode")


def test_an_output_left_out_corrupts_nothing(models):
    h, w = SIZES["139x160"]
    frames, boxes = models.frames(h, w)
    want = models.ref("exact", h, w)
    ns = models.handle()
    few = ns.segment(frames, boxes, "exact", outputs=("contour",))
    assert set(few) == {"contour", "stats", "iou"}
    _assert_same(few, want, keys=("contour", "stats", "iou"))
    _assert_same(ns.segment(frames, boxes, "exact"), want)


@pytest.mark.parametrize("plan", PLANS)
def test_chunks(models, plan):
    """n = 5 on a handle with max_batch = 2: chunks of 2, 2 and 1 equal the Python plan on the whole batch"""
    h, w = SIZES["90x160"]
    frames, boxes = models.frames(h, w, 5)
    want = models.ref(plan, h, w, 5)
    ns = models.handle(2)
    assert torch.equal(ns.encode(frames, plan), want["emb"])
    _assert_same(ns.segment(frames, boxes, plan), want, what=f"chunks {plan}")


@pytest.mark.parametrize("plan", PLANS)
def test_a_call_leaves_nothing_behind_for_the_next(models, cuda, plan):
    """n = 3, then 1, then 3 frames of 64 x 96 on ONE handle with max_batch = 3.  A call's buffers lie where its own walk of the plan
    puts them, so the smaller call lays them over what the larger one left and the larger one over that again: each result equals,
    bit for bit, that of a fresh handle given the same call alone."""
    from lmx import native

    frames, boxes = models.frames(64, 96, 3)
    with native.NativeSam(models.path, 3, cuda) as ns:
        for n in (3, 1, 3):
            f, b = frames[:n].contiguous(), boxes[:n].contiguous()
            got = ns.segment(f, b, plan)
            with native.NativeSam(models.path, 3, cuda) as fresh:
                want = fresh.segment(f, b, plan)
            _assert_same(got, want, what=f"{plan}, n = {n}")
            assert bool(torch.isfinite(want["lowres"]).all()) and float(want["lowres"].std()) > 0


def test_sizes_and_plans_alternate_and_handles_are_independent(models, cuda):
    from lmx import native

    ns = models.handle()
    other = native.NativeSam(models.path, 3, cuda)
    try:
        for _ in range(2):
            for size, plan in (("90x160", "f16"), ("64x64", "exact"), ("90x160", "exact"), ("139x160", "f16")):
                h, w = SIZES[size]
                frames, boxes = models.frames(h, w)
                _assert_same(ns.segment(frames, boxes, plan), models.ref(plan, h, w), what=f"{size} {plan}")
                if size == "90x160":
                    _assert_same(other.segment(frames, boxes, plan), models.ref(plan, h, w), what=f"second handle {size} {plan}")
    finally:
        other.close()


def test_max_batch_1_with_a_band(models):
    """the table pass runs one frame on the whole grid: more room than the band's workspace of one frame has"""
    h, w = SIZES["90x160"]
    frames, boxes = models.frames(h, w)
    ns = models.handle(1)
    for plan in PLANS:
        _assert_same(ns.segment(frames, boxes, plan), models.ref(plan, h, w), what=f"max_batch 1 {plan}")


def test_segment_only_enqueues_on_the_callers_stream(models, cuda):
    h, w = SIZES["90x160"]
    frames, boxes = models.frames(h, w)
    want = models.ref("exact", h, w)
    ns = models.handle()
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
    side.synchronize()
    assert returned_early, "lmx_sam_segment returned only after the work queued ahead of it had finished: it synchronised"
    _assert_same(got, want)


def test_host_entry_equals_device_entry(models):
    h, w = SIZES["139x160"]
    frames, boxes = models.frames(h, w, 5)
    ns = models.handle(2)
    for plan in PLANS:
        dev_out = ns.segment(frames, boxes, plan)
        host_out = ns.segment_host(frames.cpu().numpy(), boxes.cpu().numpy(), plan)
        assert set(host_out) == set(dev_out) == set(OUT)
        for k in OUT:
            d = dev_out[k].cpu().numpy()
            assert host_out[k].dtype == d.dtype and host_out[k].shape == d.shape and np.array_equal(host_out[k], d), (plan, k)


def test_errors_are_returned_not_faults(models, cuda, tmp_path):
    """bad arguments only: every refused call is refused on the host, before any launch; the handle still segments afterwards"""
    from lmx import native

    lib = native._lib.load()
    err = lambda: lib.lmx_last_error().decode()
    h, w = SIZES["90x160"]
    frames, boxes = models.frames(h, w)
    ns = models.handle()
    stats, iou = torch.empty((3, 8), dtype=torch.int64, device=cuda), torch.empty((3,), dtype=torch.float32, device=cuda)

    def seg(n=3, prec=0, st=stats.data_ptr(), handle=ns._h):
        return lib.lmx_sam_segment(handle, frames.data_ptr(), n, h, w, boxes.data_ptr(), prec, None, None, st, None, iou.data_ptr(), None, None)

    with torch.cuda.device(cuda):
        assert seg(st=None) == -1 and "null pointer (stats" in err()
        assert seg(n=0) == -1 and "n = 0" in err()
        assert seg(n=-1) == -1 and "n = -1" in err()
        assert seg(prec=7) == -1 and "precision 7" in err()
    f16_only = tmp_path / "f16.lmx"
    native.write_sam_image(models.enc, models.dec, f16_only, ("f16",))
    n16 = native.NativeSam(f16_only, 2, cuda)
    try:
        with pytest.raises(native.LmxError, match="does not hold the exact plan"):
            n16.prepare(h, w, "exact")
    finally:
        n16.close()
    huge = native.NativeSam(models.path, 4000, cuda)  # 4000 frames: the patch matrix alone passes 2 GB
    try:
        with pytest.raises(native.LmxError, match="buffer '.*' .*2 GB"):
            huge.prepare(h, w, "f16")
    finally:
        huge.close()
    if torch.cuda.device_count() >= 2:
        with torch.cuda.device(torch.device("cuda", 1)):
            assert seg() == -1 and "the current device is 1" in err()
    _assert_same(ns.segment(frames, boxes, "f16"), models.ref("f16", h, w))


@pytest.mark.parametrize("plan", PLANS)
def test_real_size_hiera_b_plus(cuda, tmp_path, plan):
    """Full Hiera-B+ at 1080 x 1920, n = 2: the embedding and every output equal the Python plan"""
    from lmx import sam

    m = _Models(cuda, tmp_path, sam.hiera_b_plus(), "bplus")
    try:
        frames, boxes = m.frames(1080, 1920, 2)
        want = m.ref(plan, 1080, 1920, 2)
        ns = m.handle(2)
        assert torch.equal(ns.encode(frames, plan), want["emb"])
        _assert_same(ns.segment(frames, boxes, plan), want, what=f"Hiera-B+ {plan}")
    finally:
        m.close()


def test_c_example_gives_the_python_masks(models, tmp_path):
    """examples/sam_segment.c, unchanged, compiled with cc against liblmx.so and run as a child process on the R8 image"""
    from lmx import _lib

    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    h, w = SIZES["90x160"]
    frames, boxes = models.frames(h, w, 5)
    want = models.ref("exact", h, w, 5)
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(np.array([5, h, w], np.int32).tobytes())
        f.write(frames.cpu().numpy().tobytes())
        f.write(boxes.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "sam_segment"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sam_segment.c"),
                    "-o", str(exe), "-L", libdir, "-llmx", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], check=True, timeout=120)
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
    r = subprocess.run([str(exe), str(models.path), str(raw), str(out), "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == b"".join(want[k].cpu().numpy().tobytes() for k in ("mask_bits", "stats", "iou"))
