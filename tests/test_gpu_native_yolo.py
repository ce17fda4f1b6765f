"""The model-level C API for YOLO on the GPU (include/lmx.h "MODEL level: YOLOv8", csrc/yolo_model.hip): lmx_yolo_predict /
lmx_yolo_detect are the launch sequence of YoloDetector written in C++ — the same lmx_k_* entry points with the same descriptors —
so the bar everywhere is EQUALITY with the Python plan (torch.equal / equal bytes) on both precision plans and for a pose model;
tests/test_gpu_yolo.py in turn holds the Python plan to the fp32 oracle.  imgsz 320, synthetic weights (seed 7 with the package's
BatchNorm statistics), synthetic frames."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_SHAPE = (17, 3)
MODELS = ("n", "l", "pose")
PLANS = ("f16", "exact")
# 1080p: downscale, top / bottom padding; 180x320: no resize (NULL tables), padding only; 481x270: portrait, left / right padding;
# 320x320: no resize, no padding; 37x53: scaleup
SIZES = {"1080x1920": (1080, 1920), "180x320": (180, 320), "481x270": (481, 270), "320x320": (320, 320), "37x53": (37, 53)}
# per model, the (conf, iou) of the low-confidence run, chosen from the Python plan alone: at it the Python plan fills max_det = 300
# and max_det = 7 on at least one frame of every size (asserted in test_detect_equals_python_plan).  The pose model has ONE class,
# so at the default iou 0.7 NMS alone keeps fewer than 300 of its 1260 .. 1470 anchors on the padded sizes: its low run raises iou.
LOW = {"n": (0.1, 0.7), "l": (0.1, 0.7), "pose": (0.001, 0.9)}
# the other (conf, iou) runs: the service's 0.25, at which n and l keep some tens of detections per frame; the synthetic pose model's best
# score is below 0.25, so it also runs at 0.05, where the Python plan keeps some tens (a frame with >= 1 and < max_det detections)
OTHER = {"n": [(0.25, 0.7)], "l": [(0.25, 0.7)], "pose": [(0.25, 0.7), (0.05, 0.7)]}


def _config(name):
    from lmx import yolo

    if name == "pose":  # the configuration tests/test_gpu_yolo.py uses, so that the package's BatchNorm statistics fit
        return yolo.YoloConfig("n", nc=1, imgsz=320, kpt_shape=POSE_SHAPE), yolo.bn_stats_path("n", pose=True)
    return yolo.YoloConfig(name, nc=80, imgsz=320), yolo.bn_stats_path(name)


def make_frames(h, w, n, seed=0):
    """u8 BGR [n,h,w,3]: seeded noise with a few bright rectangles per frame"""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    f = rng.integers(0, 96, (n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        for _ in range(3):
            rh, rw = int(rng.integers(max(h // 6, 2), max(h // 2, 3))), int(rng.integers(max(w // 6, 2), max(w // 2, 3)))
            y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
            f[i, y0:y0 + rh, x0:x0 + rw] = rng.integers(180, 256, (3,), dtype=np.uint8)
    return f


class _Models:
    """Per model, built once: the Python detector, its weight image (both plans) and (per max_batch) an open handle."""

    def __init__(self, dev, tmp):
        self.dev, self.tmp, self._m, self._h, self._frames = dev, tmp, {}, {}, {}

    def model(self, name):
        from lmx import native, yolo

        if name not in self._m:
            cfg, bn = _config(name)
            det = yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7, bn), self.dev)
            path = self.tmp / f"{name}.lmx"
            native.write_yolo_image(det, path)
            self._m[name] = (det, path)
        return self._m[name]

    def handle(self, name, max_batch=4):
        from lmx import native

        if (name, max_batch) not in self._h:
            self._h[name, max_batch] = native.NativeYolo(self.model(name)[1], max_batch, self.dev)
        return self._h[name, max_batch]

    def frames(self, h, w, n=2):
        if (h, w, n) not in self._frames:
            self._frames[h, w, n] = torch.from_numpy(make_frames(h, w, n)).to(self.dev)
        return self._frames[h, w, n]

    def close(self):
        for nd in self._h.values():
            nd.close()


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_yolo"))
    yield m
    m.close()


def py_predict(det, frames, plan):
    pred = det.forward_letterboxed(det.preprocess(frames)[0], plan)
    return pred[0] if det.cfg.kpt_shape is not None else pred


def py_detect(det, frames, plan, conf=0.25, max_det=300, iou=0.7):
    fn = det.detect_pose if det.cfg.kpt_shape is not None else det.detect
    return tuple(fn(frames, conf=conf, iou=iou, max_det=max_det, precision=plan))


def _assert_same(got, want, what=""):
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, ("boxes", "scores", "cls", "src", "counts", "kpts")):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{what} {name}"


def test_the_l_model_reaches_split_k(models):
    """yolov8l at imgsz 320 has exact-plan 3 x 3 convolutions that are split over k: asserted from lmx_h_conv_split_k over its layers"""
    from lmx import native

    det, _ = models.model("l")
    factors = set()
    px = {1: 80 * 80, 3: 40 * 40, 5: 20 * 20, 7: 10 * 10, 16: 20 * 20, 19: 10 * 10}
    for i, p in px.items():
        m = det.table[i]
        factors.add(native.conv_split_k(p, m["c2"], 27 * m["c1"], 3 * m["c1"]))
    for i, hw in ((2, 80), (4, 40), (6, 20), (8, 10), (12, 20), (15, 40), (18, 20), (21, 10)):
        c = det.table[i]["c2"] // 2
        factors.add(native.conv_split_k(hw * hw, c, 27 * c, 3 * c))
    assert max(factors) >= 2, factors


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", MODELS)
def test_predict_equals_python_plan(models, name, plan, size):
    det, _ = models.model(name)
    h, w = SIZES[size]
    frames = models.frames(h, w)
    want = py_predict(det, frames, plan)
    ny = models.handle(name)
    got = ny.predict(frames, plan)
    oh, ow, A = ny.anchors(h, w)
    geo = det.preprocess(frames)[1]
    assert (oh, ow) == (geo.oh, geo.ow) and tuple(got.shape) == (2, A, 4 + det.cfg.nc) == tuple(want.shape)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max())}"


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", MODELS)
def test_detect_equals_python_plan(models, name, plan, size):
    det, _ = models.model(name)
    h, w = SIZES[size]
    frames = models.frames(h, w)
    ny = models.handle(name)
    partial = False  # some frame keeps >= 1 and < max_det detections
    for max_det in (300, 7):
        for conf, iou in OTHER[name] + [LOW[name]]:
            want = py_detect(det, frames, plan, conf, max_det, iou)
            counts = want[4]
            print(f"{name} {plan} {size} conf {conf} iou {iou} max_det {max_det}: counts {counts.tolist()}")
            if (conf, iou) == LOW[name]:
                assert int(counts.max()) == max_det, f"conf {conf} iou {iou} does not fill max_det {max_det}: counts {counts.tolist()}"
            partial = partial or bool(((counts >= 1) & (counts < max_det)).any())
            got = ny.detect(frames, plan, conf=conf, iou=iou, max_det=max_det)
            _assert_same(got, want, f"conf {conf} iou {iou} max_det {max_det}")
            assert bool((got[3][got[3] < 0] == -1).all()) and int((got[3] >= 0).sum()) == int(counts.sum())
    assert partial, "no frame keeps between 1 and max_det - 1 detections at any (conf, max_det) of this case"
    info = ny.info
    k, ndim = det.cfg.kpt_shape or (0, 0)
    assert (chr(info.scale), info.nc, info.imgsz, info.kpt_k, info.kpt_ndim, info.plans, info.max_batch) == (det.cfg.scale, det.cfg.nc, 320, k, ndim, 3, 4)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", ["n", "pose"])
def test_chunks(models, name, plan):
    """max_batch = 3: n = 1, 3, 4, 7 run in chunks of 3 with a ragged last one, and equal the Python plan run ON THE SAME CHUNKS and
    concatenated.  (Equality with the Python plan on the whole batch is not claimed: the launcher picks some kernels from M, and batch
    invariance of the exact plan is not established for every shape.)"""
    det, _ = models.model(name)
    ny = models.handle(name, 3)
    frames = models.frames(481, 270, 7)
    for n in (1, 3, 4, 7):
        sub = frames[:n].contiguous()
        chunks = [sub[i:i + 3].contiguous() for i in range(0, n, 3)]
        want_pred = torch.cat([py_predict(det, c, plan) for c in chunks], 0)
        assert torch.equal(ny.predict(sub, plan), want_pred), n
        want = tuple(torch.cat(ts, 0) for ts in zip(*(py_detect(det, c, plan, LOW[name][0], 20) for c in chunks)))
        _assert_same(ny.detect(sub, plan, conf=LOW[name][0], max_det=20), want, f"n = {n}")


def test_two_sizes_alternate_on_one_handle(models):
    det, _ = models.model("n")
    ny = models.handle("n")
    a, b = models.frames(180, 320), models.frames(481, 270)
    wa, wb = py_detect(det, a, "exact"), py_detect(det, b, "exact")
    ga1, gb, ga2 = ny.detect(a, "exact"), ny.detect(b, "exact"), ny.detect(a, "exact")
    _assert_same(ga1, wa)
    _assert_same(gb, wb)
    _assert_same(ga2, wa)


def test_two_plans_alternate_on_one_handle(models):
    det, _ = models.model("pose")
    ny = models.handle("pose")
    a = models.frames(1080, 1920)
    wf, wx = py_detect(det, a, "f16"), py_detect(det, a, "exact")
    g1, g2, g3 = ny.detect(a, "f16"), ny.detect(a, "exact"), ny.detect(a, "f16")
    _assert_same(g1, wf)
    _assert_same(g2, wx)
    _assert_same(g3, wf)
    assert not torch.equal(py_predict(det, a, "f16"), py_predict(det, a, "exact")), "the two plans give the same bits: nothing alternated"


def test_two_handles_are_independent(models, cuda):
    from lmx import native

    (d1, p1), (d2, p2) = models.model("n"), models.model("pose")
    frames = models.frames(180, 320)
    w1, w2 = py_detect(d1, frames, "f16"), py_detect(d2, frames, "f16")
    h1, h2 = native.NativeYolo(p1, 2, cuda), native.NativeYolo(p2, 2, cuda)
    try:
        _assert_same(h1.detect(frames, "f16"), w1)
        _assert_same(h2.detect(frames, "f16"), w2)
        _assert_same(h1.detect(frames, "f16"), w1)
        h1.close()
        with pytest.raises(native.LmxError, match="closed"):
            h1.detect(frames, "f16")
        _assert_same(h2.detect(frames, "f16"), w2)
    finally:
        h1.close()
        h2.close()


def test_detect_only_enqueues_on_the_callers_stream(models, cuda):
    """After lmx_yolo_prepare, detect on a side stream; a consumer on that stream reads the outputs before any host synchronisation."""
    det, _ = models.model("n")
    ny = models.handle("n")
    frames = models.frames(333, 517)
    want = py_detect(det, frames, "exact")
    wz = want[0] * 2.0 + want[1].unsqueeze(-1) + want[4].view(-1, 1, 1).float()
    ny.prepare(333, 517, "exact")
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        got = ny.detect(frames, "exact")
        z = got[0] * 2.0 + got[1].unsqueeze(-1) + got[4].view(-1, 1, 1).float()
    side.synchronize()
    assert torch.equal(z, wz)
    _assert_same(got, want)


@pytest.mark.parametrize("name", ["n", "pose"])
def test_host_entry_equals_device_entry(models, name):
    det, _ = models.model(name)
    ny = models.handle(name, 3)
    frames = models.frames(481, 270, 7)
    dev_out = ny.detect(frames, "f16", conf=LOW[name][0], max_det=20)
    host_out = ny.detect_host(frames.cpu().numpy(), "f16", conf=LOW[name][0], max_det=20)
    assert len(host_out) == len(dev_out) == (6 if name == "pose" else 5)
    for h, d in zip(host_out, dev_out):
        assert h.dtype == d.cpu().numpy().dtype and h.tobytes() == d.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", MODELS)
def test_class_names(models, name):
    det, _ = models.model(name)
    ny = models.handle(name)
    assert [ny.class_name(i) for i in range(det.cfg.nc)] == [det.names[i] for i in range(det.cfg.nc)]
    assert ny.class_name(-1) is None and ny.class_name(det.cfg.nc) is None


def test_errors_are_returned_not_faults(models, cuda):
    from lmx import native

    det, path = models.model("n")
    pdet, ppath = models.model("pose")
    ny, npose = models.handle("n"), models.handle("pose")
    lib = native._lib.load()
    err = lambda: lib.lmx_last_error().decode()
    one = models.frames(180, 320)
    with pytest.raises(native.LmxError, match="n = 0"):
        ny.detect(torch.empty((0, 180, 320, 3), dtype=torch.uint8, device=cuda), "f16")
    out = [torch.empty((2, 300, 4), dtype=torch.float32, device=cuda), torch.empty((2, 300), dtype=torch.float32, device=cuda),
           torch.empty((2, 300), dtype=torch.int32, device=cuda), torch.empty((2, 300), dtype=torch.int32, device=cuda),
           torch.empty((2,), dtype=torch.int32, device=cuda)]
    ptr = [t.data_ptr() for t in out]
    kp = torch.empty((2, 300, 17, 3), dtype=torch.float32, device=cuda)
    args = (0.25, 0.7, 300)
    assert lib.lmx_yolo_detect(ny._h, one.data_ptr(), -1, 180, 320, 0, *args, *ptr, None, None) == -1 and "n = -1" in err()
    assert lib.lmx_yolo_detect(ny._h, None, 2, 180, 320, 0, *args, *ptr, None, None) == -1 and "null" in err()
    for i in range(5):  # each output in turn
        p = list(ptr)
        p[i] = None
        assert lib.lmx_yolo_detect(ny._h, one.data_ptr(), 2, 180, 320, 0, *args, *p, None, None) == -1 and "null" in err()
    assert lib.lmx_yolo_predict(ny._h, one.data_ptr(), 2, 180, 320, 0, None, None) == -1 and "null" in err()
    # kpts given for a detection image, missing for a pose image
    assert lib.lmx_yolo_detect(ny._h, one.data_ptr(), 2, 180, 320, 0, *args, *ptr, kp.data_ptr(), None) == -1 and "kpts must be NULL" in err()
    assert lib.lmx_yolo_detect(npose._h, one.data_ptr(), 2, 180, 320, 0, *args, *ptr, None, None) == -1 and "kpts must be given" in err()
    for md in (0, -5):
        with pytest.raises(native.LmxError, match="max_det"):
            ny.detect(one, "f16", max_det=md)
    assert lib.lmx_yolo_detect(ny._h, one.data_ptr(), 2, 180, 320, 2, *args, *ptr, None, None) == -1 and "precision 2" in err()
    # a plan absent from an f16-only image
    f16_only = models.tmp / "n_f16.lmx"
    native.write_yolo_image(det, f16_only, ("f16",))
    with native.NativeYolo(f16_only, 2, cuda) as h2:
        assert h2.info.plans == 1
        with pytest.raises(native.LmxError, match="does not hold the exact plan"):
            h2.prepare(180, 320, "exact")
        with pytest.raises(native.LmxError, match="does not hold the exact plan"):
            h2.detect(one, "exact")
        _assert_same(h2.detect(one, "f16"), py_detect(det, one, "f16"))
    for mb in (0, -3):
        with pytest.raises(native.LmxError, match="max_batch"):
            native.NativeYolo(path, mb, cuda)
    with pytest.raises(native.LmxError, match="cannot open"):
        native.NativeYolo(str(path) + ".absent", 2, cuda)
    # a workspace beyond what lmx_k_gemm's index arithmetic accepts: refused at prepare, with the buffer named, before anything is allocated
    with native.NativeYolo(path, 65535, cuda) as big:
        with pytest.raises(native.LmxError, match="buffer '.*the GEMM kernels index below 2 GB"):
            big.prepare(180, 320, "f16")
    # the handles that saw the errors still give the right answer
    _assert_same(ny.detect(one, "f16"), py_detect(det, one, "f16"))
    _assert_same(npose.detect(one, "exact"), py_detect(pdet, one, "exact"))


def test_a_handle_keeps_16_prepared_pairs(models, cuda):
    """16 (frame size, plan) pairs are kept, the 17th is refused by prepare and by detect alike, a pair already held still serves"""
    from lmx import native

    det, path = models.model("n")
    with native.NativeYolo(path, 1, cuda) as h:
        for i in range(16):
            h.prepare(33 + i, 40, "f16")
        with pytest.raises(native.LmxError, match="already holds 16"):
            h.prepare(33 + 16, 40, "f16")
        with pytest.raises(native.LmxError, match="already holds 16"):
            h.prepare(33, 40, "exact")  # a held size under the other plan is another pair
        one = models.frames(180, 320, 1)
        with pytest.raises(native.LmxError, match="already holds 16"):
            h.detect(one, "f16")
        small = models.frames(33, 40, 1)
        _assert_same(h.detect(small, "f16"), py_detect(det, small, "f16"))


def test_c_example_gives_the_python_detections(models, tmp_path):
    """examples/yolo_detect.c, compiled with cc against liblmx.so and run as a child process on the exported image: its output file
    holds the Python plan's bytes (exact plan, conf 0.25, max_det 300, chunks of 3).  The child's loader is pointed at the HIP runtime
    this process loaded."""
    from lmx import _lib

    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    det, path = models.model("n")
    frames = models.frames(180, 320, 4)
    want = [torch.cat(ts, 0).cpu().numpy() for ts in zip(*(py_detect(det, frames[i:i + 3].contiguous(), "exact") for i in (0, 3)))]
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(np.array([4, 180, 320], np.int32).tobytes())
        f.write(frames.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "yolo_detect"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "yolo_detect.c"),
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
    out = tmp_path / "det.bin"
    r = subprocess.run([str(exe), str(path), str(raw), str(out), "3"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    boxes, scores, cls, src, counts = want
    assert out.read_bytes() == counts.tobytes() + boxes.tobytes() + scores.tobytes() + cls.tobytes()
