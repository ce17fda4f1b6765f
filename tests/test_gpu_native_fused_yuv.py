"""The fused per-frame path from decoder frames (csrc/fused_model.hip: lmx_fused_step_yuv, lmx_fused_step_yuv_host): the records EQUAL
(torch.equal) those of lmx_k_yuv420_to_bgr followed by lmx_fused_step — on both plans, dense and scheduled, with and without padding
rows, from a pitched NV12 surface and from tight I420 planes; the host form equals the device form on the same bytes; a handle that
has seen YUV steps on BGR as one that never did; and the BGR buffer exists only from the first _yuv call on.  Models, weight images
and helpers are those of tests/test_gpu_native_fused.py (YOLOv8-n at imgsz 320, Hiera (2,2,3,1), a 2-layer DINOv3, CHUNK = 2); frames
of 180 x 320 and 150 x 100 (13-byte mask_bits rows), n = 5 with max_frames = 7, made NV12 / I420 from make_frames through
yuvref.bgr_to_yuv (a fixed map: only determinism matters)."""
import numpy as np
import pytest
import torch

import yuvref
from test_gpu_native_fused import CHUNK, PLANS, _assert_records, _Models, _step
from test_gpu_native_yolo import make_frames

pytestmark = pytest.mark.gpu
N, MAX_FRAMES = 5, 7
SIZES = ((180, 320), (150, 100))
SOURCES = ("nv12_pitched", "i420_tight")


class _Yuv:
    """per frame size, built once: the YUV planes on the host, the device views of each source, the BGR frames lmx_k_yuv420_to_bgr makes
    of them, and per plan a confidence threshold that splits the frames"""

    def __init__(self, models):
        self.m, self._planes, self._dev, self._bgr, self._conf = models, {}, {}, {}, {}

    def planes(self, h, w):
        if (h, w) not in self._planes:
            self._planes[h, w] = yuvref.bgr_to_yuv(make_frames(h, w, N))
        return self._planes[h, w]

    def device(self, h, w, source):
        """kwargs of K.yuv420_to_bgr / NativeFused.step_yuv: y, c, h, w, layout, matrix, v"""
        if (h, w, source) not in self._dev:
            dev = self.m.dev
            y, u, v = self.planes(h, w)
            if source == "nv12_pitched":  # a surface pitched to 256 bytes, the chroma plane in an allocation of its own, 3 spare rows per frame
                pitch = -(-w // 256) * 256
                dy = torch.zeros((N, h + 3, pitch), dtype=torch.uint8, device=dev)
                dc = torch.zeros((N, h // 2 + 3, pitch), dtype=torch.uint8, device=dev)
                dy[:, :h, :w] = torch.from_numpy(y).to(dev)
                dc[:, : h // 2, :w] = torch.from_numpy(yuvref.interleave(u, v)).to(dev)
                self._dev[h, w, source] = dict(y=dy[:, :h, :w], c=dc[:, : h // 2, :w], h=h, w=w, layout="nv12", matrix="bt601", v=None)
            else:
                t = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in (y, u, v)]
                self._dev[h, w, source] = dict(y=t[0], c=t[1], h=h, w=w, layout="i420", matrix="bt709", v=t[2])
        return self._dev[h, w, source]

    def bgr(self, h, w, source):
        from lmx import kernels as K

        if (h, w, source) not in self._bgr:
            self._bgr[h, w, source] = K.yuv420_to_bgr(**self.device(h, w, source))
            torch.cuda.synchronize(self.m.dev)
        return self._bgr[h, w, source]

    def conf(self, plan, h, w, source):
        """between two frames' top scores, where they lie furthest apart: some frames keep a detection, some have none"""
        key = (plan, h, w, source)
        if key not in self._conf:
            scores = self.m.det.detect(self.bgr(h, w, source), conf=0.001, precision=plan)[1]
            top = sorted(float(s) for s in scores[:, 0].cpu())
            gap, i = max((top[i + 1] - top[i], i) for i in range(len(top) - 1))
            assert gap > 1e-4, f"the frames' top scores {top} leave no threshold between them"
            self._conf[key] = (top[i] + top[i + 1]) / 2
        return self._conf[key]


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_fused_yuv"))
    yield m
    m.close()


@pytest.fixture(scope="module")
def yuv(models):
    return _Yuv(models)


def _step_yuv(ns, src, plan, conf, **kw):
    """one step from YUV, finished: ONE step in flight per handle"""
    got, layout = ns.step_yuv(src["y"], src["c"], src["h"], src["w"], plan, layout=src["layout"], matrix=src["matrix"], v=src["v"], conf=conf, **kw)
    torch.cuda.synchronize(src["y"].device)
    return got, layout


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_step_yuv_equals_convert_then_step(models, yuv, size, plan):
    """dense and scheduled (det_idx = [0, 2, 4], emb_idx = [0, 3]), n_rows = n and n_rows = 8, NV12 pitched and I420 tight"""
    h, w = size
    ns = models.handle(MAX_FRAMES, 2)
    for source in SOURCES:
        src, bgr, conf = yuv.device(h, w, source), yuv.bgr(h, w, source), yuv.conf(plan, h, w, source)
        for sched in (None, ([0, 2, 4], [0, 3])):
            if sched:
                ns.schedule(N, *sched)
            try:
                for n_rows in (N, 8):
                    want, want_layout = _step(ns, bgr, plan, conf, n_rows=n_rows)
                    got, layout = _step_yuv(ns, src, plan, conf, n_rows=n_rows)
                    what = f"{source} {'scheduled' if sched else 'dense'} n_rows = {n_rows}"
                    _assert_records(got, layout, want, want_layout, what)
                    assert got[:, 0].tolist() == [1] * N + [0] * (n_rows - N), what
                    if sched:
                        assert [f[0] for f in layout][-3:] == ["ran_det", "ran_emb", "scores"]
                    else:
                        counts = [int(c) for c in _counts(got, layout)]
                        assert any(c > 0 for c in counts[:N]) and any(c == 0 for c in counts[:N]), f"conf must split the frames: counts {counts}"
            finally:
                if sched:
                    ns.schedule(N)
    if w == 100:
        assert dict((f[0], f[4]) for f in layout)["mask_bits"] == 150 * 13


def _counts(records, layout):
    from lmx import dist

    return dist.unpack_records(records, layout, keep_valid_only=False)["counts"].cpu().tolist()


@pytest.mark.parametrize("layout_name", ["nv12", "i420"])
def test_step_yuv_host_equals_step_yuv(models, yuv, layout_name):
    """the tightly packed rawvideo blob [n][h * 3 / 2][w] through lmx_fused_step_yuv_host, and the same bytes as device planes through
    lmx_fused_step_yuv"""
    h, w = 150, 100
    dev = models.dev
    y, u, v = yuv.planes(h, w)
    chroma = yuvref.interleave(u, v).reshape(N, -1) if layout_name == "nv12" else np.concatenate([u.reshape(N, -1), v.reshape(N, -1)], axis=1)
    blob = np.ascontiguousarray(np.concatenate([y.reshape(N, -1), chroma], axis=1).reshape(N, h * 3 // 2, w))
    d = torch.from_numpy(blob).to(dev)
    luma = h * w
    flat = d.view(N, -1)
    if layout_name == "nv12":
        src = dict(y=flat[:, :luma].unflatten(1, (h, w)), c=flat[:, luma:].unflatten(1, (h // 2, w)), h=h, w=w, layout="nv12", matrix="bt709", v=None)
    else:
        q = luma // 4
        src = dict(y=flat[:, :luma].unflatten(1, (h, w)), c=flat[:, luma:luma + q].unflatten(1, (h // 2, w // 2)), h=h, w=w, layout="i420", matrix="bt709",
                   v=flat[:, luma + q:].unflatten(1, (h // 2, w // 2)))
    ns = models.handle(MAX_FRAMES, 2)
    for plan in PLANS:
        conf = yuv.conf(plan, h, w, "i420_tight")
        dev_out, layout = _step_yuv(ns, src, plan, conf, n_rows=N + 1)
        host_out, host_layout = ns.step_yuv_host(blob, plan, layout=layout_name, matrix="bt709", conf=conf, n_rows=N + 1)
        assert host_layout == layout and host_out.dtype == np.uint8 and np.array_equal(host_out, dev_out.cpu().numpy()), plan
    host_out, _ = ns.step_yuv_host(blob[:0], "f16", layout=layout_name, n_rows=2)
    assert host_out.shape[0] == 2 and not host_out.any()


def test_bgr_steps_around_a_yuv_step_equal_a_handle_that_never_saw_yuv(models, yuv):
    h, w, plan = 180, 320, "f16"
    frames, conf = models.frames(h, w, N), models.conf(plan, h, w, N)
    never = models.handle(MAX_FRAMES, 3)  # no test of this module sends it YUV
    want, want_layout = _step(never, frames, plan, conf)
    ns = models.handle(MAX_FRAMES, 2)
    before, layout = _step(ns, frames, plan, conf)
    _assert_records(before, layout, want, want_layout, "BGR before YUV")
    _step_yuv(ns, yuv.device(h, w, "nv12_pitched"), plan, conf)
    _step_yuv(ns, yuv.device(150, 100, "i420_tight"), plan, conf)  # another size: the buffer is replaced
    after, layout = _step(ns, frames, plan, conf)
    _assert_records(after, layout, want, want_layout, "BGR after YUV")
    _assert_records(after, layout, *models.ref(plan, h, w, N)[:2], "BGR after YUV against the Python path")


def test_refusals(models, yuv):
    from lmx import native

    h, w, plan = 180, 320, "f16"
    ns = models.handle(MAX_FRAMES, 2)
    src = yuv.device(h, w, "i420_tight")
    with pytest.raises(native.LmxError, match="even sizes"):
        ns.step_yuv(src["y"], src["c"], h - 1, w, plan, layout="i420", v=src["v"])
    with pytest.raises(native.LmxError, match="n_rows = 2 is below n = 5"):
        ns.step_yuv(src["y"], src["c"], h, w, plan, layout="i420", v=src["v"], n_rows=2)
    with pytest.raises(native.LmxError, match="layout 'nv21'"):
        ns.step_yuv_host(np.zeros((1, 3, 2), np.uint8), plan, layout="nv21")
    lib = ns._lib
    blob = np.zeros((1, h * 3 // 2, w), np.uint8)
    rec = np.zeros((1, ns.layout(h, w)[1]), np.uint8)
    with torch.cuda.device(models.dev):
        assert lib.lmx_fused_step_yuv_host(ns._h, blob.ctypes.data, 2, 0, 1, h, w, 0, 0.5, rec.ctypes.data, 1) == -1
        assert "layout 2" in lib.lmx_last_error().decode()
        assert lib.lmx_fused_step_yuv_host(ns._h, blob.ctypes.data, 0, 3, 1, h, w, 0, 0.5, rec.ctypes.data, 1) == -1
        assert "matrix 3" in lib.lmx_last_error().decode()
    got, layout = _step_yuv(ns, src, plan, yuv.conf(plan, h, w, "i420_tight"))  # the handle still steps
    want, want_layout = _step(ns, yuv.bgr(h, w, "i420_tight"), plan, yuv.conf(plan, h, w, "i420_tight"))
    _assert_records(got, layout, want, want_layout, "after the refusals")


def test_the_bgr_buffer_appears_with_the_first_yuv_call_only(models, yuv, cuda):
    """a BGR-only prepare and step hold what they held before the _yuv entry points existed: lmx_fused_prepare and lmx_fused_step do
    not allocate the converted-frame buffer; the first lmx_fused_step_yuv does (max_frames frames of the size), the second nothing"""
    from lmx import native

    h, w, plan, max_frames = 180, 320, "f16", 24
    buffer_bytes = max_frames * h * w * 3  # 4.1 MB: well above the allocator's granule
    frames, conf = models.frames(h, w, N), models.conf(plan, h, w, N)
    src = yuv.device(h, w, "nv12_pitched")
    fresh = native.NativeFused(*models.paths, max_frames, CHUNK, sam_lanes=1, device=cuda)
    try:
        fresh.prepare(h, w, plan)
        want, layout = _step(fresh, frames, plan, conf)
        _step(fresh, frames, plan, conf)  # its records are dropped at once: torch's allocator now keeps a spare block of the records' size: later steps take it again
        with torch.cuda.device(cuda):
            free_prepared = torch.cuda.mem_get_info(cuda)[0]
            got = _step(fresh, frames, plan, conf)[0]
            assert torch.equal(got, want)
            del got
            free_bgr = torch.cuda.mem_get_info(cuda)[0]
            _step_yuv(fresh, src, plan, conf)
            free_yuv = torch.cuda.mem_get_info(cuda)[0]
            _step_yuv(fresh, src, plan, conf)
            free_yuv2 = torch.cuda.mem_get_info(cuda)[0]
        assert free_bgr >= free_prepared, "a BGR step on a prepared handle allocated device memory"
        assert free_bgr - free_yuv >= buffer_bytes, (free_bgr, free_yuv, buffer_bytes)
        assert free_yuv2 >= free_yuv, "the second _yuv step allocated again"
        again, layout2 = _step(fresh, frames, plan, conf)
        assert layout2 == layout and torch.equal(again, want)
    finally:
        fresh.close()
