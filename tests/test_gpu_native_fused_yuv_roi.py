"""The fused per-frame path on a crop window of decoder frames (csrc/fused_model.hip: lmx_fused_step_yuv_roi): the records EQUAL
(torch.equal) those of lmx_k_yuv420_to_bgr_roi followed by lmx_fused_step at the window's size, on both plans — for a window of odd
position and odd sizes, for the full-frame window (which also equals lmx_fused_step_yuv), and across calls that bring another window
size, so that the handle's BGR buffer is replaced and still serves.  Models, weight images and helpers are those of
tests/test_gpu_native_fused.py and tests/test_gpu_native_fused_yuv.py; frames of 180 x 320, n = 5 with max_frames = 7."""
import pytest
import torch

from test_gpu_native_fused import PLANS, _assert_records, _Models, _step
from test_gpu_native_fused_yuv import MAX_FRAMES, N, _step_yuv, _Yuv

pytestmark = pytest.mark.gpu
H, W = 180, 320
ODD = (33, 21, 201, 131)  # x, y, w, h: every one of them odd
OTHER = (64, 10, 128, 96)


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_fused_yuv_roi"))
    yield m
    m.close()


@pytest.fixture(scope="module")
def yuv(models):
    return _Yuv(models)


def _window(src, roi):
    """lmx_k_yuv420_to_bgr_roi on the planes of _Yuv.device"""
    from lmx import kernels as K

    bgr = K.yuv420_to_bgr_roi(src["y"], src["c"], src["h"], src["w"], roi, layout=src["layout"], matrix=src["matrix"], v=src["v"])
    torch.cuda.synchronize(bgr.device)
    return bgr


def _conf(models, bgr, plan):
    """a threshold among the frames' top scores (where they lie furthest apart), so that detections, masks and embeddings are in play"""
    top = sorted(float(s) for s in models.det.detect(bgr, conf=0.001, precision=plan)[1][:, 0].cpu())
    gap, i = max((top[i + 1] - top[i], i) for i in range(len(top) - 1))
    return (top[i] + top[i + 1]) / 2 if gap > 1e-4 else 0.25


def _step_roi(ns, src, roi, plan, conf, **kw):
    got, layout = ns.step_yuv_roi(src["y"], src["c"], src["h"], src["w"], roi, plan, layout=src["layout"], matrix=src["matrix"], v=src["v"], conf=conf, **kw)
    torch.cuda.synchronize(src["y"].device)
    return got, layout


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("source", ["nv12_pitched", "i420_tight"])
def test_step_yuv_roi_equals_window_then_step(models, yuv, source, plan):
    """the odd window, then another window size (the buffer is replaced), then the odd window again: each equals convert-then-step"""
    ns = models.handle(MAX_FRAMES, 2)
    src = yuv.device(H, W, source)
    for roi in (ODD, OTHER, ODD):
        bgr = _window(src, roi)
        assert tuple(bgr.shape) == (N, roi[3], roi[2], 3)
        conf = _conf(models, bgr, plan)
        want, want_layout = _step(ns, bgr, plan, conf, n_rows=N + 1)
        got, layout = _step_roi(ns, src, roi, plan, conf, n_rows=N + 1)
        _assert_records(got, layout, want, want_layout, f"{source} roi {roi}")
        assert got[:, 0].tolist() == [1] * N + [0]


@pytest.mark.parametrize("plan", PLANS)
def test_the_full_frame_window_equals_step_yuv(models, yuv, plan):
    ns = models.handle(MAX_FRAMES, 2)
    src = yuv.device(H, W, "nv12_pitched")
    conf = yuv.conf(plan, H, W, "nv12_pitched")
    want, want_layout = _step_yuv(ns, src, plan, conf)
    got, layout = _step_roi(ns, src, (0, 0, W, H), plan, conf)
    _assert_records(got, layout, want, want_layout, "the full-frame window against lmx_fused_step_yuv")
    bgr = _window(src, (0, 0, W, H))
    assert torch.equal(bgr, yuv.bgr(H, W, "nv12_pitched"))
    _assert_records(got, layout, *_step(ns, bgr, plan, conf), "the full-frame window against window-then-step")


def test_refusals_leave_the_handle_working(models, yuv):
    from lmx import native

    ns = models.handle(MAX_FRAMES, 2)
    src = yuv.device(H, W, "i420_tight")
    kw = dict(layout="i420", v=src["v"])
    with pytest.raises(native.LmxError, match="is outside the 180 x 320 frame"):
        ns.step_yuv_roi(src["y"], src["c"], H, W, (300, 0, 21, 20), "f16", **kw)
    with pytest.raises(native.LmxError, match="roi is empty"):
        ns.step_yuv_roi(src["y"], src["c"], H, W, (0, 0, 0, 20), "f16", **kw)
    with pytest.raises(native.LmxError, match="even sizes"):
        ns.step_yuv_roi(src["y"], src["c"], H - 1, W, (0, 0, 20, 20), "f16", **kw)
    with pytest.raises(native.LmxError, match="n_rows = 2 is below n = 5"):
        ns.step_yuv_roi(src["y"], src["c"], H, W, OTHER, "f16", n_rows=2, **kw)
    bgr = _window(src, OTHER)
    conf = _conf(models, bgr, "f16")
    _assert_records(*_step_roi(ns, src, OTHER, "f16", conf), *_step(ns, bgr, "f16", conf), "after the refusals")
