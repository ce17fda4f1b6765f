"""The fused per-frame path behind the C API (csrc/fused_model.hip): lmx_fused_step is the launch sequence of FusedExtractor.step on
internal streams — YOLO, DINO and the SAM passes on workspace lanes of one weight upload — ending in lmx_k_pack_records.  The bar
everywhere is EQUALITY (torch.equal / np.array_equal) with the Python path: the reference of every test is
lmx.dist.pack_records(FusedExtractor.from_models(detector, HieraEncoder(band="blocks"), decoder, embedder).step(...)), computed once per
case and left unchanged.  Small models: YOLOv8-n at imgsz 320, Hiera R8 (tests/test_gpu_native_sam_hiera.py), a 2-layer DINOv3;
frames of 180 x 320 and 90 x 160, and 150 x 100 whose mask_bits rows are 13 bytes."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_native_yolo import make_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = ("f16", "exact")
CHUNK = 2


class _Models:
    """Built once: the three Python models, their weight images, the Python FusedExtractor over them (and one that keeps a single
    stream), open handles per (max_frames, sam_lanes), frames per (h, w, n), and the reference records per case."""

    def __init__(self, dev, tmp):
        from lmx import dino, native, pipeline, sam, sam_decoder, weights, yolo

        self.dev, self.tmp, self._h, self._frames, self._ref, self._conf = dev, tmp, {}, {}, {}, {}
        ycfg = yolo.YoloConfig("n", nc=80, imgsz=320)
        self.det = yolo.YoloDetector(ycfg, yolo.synthetic_state_dict(ycfg, 7, yolo.bn_stats_path("n")), dev)
        scfg = sam.HieraConfig(blocks=(2, 2, 3, 1), global_blocks=(6,))
        self.enc = sam.HieraEncoder(scfg, weights.synth_state_dict(sam.param_spec(scfg), 5), dev, band="blocks")
        self.dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), dev)
        dcfg = dataclasses.replace(dino.dinov3_vitl16(), layers=2)
        self.emb = dino.DinoEmbedder(dcfg, weights.synth_state_dict(dino.param_spec(dcfg), 40), dev)
        self.paths = (tmp / "yolo.lmx", tmp / "sam.lmx", tmp / "dino.lmx")
        native.write_yolo_image(self.det, self.paths[0])
        native.write_sam_image(self.enc, self.dec, self.paths[1], PLANS)
        native.write_dino_image(self.emb, self.paths[2])
        self.fx = pipeline.FusedExtractor.from_models(self.det, self.enc, self.dec, self.emb)
        self.fx.serial = False
        self.fx_serial = pipeline.FusedExtractor.from_models(self.det, self.enc, self.dec, self.emb)
        self.fx_serial.serial = True  # LMX_SERIAL: every launch on the caller's stream

    def handle(self, max_frames=7, sam_lanes=2):
        from lmx import native

        key = (max_frames, sam_lanes)
        if key not in self._h:
            self._h[key] = native.NativeFused(*self.paths, max_frames, CHUNK, sam_lanes=sam_lanes, device=self.dev)
        return self._h[key]

    def frames(self, h, w, n):
        if (h, w, n) not in self._frames:
            self._frames[h, w, n] = torch.from_numpy(make_frames(h, w, n)).to(self.dev)
        return self._frames[h, w, n]

    def conf(self, plan, h, w, n):
        """a threshold between the per-frame top scores of the reference: at least one frame keeps a detection and at least one has none"""
        key = (plan, h, w, n)
        if key not in self._conf:
            scores = self.det.detect(self.frames(h, w, n), conf=0.001, precision=plan)[1]
            top = sorted(float(s) for s in scores[:, 0].cpu())
            gaps = [(top[i + 1] - top[i], i) for i in range(len(top) - 1)]
            gap, i = max(gaps)
            assert gap > 1e-4, f"the frames' top scores {top} leave no threshold between them"
            self._conf[key] = (top[i] + top[i + 1]) / 2
        return self._conf[key]

    def ref(self, plan, h, w, n, det_idx=None, emb_idx=None, n_rows=None, serial=False):
        """(records uint8 [n_rows, stride], layout, dict) of the Python path"""
        from lmx import dist

        key = (plan, h, w, n, None if det_idx is None else tuple(det_idx), None if emb_idx is None else tuple(emb_idx), n_rows, serial)
        if key not in self._ref:
            fx = self.fx_serial if serial else self.fx
            out = fx.step(self.frames(h, w, n), conf=self.conf(plan, h, w, n), sam_chunk=CHUNK, det_idx=det_idx, emb_idx=emb_idx, precision=plan)
            torch.cuda.synchronize(self.dev)
            out.pop("mask", None)
            buf, layout = dist.pack_records(out, n_rows)
            self._ref[key] = (buf, layout, out)
        return self._ref[key]

    def close(self):
        for h in self._h.values():
            h.close()


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_fused"))
    yield m
    m.close()


def _step(ns, frames, plan, conf, **kw):
    """one step, finished: ONE step in flight per handle"""
    got, layout = ns.step(frames, plan, conf=conf, **kw)
    torch.cuda.synchronize(frames.device)
    return got, layout


def _assert_records(got, layout, want, want_layout, what):
    from lmx import dist

    assert layout == want_layout, (what, layout, want_layout)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    if not torch.equal(got, want):
        g, r = dist.unpack_records(got, layout, keep_valid_only=False), dist.unpack_records(want, layout, keep_valid_only=False)
        diff = {k: int((g[k] != r[k]).sum()) for k in g if not torch.equal(g[k], r[k])}
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.numel()} bytes differ; elements per field: {diff}; "
                             f"valid words {got[:, 0].tolist()} / {want[:, 0].tolist()}")


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("case", ["n5_ragged_last_pass", "n7_lane_reused"])
def test_dense_step_equals_python(models, plan, case):
    """n = 5 in passes of 2 (the last pass holds one frame) on three lanes; n = 7 in passes of 2 on two lanes: passes 0 and 2 share a
    lane, passes 1 and 3 the other, so a lane is taken again while its neighbour is still busy"""
    (h, w), n, lanes = {"n5_ragged_last_pass": ((180, 320), 5, 3), "n7_lane_reused": ((90, 160), 7, 2)}[case]
    frames = models.frames(h, w, n)
    want, want_layout, out = models.ref(plan, h, w, n)
    counts = out["counts"].cpu().tolist()
    assert any(c > 0 for c in counts) and any(c == 0 for c in counts), f"conf must split the frames: counts {counts}"
    ns = models.handle(7, lanes)
    assert (ns.info.max_det, ns.info.hidden, ns.info.max_frames, ns.info.sam_chunk, ns.info.sam_lanes) == (300, models.emb.cfg.hidden, 7, CHUNK, lanes)
    assert (ns.info.yolo.imgsz, ns.info.sam.encoder, ns.info.dino.layers) == (320, 2, 2)
    got, layout = _step(ns, frames, plan, models.conf(plan, h, w, n))
    _assert_records(got, layout, want, want_layout, f"{case} {plan}")


def test_lanes_do_not_change_the_bytes(models):
    """sam_lanes = 1 == sam_lanes = 3 == the Python path on one stream (LMX_SERIAL) == the Python path on its stream pool"""
    h, w, n, plan = 150, 100, 5, "exact"
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    serial, serial_layout, _ = models.ref(plan, h, w, n, serial=True)
    pooled = models.ref(plan, h, w, n)[0]
    assert torch.equal(serial, pooled)
    for lanes in (1, 3):
        got, layout = _step(models.handle(7, lanes), frames, plan, conf)
        _assert_records(got, layout, serial, serial_layout, f"sam_lanes = {lanes}")
    assert dict((f[0], f[4]) for f in layout)["mask_bits"] == 150 * 13


def test_two_consecutive_steps_are_bit_equal(models):
    h, w, n, plan = 90, 160, 7, "f16"
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    ns = models.handle(7, 2)
    first, _ = _step(ns, frames, plan, conf)
    second, layout = _step(ns, frames, plan, conf)
    assert torch.equal(first, second)
    _assert_records(second, layout, *models.ref(plan, h, w, n)[:2], "second step")


def test_scheduled_step_equals_python_and_clearing_gives_the_dense_bytes(models):
    h, w, n, plan = 180, 320, 5, "exact"
    det_idx, emb_idx = [0, 3], [0, 4]
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    want, want_layout, out = models.ref(plan, h, w, n, det_idx=det_idx, emb_idx=emb_idx)
    assert out["ran_det"].tolist() == [1, 0, 0, 1, 0] and out["ran_emb"].tolist() == [1, 0, 0, 0, 1]
    ns = models.handle(7, 2)
    ns.schedule(n, det_idx, emb_idx)
    try:
        got, layout = _step(ns, frames, plan, conf)
        _assert_records(got, layout, want, want_layout, "scheduled")
        assert got[1, 0] == 1 and not bool(got[1, 8:].any()), "frame 1 ran nowhere: a zero row with valid = 1"
        assert [f[0] for f in layout][-3:] == ["ran_det", "ran_emb", "scores"]
        with pytest.raises(Exception, match="the schedule was set for 5"):
            ns.step(models.frames(h, w, 5)[:4].contiguous(), plan, conf=conf)
        with pytest.raises(Exception, match=r"det_idx\[1\] = 1 after det_idx\[0\] = 3"):
            ns.schedule(n, [3, 1], emb_idx)
        with pytest.raises(Exception, match=r"emb_idx\[0\] = 5 outside 0 .. 4"):
            ns.schedule(n, det_idx, [5])
        got, layout = _step(ns, frames, plan, conf)  # a refused schedule leaves the one before in place
        _assert_records(got, layout, want, want_layout, "scheduled, after refused schedules")
        only_det = models.ref(plan, h, w, n, det_idx=det_idx)
        ns.schedule(n, det_idx, None)  # emb_idx = None: DINO on every frame, read in place
        got, layout = _step(ns, frames, plan, conf)
        _assert_records(got, layout, *only_det[:2], "det_idx alone")
    finally:
        ns.schedule(n)
    got, layout = _step(ns, frames, plan, conf)
    _assert_records(got, layout, *models.ref(plan, h, w, n)[:2], "dense again")


def test_padding_rows_and_an_empty_step(models):
    h, w, n, plan = 150, 100, 5, "f16"
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    ns = models.handle(7, 2)
    want, want_layout, _ = models.ref(plan, h, w, n, n_rows=n + 3)
    got, layout = _step(ns, frames, plan, conf, n_rows=n + 3)
    _assert_records(got, layout, want, want_layout, "n_rows = n + 3")
    assert got[:, 0].tolist() == [1] * n + [0] * 3 and not bool(got[n:].any())
    stride = want.shape[1]
    for rows in (0, 4):
        got, layout = _step(ns, frames[:0], plan, conf, n_rows=rows)
        assert tuple(got.shape) == (rows, stride) and layout == want_layout and not bool(got.any())


def test_step_only_enqueues_on_the_callers_stream(models, cuda):
    """a prepared step returns while work queued ahead of it on the caller's stream is still running: it creates nothing and does
    not synchronise, and its internal streams start behind the caller's stream"""
    h, w, n, plan = 90, 160, 7, "exact"
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    want, want_layout, _ = models.ref(plan, h, w, n)
    ns = models.handle(7, 2)
    ns.prepare(h, w, plan)
    _step(ns, frames, plan, conf)  # every kernel's code object is on the device after this
    a = torch.randn((8192, 8192), device=cuda)
    c = torch.empty_like(a)
    staged = torch.empty_like(frames)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    ahead = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(24):  # some hundred milliseconds of f32 GEMM in front of the call
            torch.matmul(a, a, out=c)
        staged.copy_(frames)  # the frames are produced on the caller's stream, behind the GEMMs
        ahead.record(side)
        got, layout = ns.step(staged, plan, conf=conf)
        returned_early = not ahead.query()
    side.synchronize()
    torch.cuda.synchronize(cuda)
    assert returned_early, "lmx_fused_step returned only after the work queued ahead of it had finished: it synchronised"
    _assert_records(got, layout, want, want_layout, "a step behind queued work")


def test_step_host_equals_step(models):
    h, w, n = 90, 160, 5
    ns = models.handle(7, 2)
    for plan in PLANS:
        frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
        dev_out, layout = _step(ns, frames, plan, conf, n_rows=n + 1)
        host_out, host_layout = ns.step_host(frames.cpu().numpy(), plan, conf=conf, n_rows=n + 1)
        assert host_layout == layout and host_out.dtype == np.uint8 and np.array_equal(host_out, dev_out.cpu().numpy()), plan
        _assert_records(dev_out, layout, *models.ref(plan, h, w, n, n_rows=n + 1)[:2], f"step {plan}")


def test_refusals_allocate_nothing_and_the_handle_still_steps(models, cuda, tmp_path):
    from lmx import native

    h, w, n, plan = 90, 160, 5, "f16"
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    f16_only = tmp_path / "yolo_f16.lmx"
    native.write_yolo_image(models.det, f16_only, ("f16",))
    small = native.NativeFused(f16_only, models.paths[1], models.paths[2], 3, CHUNK, sam_lanes=1, device=cuda)
    three, conf3 = models.frames(h, w, 3), models.conf(plan, h, w, 3)
    lib, err = small._lib, lambda: small._lib.lmx_last_error().decode()
    rec = torch.empty((5, small.layout(h, w)[1]), dtype=torch.uint8, device=cuda)

    def raw(fr, n, precision, n_rows):
        return lib.lmx_fused_step(small._h, fr.data_ptr(), n, h, w, precision, conf, rec.data_ptr(), n_rows, None)

    try:
        with torch.cuda.device(cuda):
            free = torch.cuda.mem_get_info(cuda)[0]
            assert lib.lmx_fused_prepare(small._h, h, w, 1) == -1 and "yolo_image does not hold the exact plan" in err()
            assert lib.lmx_fused_prepare(small._h, h, w, 7) == -1 and "precision 7" in err()
            assert raw(three, 3, 1, 3) == -1 and "yolo_image does not hold the exact plan" in err()
            assert raw(frames, 5, 0, 5) == -1 and "n = 5 frames outside 0 .. max_frames = 3" in err()
            assert raw(three, 3, 0, 2) == -1 and "n_rows = 2 is below n = 3" in err()
            assert raw(three, -1, 0, 3) == -1 and "n = -1" in err()
            assert torch.cuda.mem_get_info(cuda)[0] >= free, "a refused call allocated device memory"
        with pytest.raises(native.LmxError, match="yolo_image does not hold the exact plan"):
            small.prepare(h, w, "exact")
        with pytest.raises(native.LmxError, match="n = 5 frames outside 0 .. max_frames = 3"):
            small.step(frames, plan, conf=conf)
        with pytest.raises(native.LmxError, match="n_rows = 2 is below n = 3"):
            small.step(three, plan, conf=conf3, n_rows=2)
        got, layout = _step(small, three, plan, conf3)
        _assert_records(got, layout, *models.ref(plan, h, w, 3)[:2], "after the refusals")
    finally:
        small.close()
    with pytest.raises(native.LmxError, match="the handle is closed"):
        small.step(three, plan, conf=conf3)
    with pytest.raises(native.LmxError, match="sam_lanes 0 outside"):
        native.NativeFused(*models.paths, 3, CHUNK, sam_lanes=0, device=cuda)
    with pytest.raises(native.LmxError, match="cannot open|No such file|missing"):
        native.NativeFused(*models.paths[:2], tmp_path / "absent.lmx", 3, CHUNK, device=cuda)


def test_a_stream_of_another_device_is_refused(models, cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no stream of another device")
    h, w, n, plan = 90, 160, 5, "f16"
    frames = models.frames(h, w, n)
    ns = models.handle(7, 2)
    lib = ns._lib
    other = torch.cuda.Stream(device=torch.device("cuda", 1))
    rec = torch.empty((n, ns.layout(h, w)[1]), dtype=torch.uint8, device=cuda)
    with torch.cuda.device(cuda):
        assert lib.lmx_fused_step(ns._h, frames.data_ptr(), n, h, w, 0, 0.5, rec.data_ptr(), n, other.cuda_stream) == -1
        assert "the stream belongs to device 1" in lib.lmx_last_error().decode()
    with torch.cuda.device(torch.device("cuda", 1)):
        assert lib.lmx_fused_step(ns._h, frames.data_ptr(), n, h, w, 0, 0.5, rec.data_ptr(), n, None) == -1
        assert "the current device is 1" in lib.lmx_last_error().decode()


def test_c_example_writes_the_python_records(models, tmp_path):
    """examples/fused_extract.c compiled with cc against liblmx.so and run as a child process: records.bin is the reference matrix"""
    from lmx import _lib

    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    h, w, n, plan = 90, 160, 5, "exact"  # the images hold both plans: the example takes the exact one
    frames, conf = models.frames(h, w, n), models.conf(plan, h, w, n)
    want = models.ref(plan, h, w, n)[0]
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(np.array([n, h, w], np.int32).tobytes())
        f.write(frames.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "fused_extract"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fused_extract.c"),
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
    out = tmp_path / "records.bin"
    r = subprocess.run([str(exe), *map(str, models.paths), str(raw), str(out), str(CHUNK), "2", repr(conf)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == want.cpu().numpy().tobytes()
