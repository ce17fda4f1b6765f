"""The model-level C API on the GPU (include/lmx.h "MODEL level", csrc/dino_model.hip): lmx_dino_embed is the launch sequence of
DinoEmbedder.embed_frames written in C++ — the same lmx_k_* entry points with the same descriptors — so the bar everywhere is
EQUALITY with the Python plan (torch.equal / equal bytes), which tests/test_gpu_dino*.py in turn hold to transformers' goldens.
Real widths at depth 2, synthetic weights, synthetic frames."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dinopre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _configs():
    from lmx import dino
    from lmx import resample as R

    rep = dataclasses.replace
    # DINOv3ViTImageProcessor's recipe as a model directory's preprocessor_config.json gives it (tests/dinopre.py, size 224, bilinear)
    pc = dinopre.dinov3_preprocessor_config(size=224)
    float_recipe = dino.DinoPreprocess(kind="float", filt={2: R.BILINEAR, 3: R.BICUBIC}[pc["resample"]], shortest_edge=None,
                                       size_hw=(pc["size"]["height"], pc["size"]["width"]), crop=None, rescale=pc["rescale_factor"],
                                       mean=tuple(pc["image_mean"]), std=tuple(pc["image_std"]))
    return {
        "dinov2_base": rep(dino.dinov2_base(), layers=2),                       # position table, Pillow recipe
        "dinov2_reg_base": dino.dinov2_reg_base(layers=2),                      # registers
        "dinov3_vitl16": rep(dino.dinov3_vitl16(), layers=2),                   # RoPE
        "dinov3_vitsplus16": dino.dinov3_vitsplus16(layers=2),                  # gated MLP
        "dinov3_float": dino.dinov3_vitsplus16(layers=2, preproc=float_recipe),  # float recipe
        "dinov3_nobias": dino.dinov3_vitsplus16(layers=2, q_bias=False, v_bias=False, proj_bias=False, mlp_bias=False),
        # Pillow recipe that squashes to a fixed size: the only one where ONE axis can keep its size (identity table / no vertical pass)
        "dinov2_squash": rep(dino.dinov2_base(), layers=2, preproc=dino.DinoPreprocess(shortest_edge=None, size_hw=(256, 256))),
        # bicubic float recipe with a centre crop: the tables are cut
        "dinov3_float_crop": dino.dinov3_vitsplus16(layers=2, preproc=rep(float_recipe, filt=R.BICUBIC, size_hw=(256, 320), crop=224)),
    }


class _Models:
    """Per configuration, built once: the Python embedder, its weight image and (per max_batch) an open handle."""

    def __init__(self, dev, tmp):
        self.dev, self.tmp, self.cfgs, self._m, self._h, self._frames = dev, tmp, _configs(), {}, {}, {}

    def model(self, name):
        from lmx import dino, native, weights

        if name not in self._m:
            cfg = self.cfgs[name]
            emb = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 40 + len(self._m)), self.dev)
            path = self.tmp / f"{name}.lmx"
            native.write_dino_image(emb, path)
            self._m[name] = (emb, path)
        return self._m[name]

    def handle(self, name, max_batch=4):
        from lmx import native

        if (name, max_batch) not in self._h:
            self._h[name, max_batch] = native.NativeDino(self.model(name)[1], max_batch, self.dev)
        return self._h[name, max_batch]

    def frames(self, h, w, n=2):
        """u8 [n,h,w,3] BGR on the device, deterministic in (h, w, n)."""
        from lmx import synth

        if (h, w, n) not in self._frames:
            self._frames[h, w, n] = torch.from_numpy(np.stack([synth.synth_frame(h + w, 3 * i, h, w) for i in range(n)], 0)).to(self.dev)
        return self._frames[h, w, n]

    def close(self):
        for nd in self._h.values():
            nd.close()


@pytest.fixture(scope="module")
def models(cuda, tmp_path_factory):
    m = _Models(cuda, tmp_path_factory.mktemp("native_dino"))
    yield m
    m.close()


def _sizes(recipe):
    """1080p, a width that is no multiple of 4, portrait, and frames whose width / height the recipe keeps."""
    if recipe.size_hw is not None:
        keep_w, keep_h = (300, recipe.size_hw[1]), (recipe.size_hw[0], 300)
    else:
        keep_w, keep_h = (300, recipe.shortest_edge), (recipe.shortest_edge, 300)
    return {"1080x1920": (1080, 1920), "270x481": (270, 481), "481x270": (481, 270), "keep_w": keep_w, "keep_h": keep_h}


@pytest.mark.parametrize("size", ["1080x1920", "270x481", "481x270", "keep_w", "keep_h"])
@pytest.mark.parametrize("name", ["dinov2_base", "dinov2_reg_base", "dinov3_vitl16", "dinov3_vitsplus16", "dinov3_float", "dinov3_nobias",
                                  "dinov2_squash", "dinov3_float_crop"])
def test_equals_python_plan(models, name, size):
    emb, _ = models.model(name)
    h, w = _sizes(emb.recipe)[size]
    if name == "dinov2_squash":  # the branches the configuration is here for
        nh, nw = emb.recipe.resized(h, w)
        assert (nw == w, nh == h) == {"keep_w": (True, False), "keep_h": (False, True)}.get(size, (False, False))
    frames = models.frames(h, w)
    want = emb.embed_frames(frames)
    nd = models.handle(name)
    got = nd.embed(frames)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, emb.cfg.hidden) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want), f"max abs difference {float((got - want).abs().max())}"
    # RGB input: the same frames with the channels already swapped
    assert torch.equal(nd.embed(frames.flip(-1).contiguous(), rgb=True), want)
    info = nd.info
    assert (info.hidden, info.heads, info.layers, info.tokens, info.max_batch) == (emb.cfg.hidden, emb.cfg.heads, 2, emb.cfg.tokens, 4)


@pytest.mark.parametrize("name", ["dinov2_base", "dinov3_float"])
def test_batches_beyond_max_batch(models, name):
    """max_batch = 3: n = 1, 3, 4, 7 run in chunks of 3 with a ragged last one and equal the Python plan on the whole batch."""
    emb, _ = models.model(name)
    nd = models.handle(name, 3)
    frames = models.frames(270, 481, 7)
    want7 = emb.embed_frames(frames)
    got7 = nd.embed(frames)
    assert torch.equal(got7, want7)
    for n in (1, 3, 4):
        sub = frames[:n].contiguous()
        got = nd.embed(sub)
        assert torch.equal(got, emb.embed_frames(sub)), n
        assert torch.equal(got, want7[:n]), n
    assert torch.equal(nd.embed(frames[:1].contiguous())[0], got7[0]), "frame 0 alone differs from frame 0 inside the 7"


@pytest.mark.parametrize("name", ["dinov2_base", "dinov3_float"])
def test_a_call_leaves_nothing_behind_for_the_next(models, cuda, name):
    """n = 3, then 1, then 3 frames on ONE handle with max_batch = 3 (Pillow recipe and float recipe).  A call's buffers lie where its
    own walk of the plan puts them, so the smaller call lays them over what the larger one left and the larger one over that again:
    each result equals, bit for bit, that of a fresh handle given the same call alone."""
    from lmx import native

    _, path = models.model(name)
    frames = models.frames(270, 481, 3)
    with native.NativeDino(path, 3, cuda) as nd:
        for n in (3, 1, 3):
            sub = frames[:n].contiguous()
            got = nd.embed(sub)
            with native.NativeDino(path, 3, cuda) as fresh:
                want = fresh.embed(sub)
            assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
            assert torch.equal(got, want), f"n = {n}: max abs difference {float((got - want).abs().max())}"


def test_two_sizes_alternate_on_one_handle(models):
    emb, _ = models.model("dinov3_vitsplus16")
    nd = models.handle("dinov3_vitsplus16")
    a, b = models.frames(270, 481), models.frames(481, 270)
    wa, wb = emb.embed_frames(a), emb.embed_frames(b)
    ga1, gb, ga2 = nd.embed(a), nd.embed(b), nd.embed(a)
    assert torch.equal(ga1, wa) and torch.equal(gb, wb) and torch.equal(ga2, wa)


def test_two_handles_are_independent(models, cuda):
    from lmx import native

    (e1, p1), (e2, p2) = models.model("dinov2_base"), models.model("dinov3_float")
    frames = models.frames(270, 481)
    w1, w2 = e1.embed_frames(frames), e2.embed_frames(frames)
    h1, h2 = native.NativeDino(p1, 2, cuda), native.NativeDino(p2, 2, cuda)
    try:
        assert torch.equal(h1.embed(frames), w1) and torch.equal(h2.embed(frames), w2) and torch.equal(h1.embed(frames), w1)
        h1.close()
        with pytest.raises(native.LmxError, match="closed"):
            h1.embed(frames)
        assert torch.equal(h2.embed(frames), w2)
    finally:
        h1.close()
        h2.close()


def test_embed_only_enqueues_on_the_callers_stream(models, cuda):
    """After lmx_dino_prepare, embed on a side stream; a consumer on that stream reads `emb` before any host synchronisation."""
    emb, _ = models.model("dinov2_reg_base")
    nd = models.handle("dinov2_reg_base")
    frames = models.frames(333, 517)
    want = emb.embed_frames(frames) * 2.0 + 1.0
    nd.prepare(333, 517)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        got = nd.embed(frames)
        z = got * 2.0 + 1.0
    side.synchronize()
    assert torch.equal(z, want)


def test_host_entry_equals_device_entry(models):
    emb, _ = models.model("dinov3_vitsplus16")
    nd = models.handle("dinov3_vitsplus16", 3)
    frames = models.frames(270, 481, 7)
    dev_out = nd.embed(frames).cpu().numpy()
    host_out = nd.embed_host(frames.cpu().numpy())
    assert host_out.dtype == np.float32 and host_out.tobytes() == dev_out.tobytes()
    assert host_out.tobytes() == emb.embed_frames(frames).cpu().numpy().tobytes()


def test_errors_are_returned_not_faults(models, cuda):
    from lmx import dino, native, weights

    emb, path = models.model("dinov2_base")
    nd = models.handle("dinov2_base")
    with pytest.raises(native.LmxError, match="n = 0"):
        nd.embed(torch.empty((0, 270, 481, 3), dtype=torch.uint8, device=cuda))
    lib = native._lib.load()
    one = models.frames(270, 481)
    out = torch.empty((2, emb.cfg.hidden), dtype=torch.float32, device=cuda)
    assert lib.lmx_dino_embed(nd._h, one.data_ptr(), -1, 270, 481, 0, out.data_ptr(), None) == -1 and b"n = -1" in lib.lmx_last_error()
    assert lib.lmx_dino_embed(nd._h, None, 2, 270, 481, 0, out.data_ptr(), None) == -1 and b"null" in lib.lmx_last_error()
    with pytest.raises(native.LmxError, match="max_batch"):
        native.NativeDino(path, 0, cuda)
    with pytest.raises(native.LmxError, match="max_batch"):
        native.NativeDino(path, -3, cuda)
    with pytest.raises(native.LmxError, match="cannot open"):
        native.NativeDino(str(path) + ".absent", 2, cuda)
    # a recipe that resizes below the crop: refused at prepare, before anything is allocated for the size
    small = dataclasses.replace(models.cfgs["dinov3_float_crop"], preproc=dataclasses.replace(models.cfgs["dinov3_float_crop"].preproc, size_hw=(192, 320)))
    e2 = dino.DinoEmbedder(small, weights.synth_state_dict(dino.param_spec(small), 2), cuda)
    p2 = models.tmp / "small.lmx"
    native.write_dino_image(e2, p2)
    with native.NativeDino(p2, 2, cuda) as h2:
        with pytest.raises(native.LmxError, match="smaller than the 224 crop"):
            h2.prepare(540, 960)
        with pytest.raises(native.LmxError, match="smaller than the 224 crop"):
            h2.embed(models.frames(270, 481))
    # the handle that saw the errors still works
    assert torch.equal(nd.embed(one), emb.embed_frames(one))


def test_c_example_gives_the_python_embeddings(models, tmp_path):
    """examples/dino_embed.c, compiled with cc against liblmx.so and run as a child process on the exported image: its output file
    holds the Python embedder's bytes.  The child's loader is pointed at the HIP runtime this process loaded."""
    from lmx import _lib

    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    emb, path = models.model("dinov2_base")
    frames = models.frames(270, 481, 4)
    want = emb.embed_frames(frames).cpu().numpy()
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(np.array([4, 270, 481], np.int32).tobytes())
        f.write(frames.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "dino_embed"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "dino_embed.c"),
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
    out = tmp_path / "emb.f32"
    r = subprocess.run([str(exe), str(path), str(raw), str(out), "3"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == want.tobytes()
