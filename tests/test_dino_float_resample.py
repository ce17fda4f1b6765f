"""lmx.resample.aa_tables (float32 antialias weights in ATen's arithmetic) + the numpy two-pass evaluation the device kernel
restates, against torch's F.interpolate(antialias=True) on CPU float32 — the resize of DINOv3ViTImageProcessor.  CPU only."""
import numpy as np
import pytest
import torch

from lmx import resample as R

# (in_h, in_w) -> (out_h, out_w): 1080p / 720p down to the network sizes, odd sizes, an upscale, mixed (one axis up, one down)
GEOMETRIES = [((1080, 1920), (224, 224)), ((720, 1280), (224, 224)), ((333, 517), (224, 224)), ((150, 200), (224, 224)),
              ((333, 517), (448, 448)), ((241, 163), (97, 301)), ((224, 300), (224, 224))]


def _torch_resize(img, oh, ow, filt):
    t = torch.from_numpy(img).permute(2, 0, 1)[None].contiguous()
    return torch.nn.functional.interpolate(t, size=(oh, ow), mode=filt, align_corners=False, antialias=True)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("filt", [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_two_pass_f32_matches_torch(geo, filt):
    """max abs difference <= 5e-7 on inputs in [0, 1] (about 4 ulp of 1.0: room for the summation order of a torch build
    without fused multiply-add).  Measured when this test was written, torch 2.10 CPU (an FMA build): 0.0 for every case
    here, bilinear and bicubic — bicubic needs no more than bilinear once the cubic polynomial is evaluated fused as well."""
    (h, w), (oh, ow) = geo
    rng = np.random.default_rng(h * 7 + ow)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.float32) * np.float32(1 / 255)
    got = R.resize_f32_reference(img, ow, oh, filt)
    ref = _torch_resize(img, oh, ow, filt)
    d = float(np.abs(got - ref).max())
    print(geo, filt, "max abs diff", d, "bit-equal fraction", float((got == ref).mean()))
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert d <= 5e-7, d


@pytest.mark.parametrize("filt", [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize("n_in,n_out", [(1920, 224), (1080, 448), (517, 224), (150, 224), (200, 448)])
def test_weights_are_torchs(n_in, n_out, filt):
    """An identity matrix resized along its width IS torch's weight table.  Tables: same layout as coeff_tables, every row
    sums to 1 within float32 rounding, taps stay inside the input, and each weight is within 1e-6 of torch's: the cubic's
    intermediates reach 4 (ulp 4.8e-7) and a torch build without fused multiply-add rounds twice more per term, so about 8 ulp
    of 1.0 is what separates two correct float32 evaluations.  Measured against torch 2.10 CPU (an FMA build): all equal."""
    b, k, ks = R.aa_tables(n_in, n_out, filt)
    assert b.dtype == np.int32 and k.dtype == np.float32 and b.shape == (2 * n_out,) and k.shape == (n_out * ks,)
    b, k = b.reshape(-1, 2), k.reshape(-1, ks)
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= ks).all()
    assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()  # what segment_cols and the kernel rely on
    assert np.abs(k.sum(1, dtype=np.float64) - 1).max() < 1e-6
    eye = torch.eye(n_in, dtype=torch.float32)[None, None]
    ref = torch.nn.functional.interpolate(eye, size=(n_in, n_out), mode=filt, align_corners=False, antialias=True)[0, 0].numpy()
    W = np.zeros((n_in, n_out), np.float32)
    for x in range(n_out):
        W[b[x, 0]:b[x, 0] + b[x, 1], x] = k[x, :b[x, 1]]
    d = float(np.abs(W - ref).max())
    print(n_in, n_out, filt, "ksize", ks, "max weight diff", d)
    assert d <= 1e-6, d


def test_segment_cols():
    b, _, _ = R.aa_tables(1920, 448, R.BILINEAR)
    bb = b.reshape(-1, 2)
    assert R.segment_cols(b) == max(bb[255, 0] + bb[255, 1] - bb[0, 0], bb[447, 0] + bb[447, 1] - bb[256, 0])
    assert R.segment_cols(R.aa_tables(1920, 224, R.BILINEAR)[0]) == 1920
