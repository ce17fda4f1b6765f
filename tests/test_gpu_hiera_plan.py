"""The Hiera trunk executes its block plan (lmx/sam.py hiera_plan) with the launches, in the order, and to the bits of the encoder
before the plan existed: test_gpu_hiera_plan.json beside this file holds, per case, the ordered launch keys of one encode() and the
SHA-256 of every stage and FPN output, recorded from that earlier encoder by record() below.  Hiera-B+ widths on a 256-pixel
canvas (grids 64 / 32 / 16 / 8: every fused kernel's divisibility holds, windows 14 and 7 are padded; one frame keeps block 21
under pooled_gemm_ok's 512-row floor, two put it over), a 1080 x 1920 frame (band 56 of 64 rows)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
SWITCHES = ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL", "LMX_MLP_IMG")
# (frames, band, switches at "0"): default switches on every batch size and both paths, all four off once
CASES = [(1, True, False), (2, True, False), (1, False, False), (2, False, False), (2, True, True)]


def _case_id(n, band, off):
    return f"n{n}-{'band' if band else 'whole'}-{'unfused' if off else 'default'}"


def _digest(t):
    a = t.detach().cpu().numpy()
    return hashlib.sha256((str(a.dtype) + str(a.shape)).encode() + a.tobytes()).hexdigest()


def _encoders(cuda):
    from lmx import sam, weights

    cfg = sam.HieraConfig(image=256)
    sd = weights.synth_state_dict(sam.param_spec(cfg), 5)
    return {True: sam.HieraEncoder(cfg, sd, cuda), False: sam.HieraEncoder(cfg, sd, cuda, band=False)}


def _run(enc, cuda, n):
    """-> dict(band, launches = the ordered launch keys of one encode(), digests = {output name: SHA-256})."""
    from lmx import kernels as K
    from lmx import sam

    frames = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)[:n]).to(cuda)
    band = enc.band_rows(*sam.resize_longest_side(1080, 1920, enc.cfg.image)) if enc.band else 0
    if band:
        enc.encode(frames)  # builds the table of constant rows, outside the trace
    K.start_launch_trace()
    try:
        out = enc.encode(frames)
        launches = [key for _, key, *_ in K.LAUNCH_TRACE]
    finally:
        K.stop_launch_trace()
    digests = {f"{name}{lvl}": _digest(t) for name in ("fpn", "stages") for lvl, t in enumerate(out[name])}
    return dict(band=band, launches=launches, digests=digests)


def record(cuda, path):
    """Write the golden file from the encoder as it stands (run at the commit whose behaviour is to be kept)."""
    encs, rec = _encoders(cuda), {}
    for n, band, off in CASES:
        old = {v: os.environ.get(v) for v in SWITCHES}
        try:
            if off:
                os.environ.update({v: "0" for v in SWITCHES})
            rec[_case_id(n, band, off)] = _run(encs[band], cuda, n)
        finally:
            for v, val in old.items():
                os.environ.pop(v, None) if val is None else os.environ.__setitem__(v, val)
    with open(path, "w") as f:
        json.dump(rec, f, indent=0)
    return rec


@pytest.fixture(scope="module")
def encoders(cuda):
    return _encoders(cuda)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("n,band,off", CASES, ids=[_case_id(*c) for c in CASES])
def test_launches_and_bits_are_those_recorded(cuda, encoders, golden, monkeypatch, n, band, off):
    if off:
        for v in SWITCHES:
            monkeypatch.setenv(v, "0")
    got, want = _run(encoders[band], cuda, n), golden[_case_id(n, band, off)]
    assert got["band"] == want["band"] == (56 if band else 0)
    for i, (a, b) in enumerate(zip(got["launches"], want["launches"])):
        assert a == b, f"launch {i}: {a!r}, recorded {b!r}"
    assert len(got["launches"]) == len(want["launches"])
    assert got["digests"] == want["digests"]
