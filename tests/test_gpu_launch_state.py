"""Per-device launch state of liblmx (csrc/api.hip: lmx_stream_device, lmx_cu_count, lmx_allow_lds): the first launches of a
process, made by several host threads at once, and made on a device that is not the current one.

First-use state exists once per loaded library, so each case runs in ONE fresh child interpreter (this file as a script); the
parent only checks its exit status.  The four calls are the launchers that raise a kernel's LDS limit and / or size a
persistent grid from the CU count: lmx_k_hiera_attn4, lmx_k_ln_mlp_img (both), lmx_k_gemm at a shape that takes gemm2's
3 x 48 KB ring, lmx_k_attention on 14 x 14 windows with >= 64 (window, head) items (attn_spp_kernel)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def _operands(dev):
    """name -> call: call() makes ONE lmx_k_* launch on torch's current stream of `dev` (lmx.kernels raises unless it returns LMX_OK)
    and returns the tensor it wrote, a fresh one per call.  Building the operands launches nothing from liblmx."""
    import numpy as np
    import torch

    from lmx import kernels as K
    from lmx import sam

    def rand(shape, seed, scale=1.0):
        return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))

    ops = {}
    # hiera_attn4: D = 224, 4 heads, 2 images of 32 x 32 tokens
    D, heads, n, G = 224, 4, 2, 32
    wqkv, bqkv = rand((3 * D, D), 1) * D ** -0.5, rand((3 * D,), 2, 0.2)
    wo, bo = rand((D, D), 3) * D ** -0.5, rand((D,), 4, 0.2)
    pk4 = tuple(torch.from_numpy(a).to(dev) for a in sam.pack_hiera_attn4(wqkv.half().float().numpy(), bqkv.numpy(), wo.half().float().numpy(), bo.numpy(), heads))
    h4, x4 = rand((n * G * G, D), 5).half().to(dev), rand((n * G * G, D), 6).to(dev)
    ops["hiera_attn4"] = lambda: K.hiera_attn4(h4, x4.clone(), pk4, n, G, G, heads)
    # ln_mlp_img: D = 112, 5000 rows
    Dm, rows = 112, 5000
    w1, b1 = rand((4 * Dm, Dm), 7) * Dm ** -0.5, rand((4 * Dm,), 8, 0.2)
    w2, b2 = rand((Dm, 4 * Dm), 9) * (4 * Dm) ** -0.5, rand((Dm,), 10, 0.2)
    vec = [1.0 + rand((Dm,), 11, 0.2), rand((Dm,), 12, 0.2), 1.0 + rand((Dm,), 13, 0.2), rand((Dm,), 14, 0.2)]
    pkm = tuple(torch.from_numpy(a).to(dev) for a in sam.pack_ln_mlp(w1.half().float().numpy(), b1.numpy(), w2.half().float().numpy(), b2.numpy(),
                                                                      *(v.numpy() for v in vec)))
    xm = (rand((rows, Dm), 15) + 0.2).to(dev)
    ops["ln_mlp_img"] = lambda: K.ln_mlp_img(xm.clone(), pkm, 1e-6)
    # gemm: 1024 x 256 x 256 is 8 tiles of 256 x 128 (<= 256): gemm2's staggered 256 x 128 x 64 tiling on a 3 x 48 KB ring
    a, w, bias = rand((1024, 256), 16).half().to(dev), (rand((256, 256), 17) / 16).half().to(dev), rand((256,), 18).to(dev)
    ops["gemm"] = lambda: K.gemm(a, w, bias=bias)
    # attention: 12 images of 28 x 28 tokens in 14 x 14 windows, 2 heads of 56: 96 (window, head) items -> attn_spp_kernel
    na, Ga, ws, Ha, hd = 12, 28, 14, 2, 56
    Da = Ha * hd
    qkv, pad = rand((na * Ga * Ga, 3 * Da), 19, 1.5).half().to(dev), rand((3 * Da,), 20).half().to(dev)

    def attention():
        out = torch.zeros((na * Ga * Ga, Da), dtype=torch.float16, device=dev)
        return K.attention(qkv[:, :Da].contiguous(), qkv[:, Da:2 * Da], qkv[:, 2 * Da:], out, na * (Ga // ws) ** 2, Ha, ws * ws, ws * ws, hd, hd ** -0.5,
                           window=dict(Gh=Ga, Gw=Ga, ws=ws, q_stride=1), pad_k=pad[Da:2 * Da], pad_v=pad[2 * Da:])

    ops["attention"] = attention
    return ops


def _child_threads():
    """4 threads, each on its own stream, make the process's FIRST four launches in four different orders; then the same calls
    serially on the default stream: every output must be the same bits, every call must have returned LMX_OK."""
    import threading

    import torch

    dev = torch.device("cuda:0")
    ops = _operands(dev)
    names = list(ops)
    torch.cuda.synchronize(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    start = threading.Barrier(4)
    got, errors = [None] * 4, []

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                start.wait()
                got[t] = {name: ops[name]() for name in names[t:] + names[:t]}
                streams[t].synchronize()
        except BaseException as e:  # LmxError: an lmx_k_* call did not return LMX_OK
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    serial = {name: ops[name]() for name in names}
    torch.cuda.synchronize(dev)
    for t in range(4):
        for name in names:
            assert torch.equal(got[t][name], serial[name]), f"thread {t}: {name} differs from the serial launch"
    print("threads ok:", ", ".join(names))


def _child_second_device():
    """The first hiera_attn4 and attn_spp launches of the process go to cuda:1 while cuda:0 is current, then to cuda:0.  Each device
    gets a stream of its own as its current stream: torch's default stream is the null stream, which belongs to no device, so a
    launch on it would go to the current device whatever device the operands are on."""
    import torch

    res = {}
    for d in (1, 0):
        dev = torch.device("cuda", d)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)  # (makes cuda:d current as well)
        torch.cuda.set_device(0)
        ops = _operands(dev)
        res[d] = {}
        for name in ("hiera_attn4", "attention"):
            assert torch.cuda.current_stream(dev).cuda_stream == stream.cuda_stream != 0 and torch.cuda.current_device() == 0
            res[d][name] = ops[name]()
            assert res[d][name].device == dev
        stream.synchronize()
    for name in res[0]:
        assert torch.equal(res[0][name].cpu(), res[1][name].cpu()), f"{name}: cuda:1 and cuda:0 differ"
    print("second device ok")


def _run_child(case):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, f"child '{case}' exited with {r.returncode}:\n{r.stderr[-4000:]}"


def test_first_launches_from_four_threads(cuda):
    _run_child("threads")


def test_first_launches_on_second_device(cuda):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: the per-device path needs two")
    _run_child("second_device")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "vision-sam3-yolo-lameless_amd")]
    {"threads": _child_threads, "second_device": _child_second_device}[sys.argv[1]]()
