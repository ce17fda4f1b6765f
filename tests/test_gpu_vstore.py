"""The vector store on the device (csrc/vstore.hip, csrc/vstore_model.hip): lmx_k_cosine_topk and lmx_k_unit_rows against their host
twin, bit for bit (np.array_equal on scores and slots), on the smallest shapes that reach every branch; batch and permutation
invariance; several passes per workgroup; row offsets past 2^31 and 2^32 bytes; the C handle and the C example."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vstoreref as V
from lmx import _lib, vstore
from lmx import kernels as K

pytestmark = pytest.mark.gpu


def _dev_topk(cuda, G, Q, k, limits=None, pad=0):
    """numpy in, numpy out; pad > 0: the gallery is a view of rows `pad` elements longer"""
    g = torch.from_numpy(G).to(cuda)
    if pad:
        wide = torch.full((G.shape[0], G.shape[1] + pad), 3.0, dtype=torch.float32, device=cuda)
        wide[:, : G.shape[1]] = g
        g = wide[:, : G.shape[1]]
    lim = None if limits is None else torch.from_numpy(np.ascontiguousarray(limits, np.int32)).to(cuda)
    s, i = K.cosine_topk(g, torch.from_numpy(Q).to(cuda), k, lim)
    return s.cpu().numpy(), i.cpu().numpy()


def _same(dev, host):
    return np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])


@pytest.mark.parametrize("D", [4, 260, 384, 1024, 4096])
def test_every_branch_against_the_twin(cuda, D):
    """N around the rows of a workgroup pass, Q around the query tile, k at both ends, dense rows and rows with a stride"""
    R, T, _ = vstore.geometry(D)
    rng = np.random.default_rng(D)
    n_max, q_max = 3 * R + 5, 2 * T + 3
    G, Q = V.unit_gauss(rng, n_max, D), V.unit_gauss(rng, q_max, D)
    for k in (1, 5, 32):
        for N in sorted({0, 1, k - 1, R - 1, R, R + 1, n_max}):
            for nq in sorted({1, max(T - 1, 1), T, T + 1, q_max}):
                g, q = np.ascontiguousarray(G[:N]), np.ascontiguousarray(Q[:nq])
                pad = 4 if (N + nq + k) % 2 else 0
                assert _same(_dev_topk(cuda, g, q, k, pad=pad), V.h_topk(g, q, k)), (D, N, nq, k, pad)


def test_duplicates_across_a_workgroup_boundary_and_negative_scores(cuda):
    D = 260
    R, T, _ = vstore.geometry(D)
    rng = np.random.default_rng(11)
    G, Q = V.unit_gauss(rng, 3 * R, D), V.unit_gauss(rng, 2, D)
    for s in (R - 1, R, 2 * R, 2 * R - 1):
        G[s] = Q[0]
    dev = _dev_topk(cuda, G, Q, 5)
    assert _same(dev, V.h_topk(G, Q, 5))
    assert dev[1][0, :4].tolist() == [R - 1, R, 2 * R - 1, 2 * R] and len(set(dev[0][0, :4].tolist())) == 1
    neg = V.ladder(rng, Q[1], 2 * R + 3, 0.15, 0.9, sign=-1.0)
    dev = _dev_topk(cuda, neg, Q[1:], 5)
    assert _same(dev, V.h_topk(neg, Q[1:], 5))
    assert dev[1][0].tolist() == [0, 1, 2, 3, 4] and (dev[0] < 0).all()


def test_limits(cuda):
    """limits of 0, inside a wave's rows, at a workgroup's edge, N and past N; and the backlog they stand for"""
    D = 384
    R, T, _ = vstore.geometry(D)
    rng = np.random.default_rng(12)
    N = 3 * R + 5
    G = V.unit_gauss(rng, N, D)
    limits = [0, 1, R + 1, R, 2 * R + 3, N, N + 7, 0, R - 1, 3 * R + 4, 2]
    Q = V.unit_gauss(rng, len(limits), D)
    dev = _dev_topk(cuda, G, Q, 5, limits)
    assert _same(dev, V.h_topk(G, Q, 5, limits))
    assert (dev[1][0] == -1).all() and (dev[0][0] == 0).all() and dev[1][1].tolist() == [0, -1, -1, -1, -1]
    for j, lim in enumerate(limits):
        assert dev[1][j].max() < max(min(lim, N), 0) or (dev[1][j] == -1).all()
    B = 2 * T + 3
    n0 = N - B
    new = np.ascontiguousarray(G[n0 : n0 + B])
    dev = _dev_topk(cuda, G, new, 5, n0 + np.arange(B))
    for j in range(B):  # B sequential search-then-append steps
        assert _same((dev[0][j : j + 1], dev[1][j : j + 1]), _dev_topk(cuda, np.ascontiguousarray(G[: n0 + j]), new[j : j + 1], 5))


def test_batch_invariance(cuda):
    """a query's results are the same bytes alone, first, last and in the middle of a batch of 2 T + 3"""
    D = 1024
    R, T, _ = vstore.geometry(D)
    rng = np.random.default_rng(13)
    G, Q = V.unit_gauss(rng, 5 * R + 3, D), V.unit_gauss(rng, 2 * T + 3, D)
    alone = _dev_topk(cuda, G, Q[:1], 5)
    for at in (0, T + 1, 2 * T + 2):
        batch = Q.copy()
        batch[[0, at]] = batch[[at, 0]]
        got = _dev_topk(cuda, G, batch, 5)
        assert _same((got[0][at : at + 1], got[1][at : at + 1]), alone), at


def test_permutation_invariance(cuda):
    """the gallery's rows permuted: the same scores, slots mapped through the permutation (no exact ties in this gallery)"""
    D = 260
    R, _, _ = vstore.geometry(D)
    rng = np.random.default_rng(14)
    G, Q = V.unit_gauss(rng, 7 * R + 1, D), V.unit_gauss(rng, 3, D)
    perm = rng.permutation(len(G))
    a, b = _dev_topk(cuda, G, Q, 8), _dev_topk(cuda, np.ascontiguousarray(G[perm]), Q, 8)
    assert (np.diff(a[0], axis=1) < 0).all()  # no exact ties
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], perm[b[1]])


def test_several_passes_per_workgroup(cuda):
    """every workgroup of the scan walks at least three passes (tests/test_gpu_persistent.py): D = 4 keeps it small"""
    D = 4
    R, T, per_cu = vstore.geometry(D)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    N = 3 * R * cus * per_cu + R + 3
    rng = np.random.default_rng(15)
    G, Q = V.unit_gauss(rng, N, D), V.unit_gauss(rng, 3, D)
    G[N - 2] = G[5] = Q[2]  # a tie between the first pass of one workgroup and the last of another
    dev = _dev_topk(cuda, G, Q, 5)
    assert _same(dev, V.h_topk(G, Q, 5))
    assert dev[1][2, :2].tolist() == [5, N - 2]


def test_row_offsets_past_2_31_and_2_32_bytes(cuda):
    """a 4.3 GB gallery of zero rows with three copies of the query: before 2^31 bytes, between, and after 2^32.  One launch"""
    N, D = 262_200, 4096
    planted = [100, 200_000, N - 1]
    assert planted[0] * D * 4 < 2 ** 31 < planted[1] * D * 4 < 2 ** 32 < planted[2] * D * 4
    q = V.unit_gauss(np.random.default_rng(16), 1, D)
    g = torch.zeros((N, D), dtype=torch.float32, device=cuda)
    tq = torch.from_numpy(q).to(cuda)
    for s in planted:
        g[s] = tq[0]
    scores, slots = (t.cpu().numpy() for t in K.cosine_topk(g, tq, 5))
    del g
    assert slots[0].tolist() == planted + [0, 1]
    assert scores[0, 0] == scores[0, 1] == scores[0, 2] and abs(float(scores[0, 0]) - 1) <= V.bound(D) + 2 ** -22
    assert (scores[0, 3:] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unit_rows_against_the_twin(cuda, dtype):
    rng = np.random.default_rng(17)
    for D in (4, 260, 1024, 4096):
        x = (rng.standard_normal((7, D)) * np.array([1e-3, 1, 1, 50, 1e4, 1, 3])[:, None]).astype(dtype)
        x[2] = 0
        assert np.array_equal(K.unit_rows(torch.from_numpy(x).to(cuda)).cpu().numpy(), V.h_unit(x)), D


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_handle(cuda):
    """lmx_vstore_* through ctypes: append, replace, grow past the capacity, get, search; the same bytes from lmx_k_cosine_topk over the
    handle's gallery and from the twin over the twin's unit rows"""
    lib = _lib.load()
    D, k = 260, 5
    rng = np.random.default_rng(18)
    raw = rng.standard_normal((17, D)) * 4
    raw32 = rng.standard_normal((9, D)).astype(np.float32)
    h = C.c_void_p()
    with torch.cuda.device(cuda):
        _lib.check(lib.lmx_vstore_open(D, 4, C.byref(h)), "open")
        try:
            for s in range(10):  # grows 4 -> 8 -> 16
                _lib.check(lib.lmx_vstore_put_host(h, s, _np_ptr(raw[s]), 2), "put")
            assert lib.lmx_vstore_count(h) == 10
            _lib.check(lib.lmx_vstore_put_host(h, 3, _np_ptr(raw[16]), 2), "replace")
            assert lib.lmx_vstore_count(h) == 10
            assert lib.lmx_vstore_put_host(h, 12, _np_ptr(raw[0]), 2) == V.EINVAL and "slot 12" in V.last_error()
            assert lib.lmx_vstore_put_host(h, -1, _np_ptr(raw[0]), 2) == V.EINVAL
            _lib.check(lib.lmx_vstore_append(h, C.c_void_p(torch.from_numpy(raw[10:16]).to(cuda).data_ptr()), 2, 6), "append")
            _lib.check(lib.lmx_vstore_append(h, C.c_void_p(torch.from_numpy(raw32).to(cuda).data_ptr()), 1, 9), "append f32")  # 25 > 16
            n = lib.lmx_vstore_count(h)
            assert n == 25
            want = np.concatenate([V.h_unit(np.concatenate([raw[:3], raw[16:17], raw[4:16]])), V.h_unit(raw32)])
            got = np.empty((n, D), np.float32)
            _lib.check(lib.lmx_vstore_read_host(h, 0, n, _np_ptr(got)), "read")
            assert np.array_equal(got, want)
            one = np.empty((D,), np.float32)
            _lib.check(lib.lmx_vstore_get_host(h, 3, _np_ptr(one)), "get")
            assert np.array_equal(one, want[3])
            assert lib.lmx_vstore_get_host(h, n, _np_ptr(one)) == V.EINVAL

            queries = rng.standard_normal((11, D))
            limits = np.array([0, 1, 25, 7, 25, 25, 12, 25, 3, 25, 25], np.int32)
            scores, slots = np.empty((11, k), np.float32), np.empty((11, k), np.int32)
            _lib.check(lib.lmx_vstore_search_host(h, _np_ptr(queries), 2, 11, _np_ptr(limits), k, _np_ptr(scores), _np_ptr(slots)), "search_host")
            assert _same((scores, slots), V.h_topk(want, V.h_unit(queries), k, limits))
            # the device entry point, and lmx_k_cosine_topk over the handle's own rows
            tq, tl = torch.from_numpy(queries).to(cuda), torch.from_numpy(limits).to(cuda)
            ds, di = torch.empty((11, k), dtype=torch.float32, device=cuda), torch.empty((11, k), dtype=torch.int32, device=cuda)
            st = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
            _lib.check(lib.lmx_vstore_search(h, C.c_void_p(tq.data_ptr()), 2, 11, C.c_void_p(tl.data_ptr()), k, C.c_void_p(ds.data_ptr()),
                                             C.c_void_p(di.data_ptr()), st), "search")
            assert _same((ds.cpu().numpy(), di.cpu().numpy()), (scores, slots))
            gal, ldg = C.c_void_p(), C.c_int64()
            _lib.check(lib.lmx_vstore_gallery(h, C.byref(gal), C.byref(ldg)), "gallery")
            ws = torch.empty((max(int(lib.lmx_h_cosine_topk_workspace(n, 11, k)), 8),), dtype=torch.uint8, device=cuda)
            ks, ki = torch.empty_like(ds), torch.empty_like(di)
            _lib.check(lib.lmx_k_cosine_topk(gal, n, D, ldg.value, C.c_void_p(K.unit_rows(tq).data_ptr()), 11, C.c_void_p(tl.data_ptr()), k,
                                             C.c_void_p(ks.data_ptr()), C.c_void_p(ki.data_ptr()), C.c_void_p(ws.data_ptr()), st), "topk")
            assert _same((ks.cpu().numpy(), ki.cpu().numpy()), (scores, slots))

            # refusals: LMX_EINVAL, a message, nothing launched (the outputs keep what they held)
            ds.fill_(-5.0)
            for kk, dt in ((0, 2), (33, 2), (5, 7)):
                rc = lib.lmx_vstore_search(h, C.c_void_p(tq.data_ptr()), dt, 11, None, kk, C.c_void_p(ds.data_ptr()), C.c_void_p(di.data_ptr()), st)
                assert rc == V.EINVAL and "lmx_vstore_search" in V.last_error()
            torch.cuda.synchronize(cuda)
            assert (ds == -5.0).all()
            if torch.cuda.device_count() > 1:
                with torch.cuda.device(1):
                    rc = lib.lmx_vstore_search_host(h, _np_ptr(queries), 2, 11, None, k, _np_ptr(scores), _np_ptr(slots))
                    assert rc == V.EINVAL and "opened on device 0" in V.last_error()
        finally:
            lib.lmx_vstore_close(h)
        bad = C.c_void_p()
        for dim in (6, 0, 4100):
            assert lib.lmx_vstore_open(dim, 4, C.byref(bad)) == V.EINVAL and "lmx_vstore_open" in V.last_error() and not bad.value


def test_kernel_refusals(cuda):
    g = torch.zeros((8, 8), dtype=torch.float32, device=cuda)
    for gal, q, k in ((g[:, :6], g[:1, :6].contiguous(), 5), (g, g[:1], 0), (g, g[:1], 33), (g[:, 1:5], g[:1, :4].contiguous(), 5)):
        with pytest.raises(K.LmxError, match="lmx_k_cosine_topk"):
            K.cosine_topk(gal, q, k)
    with pytest.raises(K.LmxError, match="lmx_k_unit_rows"):
        K.unit_rows(torch.zeros((2, 6), dtype=torch.float32, device=cuda))


def test_example_vstore_search(cuda, tmp_path):
    """examples/vstore_search.c, compiled with cc against include/lmx.h and liblmx.so and run as a child process: it prints the
    planted neighbour"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "vstore_search"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "vstore_search.c"),
                    "-o", str(exe), "-L", libdir, "-llmx", "-L", os.path.join(rocm, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}"], check=True,
                   timeout=120)
    _lib.load()
    # the HIP runtime this process loaded, first on the child's search path (as tests/test_gpu_native_yolo.py does)
    hip = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(hip) == 1, hip
    hipdir, soname, search = os.path.dirname(hip[0]), "libamdhip64.so.7", [os.path.dirname(hip[0])]
    if not os.path.exists(os.path.join(hipdir, soname)):
        rt = tmp_path / "rt"
        rt.mkdir()
        os.symlink(hip[0], rt / soname)
        search.append(str(rt))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(search + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
    r = subprocess.run([str(exe), "300", "384", "41"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "vstore_search: 300 rows of 384 elements" and lines[1].startswith("rank 0 slot 41 score 0.9")
    assert lines[-1] == "planted neighbour found: slot 41"
