"""lmx_k_pack_records (csrc/records.hip): the record matrix of lmx.dist.pack_records from one launch that stores every byte once.
The bar is EQUALITY with the torch path: dist.pack_records for the identity layout, and for row maps a torch restatement of
FusedExtractor.step's scatter (zeros, then index_copy_ per field).  One record holds every row size at which the kernel takes another
path: below a word (1, 3, 4, 7), a word (8), a word and a ragged tail (13, 17), two words (16), long rows of whole 16-byte blocks
(4800) and a long row that is even but no multiple of 4 (150 * 13 = 1950: mask bits of a 150 x 100 frame); the sources start on odd
addresses, and `out` starts as 0xFF so that a byte the kernel leaves out shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
ROW_BYTES = (1, 3, 4, 7, 8, 13, 16, 17, 4800, 150 * 13)


def _fields(dev, n, odd=True, seed=0):
    """{name: uint8 [n, row_bytes]} of random bytes; odd: each tensor is a slice that starts one byte into its allocation"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rec = {}
    for i, nb in enumerate(ROW_BYTES):
        flat = torch.randint(0, 256, (n * nb + 1,), dtype=torch.uint8, generator=g).to(dev)
        t = flat[1:].view(n, nb) if odd else flat[:n * nb].view(n, nb)
        assert not odd or n == 0 or t.data_ptr() % 2 == 1
        rec[f"f{i:02d}_{nb}"] = t
    return rec


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_equals_dist_pack_records(cuda, n, extra):
    from lmx import dist
    from lmx import kernels as K

    rec = _fields(cuda, n)
    want, want_layout = dist.pack_records(rec, n + extra)
    out = torch.full_like(want, 0xFF)
    got, layout = K.pack_records(rec, n + extra, out=out)
    assert got is out and layout == want_layout
    assert tuple(got.shape) == (n + extra, want.shape[1])
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} bytes differ"
    fresh, _ = K.pack_records(rec, n + extra)  # the wrapper's own torch.empty
    assert torch.equal(fresh, want)


def test_typed_fields_aligned_sources_and_an_out_that_starts_on_an_odd_word(cuda):
    """the step's own dtypes (16-byte aligned sources: the 16-byte loads), into rows 1 .. of a larger matrix: `out` is 8 mod 16"""
    from lmx import dist
    from lmx import kernels as K

    g = torch.Generator(device="cpu").manual_seed(3)
    n = 3
    rec = dict(boxes=torch.randn((n, 300, 4), generator=g), cls=torch.randint(0, 80, (n, 300), dtype=torch.int32, generator=g),
               counts=torch.randint(0, 300, (n,), dtype=torch.int32, generator=g), embedding=torch.randn((n, 390), generator=g),
               mask_bits=torch.randint(0, 256, (n, 90, 20), dtype=torch.uint8, generator=g),
               mask_stats=torch.randint(-2 ** 40, 2 ** 40, (n, 8), dtype=torch.int64, generator=g), mask_iou=torch.randn((n,), generator=g))
    rec = {k: v.to(cuda) for k, v in rec.items()}
    want, _ = dist.pack_records(rec, n + 1)
    stride = want.shape[1]
    assert stride % 16 == 8  # a row ahead moves the matrix onto the second word of a 16-byte block
    big = torch.full((n + 3, stride), 0xFF, dtype=torch.uint8, device=cuda)
    out = big[1:n + 2]
    assert out.data_ptr() % 16 == 8
    got, layout = K.pack_records(rec, n + 1, out=out)
    assert torch.equal(got, want)
    assert bool((big[0] == 0xFF).all()) and bool((big[n + 2] == 0xFF).all()), "bytes outside out were written"
    back = dist.unpack_records(got, layout)
    assert all(torch.equal(back[k], rec[k]) for k in rec)


def _scatter_reference(rec, maps, field_map, n_valid, n_rows):
    """zeros, then index_copy_ of each field through its map (FusedExtractor.step), packed by dist.pack_records"""
    from lmx import dist

    full = {}
    for k, v in rec.items():
        o = torch.zeros((n_valid,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
        if k in field_map:
            m = maps[field_map[k]].long()
            rows = torch.nonzero(m >= 0)[:, 0]
            o.index_copy_(0, rows, v[m[rows]])
        else:
            k_rows = min(n_valid, v.shape[0])
            o[:k_rows] = v[:k_rows]
        full[k] = o
    return dist.pack_records(full, n_rows)[0]


@pytest.mark.parametrize("case", ["permuted", "sparse", "none"])
def test_row_maps_equal_the_index_copy_restatement(cuda, case):
    from lmx import kernels as K

    n_valid, n_rows = 5, 7
    rec = _fields(cuda, 5, seed=1)
    names = sorted(rec)
    few = {k: rec[k][:2] for k in names[5:]}  # the second map's fields hold two rows only
    rec = {**{k: rec[k] for k in names[:5]}, **few}
    first = {"permuted": [3, 0, 4, 1, 2], "sparse": [-1, 2, -1, -1, 0], "none": [-1] * 5}[case]
    second = {"permuted": [1, -1, 0, -1, -1], "sparse": [-1, -1, -1, 1, -1], "none": [-1] * 5}[case]
    maps = [torch.tensor(m, dtype=torch.int32, device=cuda) for m in (first, second)]
    field_map = {**{k: 0 for k in names[1:5]}, **{k: 1 for k in names[5:9]}}  # names[0] and names[9] keep the identity
    want = _scatter_reference(rec, maps, field_map, n_valid, n_rows)
    out = torch.full_like(want, 0xFF)
    got, _ = K.pack_records(rec, n_rows, row_maps=maps, field_map=field_map, n_valid=n_valid, out=out)
    assert torch.equal(got, want), f"{case}: {int((got != want).sum())} of {got.numel()} bytes differ"
    assert bool((got[n_valid:] == 0).all()) and bool((got[:n_valid, 0] == 1).all())


def test_refusals(cuda):
    from lmx import kernels as K

    rec = _fields(cuda, 3)
    with pytest.raises(K.LmxError, match="do not fit"):
        K.pack_records(rec, 2)
    with pytest.raises(K.LmxError, match="rows, expected"):
        K.pack_records({**rec, "short": torch.zeros((2, 4), dtype=torch.uint8, device=cuda)})
    with pytest.raises(K.LmxError, match="row map"):
        K.pack_records(rec, 3, row_maps=[torch.zeros(2, dtype=torch.int32, device=cuda)], field_map={sorted(rec)[0]: 0})
    lib = K._lib.load()
    f = (K._lib.RecordField * 2)()
    f[0].src, f[0].row_bytes, f[0].offset, f[0].map, f[0].n_src = rec[sorted(rec)[0]].data_ptr(), 4, 8, -1, 3
    f[1].src, f[1].row_bytes, f[1].offset, f[1].map, f[1].n_src = rec[sorted(rec)[1]].data_ptr(), 4, 8, -1, 3
    out = torch.empty((3, 24), dtype=torch.uint8, device=cuda)
    assert lib.lmx_k_pack_records(f, 2, None, 0, 3, 3, 24, out.data_ptr(), None) == -1 and "field 1 at offset 8" in lib.lmx_last_error().decode()
    assert lib.lmx_k_pack_records(f, 1, None, 0, 3, 3, 20, out.data_ptr(), None) == -1 and "stride 20" in lib.lmx_last_error().decode()
    assert lib.lmx_k_pack_records(f, 1, None, 0, 4, 3, 24, out.data_ptr(), None) == -1 and "n_valid 4" in lib.lmx_last_error().decode()
    f[0].map = 0
    assert lib.lmx_k_pack_records(f, 1, None, 0, 3, 3, 24, out.data_ptr(), None) == -1 and "follows map 0 of 0" in lib.lmx_last_error().decode()
