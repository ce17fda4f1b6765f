"""The host arithmetic of the fused record (csrc/host_records.cpp) against the Python it restates, without a GPU:
lmx_h_record_layout == lmx.dist.record_layout of the dict FusedExtractor.step returns, lmx_h_stream_plan == lmx.pipeline.stream_plan,
and lmx_h_row_map == the index_copy_ / index_fill_ scatter of FusedExtractor.step's reference schedule, with every malformed index
list refused by name.  The sweeps are shared with tests/test_fused_sanitized.py, which runs them again in a stand-alone program."""
import itertools
import re

import pytest
import torch

from lmx import dist, pipeline
from lmx import kernels as K

SIZES = [(180, 320), (90, 160), (150, 100), (1080, 1920), (1, 1), (7, 9), (64, 64), (33, 1023)]  # widths with and without w % 8 == 0
HIDDENS = [384, 768, 1024, 4 * 97]                                                            # ... one odd multiple of 4
MAX_DETS = [300, 1, 7]
ROW_MAP_CASES = [(5, [0, 3]), (5, [0, 4]), (5, []), (5, [0, 1, 2, 3, 4]), (1, [0]), (0, []), (7, [6]), (9, [1, 2, 5, 8])]
BAD_ROW_MAPS = [(5, [0, 5], "det_idx[1] = 5 outside 0 .. 4"), (5, [-1], "det_idx[0] = -1 outside 0 .. 4"), (5, [2, 2], "det_idx[1] = 2 repeats det_idx[0]"),
                (5, [3, 1], "det_idx[1] = 1 after det_idx[0] = 3"), (0, [0], "names 1 frames of 0"), (3, [0, 1, 2, 2], "names 4 frames of 3"),
                (4, [0, 1, 3, 2], "det_idx[3] = 2 after det_idx[2] = 3")]


def step_dict(n, h, w, hidden, max_det, scheduled):
    """the dict FusedExtractor.step returns (lmx/pipeline.py: the dense dict of _step_dense, plus ran_det / ran_emb under a schedule),
    with the dtypes its kernels write"""
    z = torch.zeros
    d = dict(boxes=z((n, max_det, 4)), scores=z((n, max_det)), cls=z((n, max_det), dtype=torch.int32), counts=z((n,), dtype=torch.int32),
             embedding=z((n, hidden)), mask_bits=z((n, h, (w + 7) // 8), dtype=torch.uint8), mask_stats=z((n, 8), dtype=torch.int64),
             mask_contour=z((n, 8), dtype=torch.int64), mask_iou=z((n,)))
    if scheduled:
        d.update(ran_det=z((n,), dtype=torch.int32), ran_emb=z((n,), dtype=torch.int32))
    return d


def layout_queries():
    return [(h, w, hidden, md, sch) for (h, w), hidden, md, sch in itertools.product(SIZES, HIDDENS, MAX_DETS, (0, 1))]


def plan_queries():
    return [(n, s, lay) for n in range(0, 13) for s in range(1, 10) for lay in ("lanes", "rr")]


def test_record_layout_equals_dist_record_layout():
    for h, w, hidden, md, sch in layout_queries():
        want = dist.record_layout(step_dict(2, h, w, hidden, md, sch))
        assert K.record_layout(h, w, hidden, md, sch) == want, (h, w, hidden, md, sch)
    names = [f[0] for f in K.record_layout(150, 100, 384, scheduled=True)[0]]
    assert names == "boxes cls counts embedding mask_bits mask_contour mask_iou mask_stats ran_det ran_emb scores".split()
    assert dict((f[0], f[4]) for f in K.record_layout(150, 100, 384)[0])["mask_bits"] == 150 * 13


def test_record_layout_refusals():
    for args, text in (((0, 8, 384, 300, 0), "frame size 0 x 8"), ((8, -1, 384, 300, 0), "frame size 8 x -1"), ((8, 8, 0, 300, 0), "hidden = 0"),
                       ((8, 8, 384, 0, 0), "max_det = 0")):
        with pytest.raises(K.LmxError, match=text):
            K.record_layout(*args)


def test_stream_plan_equals_pipeline_stream_plan():
    for n, s, lay in plan_queries():
        assert K.stream_plan(n, s, lay) == pipeline.stream_plan(n, s, lay), (n, s, lay)
    lib = K._lib.load()
    assert lib.lmx_h_stream_plan(2, 4, 2, None, None, None, None) == -1 and "layout 2" in lib.lmx_last_error().decode()
    assert lib.lmx_h_stream_plan(-1, 4, 0, None, None, None, None) == -1 and "n_chunks = -1" in lib.lmx_last_error().decode()


def scatter_reference(n, idx):
    """what FusedExtractor.step does with an index list: out.index_copy_(0, idx, part) and ran.index_fill_(0, idx, 1); the source row
    that lands in row r, or -1 where the zeros stay"""
    ii = torch.as_tensor(idx, dtype=torch.int64)
    out = torch.zeros((n,), dtype=torch.int64)
    out.index_copy_(0, ii, torch.arange(1, len(idx) + 1))  # part row j tagged j + 1
    ran = torch.zeros((n,), dtype=torch.int32)
    ran.index_fill_(0, ii, 1)
    return (out - 1).tolist(), ran.tolist()


def test_row_map_equals_the_index_copy_scatter():
    for n, idx in ROW_MAP_CASES:
        assert K.row_map(n, idx) == scatter_reference(n, idx), (n, idx)
    for n in range(0, 7):  # every ascending subset of up to 6 frames
        for k in range(n + 1):
            for idx in itertools.combinations(range(n), k):
                assert K.row_map(n, idx) == scatter_reference(n, list(idx))


@pytest.mark.parametrize("n,idx,text", BAD_ROW_MAPS)
def test_row_map_names_the_bad_index(n, idx, text):
    with pytest.raises(K.LmxError, match=re.escape(text)):
        K.row_map(n, idx, what="det_idx")
