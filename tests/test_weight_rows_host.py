"""The weight tables of the TCN, the gait transformer, the graph transformer and GraphGPS, as the library states them
(lmx_h_<model>_tensors; csrc/weights_table.h, lmx_<model>_tensor_rows in csrc/host_<model>.cpp), held to the two things nothing else
derives from them: the ctypes structs of lmx/_lib.py (every row's pointer offset is the offset of the field its name stands for) and
pack_tensors (names and shapes, in order).  Per model over every configuration of its ref module and the corners of the table: the
most layers, GraphGPS with one live layer (no edge update at all), a TCN without and one with a residual convolution in every block.
Host arithmetic only."""
import ctypes as C
import dataclasses
import functools
import os
import re

import pytest
import torch

import gfmref
import gnnref
import tcnref
import xfmref
from lmx import _lib, checkpoints, gfm, gnn, tcn, xfm
from lmx import kernels as K

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TENSOR_ROWS = int(re.search(r"#define LMX_MAX_TENSOR_ROWS (\d+)", open(os.path.join(ROOT, "include", "lmx.h")).read()).group(1))


def _layered(name):
    """(field, index) of a tensor named as its field of the weights struct: "layer.3.qkv_w" -> ("qkv_w", 3), "vu1_w" -> ("vu1_w", 0)"""
    parts = name.split(".")
    return (parts[2], int(parts[1])) if parts[0] == "layer" else (name, 0)


def _xfm_field(name):
    parts = name.split(".")
    if parts[0] == "layer":
        return f"{parts[2]}_{parts[3]}", int(parts[1])
    return "_".join(parts[1:] if parts[0] == "head" else parts), 0


def _tcn_field(name):
    parts = name.split(".")
    if parts[0] == "head":
        return f"{parts[1]}_{parts[2]}", 0
    block = int(parts[1])
    if parts[2] == "res":
        return f"res_{parts[3]}", block
    return f"conv_{parts[3]}", 2 * block + int(parts[2][-1]) - 1


def _changes(cfg):
    return sum(a != b for a, b in zip((cfg.input_dim,) + tuple(cfg.channels), cfg.channels))


@dataclasses.dataclass(frozen=True)
class Model:
    name: str
    Struct: type
    ref: object
    args: object        # cfg -> the positional arguments of K.<model>_check_config / _tensor_shapes / _weights
    packed: object      # cfg -> pack_tensors over a seeded random state dict
    field: object       # tensor name -> (field of Struct, index)
    count: object       # cfg -> the closed form of the row count
    corners: tuple
    bad: tuple          # (field, value, the text that names it): one value per field outside the list, from the bad-image tables and, for
                        # the fields those leave out, the first value past the list of include/lmx.h


def _tcn_packed(cfg):
    return tcn.pack_tensors(cfg, checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 3), cfg.dropout)[1])


def _xfm_packed(cfg):
    return xfm.pack_tensors(cfg, checkpoints.xfm_from_state_dict(xfmref.state_dict(cfg, 3), n_heads=cfg.n_heads, dropout=cfg.dropout,
                                                                 max_len=cfg.max_len)[1])


def _gfm_packed(cfg):
    return gfm.pack_tensors(cfg, checkpoints.gfm_from_state_dict(gfmref.state_dict(cfg, 3), num_heads=cfg.n_heads, dropout=cfg.dropout)[1])


def _gnn_packed(cfg):
    return gnn.pack_tensors(cfg, checkpoints.gnn_from_state_dict(gnnref.state_dict(cfg, 3), num_heads=cfg.n_heads, dropout=cfg.dropout)[1])


MODELS = {
    "tcn": Model("tcn", _lib.TcnWeights, tcnref, lambda c: (c.input_dim, c.channels, c.kernel_size, c.head), _tcn_packed, _tcn_field,
                 lambda c: 4 * len(c.channels) + 2 * _changes(c) + 4,
                 (tcn.TcnConfig(input_dim=32, channels=(32, 32, 32), kernel_size=2, head=8),          # no res.* at all
                  tcn.TcnConfig(input_dim=5, channels=(16, 32, 64, 32), kernel_size=3, head=8),       # res.* in every block
                  tcn.TcnConfig(input_dim=44, channels=(16,) * 8, kernel_size=2, head=8)),            # the most blocks
                 (("n_blocks", -3, "n_blocks -3"), ("k", 4, "k 4"), ("channels", 24, "channels[0] = 24"), ("input_dim", 65, "input_dim 65"),
                  ("head", 65, "head 65"))),
    "xfm": Model("xfm", _lib.XfmWeights, xfmref, lambda c: c.shape(), _xfm_packed, _xfm_field, lambda c: 3 + 12 * c.n_layers + 6,
                 (dataclasses.replace(xfmref.TINY, n_layers=8),),
                 (("d_model", 24, "d_model 24"), ("n_heads", 0, "n_heads 0"), ("n_layers", 9, "n_layers 9"), ("ff", 40, "ff 40"),
                  ("input_dim", 65, "input_dim 65"), ("head", 65, "head 65"), ("max_len", 161, "max_len 161"))),
    "gfm": Model("gfm", _lib.GfmWeights, gfmref, lambda c: c.shape(), _gfm_packed, _layered, lambda c: 14 + 17 * c.n_layers + 26,
                 (dataclasses.replace(gfmref.TINY, n_layers=8),),
                 (("d_model", 40, "d_model 40"), ("n_heads", 0, "n_heads 0"), ("n_layers", 9, "n_layers 9"), ("ff", 520, "ff 520"),
                  ("edge_dim", 4, "edge_dim 4"), ("max_spd", 31, "max_spd 31"), ("input_dim", 65, "input_dim 65"),
                  ("max_degree", 256, "max_degree 256"))),
    "gnn": Model("gnn", _lib.GnnWeights, gnnref, lambda c: c.shape(), _gnn_packed, _layered, lambda c: 20 + 32 * c.n_layers - 8 + 16,
                 (dataclasses.replace(gnnref.TINY, n_layers=4), dataclasses.replace(gnnref.WIDE, n_layers=1)),
                 (("d_model", 40, "d_model 40"), ("n_heads", 0, "n_heads 0"), ("n_layers", 5, "n_layers 5"), ("pe_dim", 12, "pe_dim 12"),
                  ("ff", 520, "ff 520"), ("edge_dim", 4, "edge_dim 4"), ("input_dim", 65, "input_dim 65"))),
}
CASES = [(m.name, i) for m in MODELS.values() for i in range(len(m.ref.CONFIGS) + len(m.corners))]


@functools.lru_cache(maxsize=None)
def _case(model, i):
    """(Model, cfg, the struct with the configuration's integers, the library's rows, pack_tensors' dict): made once per case"""
    m = MODELS[model]
    cfg = (tuple(m.ref.CONFIGS.values()) + m.corners)[i]
    ints = K._tcn_ints(*m.args(cfg)) if model == "tcn" else K._ints(m.Struct, *m.args(cfg))
    w = K._model_config(m.Struct, "test", ints)
    return m, cfg, w, K._model_rows(model, "test", w), m.packed(cfg)


def _slots(Struct):
    """byte offset of every pointer of the struct"""
    out = []
    for name, ctype in Struct._fields_:
        element = ctype
        while issubclass(element, C.Array):
            element = element._type_
        if element is C.c_void_p:
            out += range(getattr(Struct, name).offset, getattr(Struct, name).offset + C.sizeof(ctype), 8)
    return out


def test_the_corners_are_corners():
    t = MODELS["tcn"].corners
    assert _changes(t[0]) == 0 and _changes(t[1]) == len(t[1].channels) and len(t[2].channels) == _lib.TcnWeights.MAX_BLOCKS
    assert MODELS["xfm"].corners[0].n_layers == _lib.XfmWeights.MAX_LAYERS and MODELS["gfm"].corners[0].n_layers == _lib.GfmWeights.MAX_LAYERS
    assert [c.n_layers for c in MODELS["gnn"].corners] == [_lib.GnnWeights.MAX_LAYERS, 1]
    assert not any("eu1_w" in name or "bne_var" in name for name, _, _ in _case("gnn", len(gnnref.CONFIGS) + 1)[3])
    assert not any(".res." in name for name, _, _ in _case("tcn", len(tcnref.CONFIGS))[3])


@pytest.mark.parametrize("model,i", CASES)
def test_rows_point_at_the_fields_their_names_stand_for(model, i):
    m, cfg, _, rows, _ = _case(model, i)
    for name, _, at in rows:
        field, index = m.field(name)
        assert at == getattr(m.Struct, field).offset + 8 * index, (name, at)
        assert index * 8 < C.sizeof(dict(m.Struct._fields_)[field]), name
    offsets = [at for _, _, at in rows]
    assert len(set(offsets)) == len(offsets) and all(at % 8 == 0 and 0 <= at <= C.sizeof(m.Struct) - 8 for at in offsets)
    assert set(offsets) <= set(_slots(m.Struct))


@pytest.mark.parametrize("model,i", CASES)
def test_rows_are_pack_tensors_in_order_and_number(model, i):
    m, cfg, _, rows, packed = _case(model, i)
    assert [(name, shape) for name, shape, _ in rows] == [(k, tuple(v.shape)) for k, v in packed.items()]
    assert len(rows) == m.count(cfg) <= MAX_TENSOR_ROWS
    assert list(getattr(K, f"{model}_tensor_shapes")(*m.args(cfg)).items()) == [(name, shape) for name, shape, _ in rows]


@pytest.mark.parametrize("model,i", CASES)
def test_weights_fill_the_named_pointers_and_no_other(model, i):
    m, cfg, _, rows, packed = _case(model, i)
    tensors = {k: torch.from_numpy(v) for k, v in packed.items()}
    w = getattr(K, f"{model}_weights")(*m.args(cfg), tensors)
    named = {at: tensors[name].data_ptr() for name, _, at in rows}
    for at in _slots(m.Struct):
        assert C.c_void_p.from_address(C.addressof(w) + at).value == named.get(at), at
    assert w._device == torch.device("cpu") and set(w._tensors) == set(tensors)


@pytest.mark.parametrize("model,i", CASES)
def test_count_only_and_a_short_array(model, i):
    _, _, w, rows, _ = _case(model, i)
    lib, n = _lib.load(), C.c_int(-1)
    fn = getattr(lib, f"lmx_h_{model}_tensors")
    assert fn(b"who", C.byref(w), None, 0, C.byref(n)) == 0 and n.value == len(rows)
    short = (_lib.TensorRow * (len(rows) - 1))()
    assert fn(b"who", C.byref(w), short, len(rows) - 1, C.byref(n)) == EINVAL
    msg = lib.lmx_last_error().decode()
    assert msg.startswith("who: ") and f"cap {len(rows) - 1}" in msg and str(len(rows)) in msg, msg
    exact = (_lib.TensorRow * len(rows))()
    assert fn(b"who", C.byref(w), exact, len(rows), C.byref(n)) == 0 and n.value == len(rows)
    assert all(r.reserved == 0 and list(r.shape[r.rank:]) == [0] * (4 - r.rank) for r in exact)


@pytest.mark.parametrize("model", list(MODELS))
def test_a_configuration_outside_the_list_is_refused_with_who_and_the_field(model):
    m, cfg, good, _, _ = _case(model, 0)
    lib, n = _lib.load(), C.c_int(0)
    for field, value, text in m.bad:
        w = m.Struct.from_buffer_copy(bytes(good))
        if field == "channels":
            w.channels[0] = value
        else:
            setattr(w, field, value)
        assert getattr(lib, f"lmx_h_{model}_tensors")(b"the caller", C.byref(w), None, 0, C.byref(n)) == EINVAL
        msg = lib.lmx_last_error().decode()
        assert msg.startswith("the caller: ") and text in msg and n.value == 0, msg
        if field != "n_blocks":  # Python derives n_blocks from the channels
            args = list(m.args(cfg))
            if model == "tcn":
                args[{"input_dim": 0, "channels": 1, "k": 2, "head": 3}[field]] = (value,) + tuple(cfg.channels[1:]) if field == "channels" else value
            else:
                args[[f for f, _ in m.Struct._fields_].index(field)] = value
            with pytest.raises(K.LmxError) as e:  # the wrapper: its own `who` in front, the field named
                getattr(K, f"{model}_check_config")("the wrapper's caller", *args)
            assert str(e.value).startswith("the wrapper's caller: ") and text in str(e.value), str(e.value)


def test_python_refuses_what_an_int32_would_cut_before_any_call(monkeypatch):
    def called(*a):
        raise AssertionError("the library was asked")

    monkeypatch.setattr(K, "_model_rows", called)
    c = xfmref.SHIPPED
    with pytest.raises(K.LmxError, match="d_model 4294967360 is not an int32"):
        K.xfm_check_config("t", c.input_dim, 2 ** 32 + c.d_model, *c.shape()[2:])
    with pytest.raises(K.LmxError, match="ff -2147483649 is not an int32"):
        K.gfm_tensor_shapes(*gfmref.TINY.shape()[:4], -2 ** 31 - 1, *gfmref.TINY.shape()[5:])
    with pytest.raises(K.LmxError, match=r"channels 4294967312 is not an int32"):
        K.tcn_check_config("t", 44, (2 ** 32 + 16, 32), 3, 32)
    with pytest.raises(K.LmxError, match=r"t: n_blocks 9 outside 1 \.\. 8"):
        K.tcn_check_config("t", 44, (32,) * 9, 3, 32)
    with pytest.raises(K.LmxError, match=r"tcn_weights: n_blocks 9 outside 1 \.\. 8"):
        K.tcn_weights(44, (32,) * 9, 3, 32, {})
