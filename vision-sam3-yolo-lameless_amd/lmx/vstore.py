"""The vector store on the device: cosine top-k over a gallery of unit rows in HBM (include/lmx.h "Vector store").

``DeviceVectorStore`` stands where ``lmx.services.runtime.MemoryVectorStore`` stands under ``DINOv3Pipeline`` and
``DeviceIdentityStore`` where ``lmx.services.tracking.MemoryIdentityStore`` stands under ``CowReIDMatcher``: the slice of Qdrant the
two services use.  Both are one core: the C handle ``lmx_vstore`` (which maps nothing but slots) plus a host table from point id to
slot and payload.  Vectors are normalised once, on the way in, by the pinned ``unit_rows``; a search is one ``lmx_k_cosine_topk``.
Parity with Qdrant itself is rank parity outside near-ties, not bits ("Vector store")."""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import LmxError, check

MAX_K = 32
_NP_DT = {np.dtype(np.float32): 1, np.dtype(np.float64): 2}  # LMX_VSTORE_F32, LMX_VSTORE_F64


def geometry(dim):
    """(R, T, workgroups per CU) of the scan kernel at dimension `dim`: rows per workgroup pass, queries per tile.  Stated once, in
    csrc/vstore.h; for tests that must reach every branch.  None of them can show in a result."""
    r, t, w = C.c_int(), C.c_int(), C.c_int()
    check(_lib.load().lmx_h_cosine_topk_geometry(dim, C.byref(r), C.byref(t), C.byref(w)), "lmx_h_cosine_topk_geometry")
    return r.value, t.value, w.value


def _raw(a, dim, what):
    """numpy f32 / f64 [n, dim], contiguous (anything else becomes float64, as the in-memory stores take it)"""
    a = np.asarray(a)
    if a.dtype not in _NP_DT:
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a.reshape(-1, dim) if a.ndim == 1 else a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise LmxError(f"{what}: vectors of {a.shape[-1]} elements in a collection of {dim}")
    return a


class DeviceStore:
    """Point ids, payloads and an ``lmx_vstore`` handle.  Upsert by an existing id replaces that slot in place."""

    def __init__(self, device="cuda:0", capacity=1024):
        self.device = torch.device(device)
        self.capacity = capacity
        self.dim = None
        self._h = None
        self.ids, self.payloads, self.slot_of = [], [], {}

    # ---- the handle
    def ensure_collection(self, dim):
        if self._h is not None:
            if dim != self.dim:
                raise LmxError(f"the collection holds vectors of {self.dim} elements, not {dim}")
            return
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(_lib.load().lmx_vstore_open(dim, self.capacity, C.byref(h)), "lmx_vstore_open")
        self._h, self.dim = h, dim

    def close(self):
        if self._h is not None:
            _lib.load().lmx_vstore_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass

    def _handle(self):
        if self._h is None:
            raise LmxError("the collection does not exist yet: call ensure_collection(dim)")
        return self._h

    def count(self):
        return len(self.ids)

    # ---- rows in
    def upsert(self, pid, vector, payload):
        h = self._handle()
        v = _raw(vector, self.dim, "upsert")
        slot = self.slot_of.get(pid, len(self.ids))
        with torch.cuda.device(self.device):
            check(_lib.load().lmx_vstore_put_host(h, slot, v.ctypes.data_as(C.c_void_p), _NP_DT[v.dtype]), "lmx_vstore_put_host")
        if slot == len(self.ids):
            self.ids.append(pid)
            self.payloads.append(dict(payload))
            self.slot_of[pid] = slot
        else:
            self.payloads[slot] = dict(payload)

    def append_many(self, pids, vectors, payloads):
        """One batched append of points whose ids are all new: the rows are normalised on the device."""
        h = self._handle()
        pids = list(pids)
        if len(set(pids)) != len(pids) or any(p in self.slot_of for p in pids):
            raise LmxError("append_many takes ids that are new to the store and distinct; upsert replaces")
        v = torch.from_numpy(_raw(vectors, self.dim, "append_many")).to(self.device)
        if v.shape[0] != len(pids):
            raise LmxError(f"append_many: {v.shape[0]} vectors for {len(pids)} ids")
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            check(_lib.load().lmx_vstore_append(h, C.c_void_p(v.data_ptr()), 1 if v.dtype == torch.float32 else 2, len(pids)), "lmx_vstore_append")
        for pid, payload in zip(pids, payloads):
            self.slot_of[pid] = len(self.ids)
            self.ids.append(pid)
            self.payloads.append(dict(payload))

    def vector(self, slot):
        """the stored f32 unit row"""
        out = np.empty((self.dim,), np.float32)
        with torch.cuda.device(self.device):
            check(_lib.load().lmx_vstore_get_host(self._handle(), slot, out.ctypes.data_as(C.c_void_p)), "lmx_vstore_get_host")
        return out

    # ---- searches
    def search_slots(self, queries, top_k, limits=None):
        """queries [Q, dim] (or one vector) -> (scores f32 [Q, k], slots int32 [Q, k]) in host memory; slot -1 / score 0 past the visible
        rows.  limits: None, or per query the number of leading slots it sees (lmx_k_cosine_topk)."""
        h = self._handle()
        q = _raw(queries, self.dim, "search")
        Q = q.shape[0]
        scores, slots = np.zeros((Q, top_k), np.float32), np.full((Q, top_k), -1, np.int32)
        lim = None
        if limits is not None:
            lim = np.ascontiguousarray(limits, np.int32)
            if lim.shape != (Q,):
                raise LmxError(f"search: {lim.shape} limits for {Q} queries")
        with torch.cuda.device(self.device):
            check(_lib.load().lmx_vstore_search_host(h, q.ctypes.data_as(C.c_void_p), _NP_DT[q.dtype], Q,
                                                     lim.ctypes.data_as(C.c_void_p) if lim is not None else None, top_k,
                                                     scores.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p)), "lmx_vstore_search_host")
        return scores, slots

    def hits(self, scores, slots, payloads=None):
        """[(slot, score, payload)] per query, padding dropped"""
        payloads = self.payloads if payloads is None else payloads
        return [[(int(s), float(sc), payloads[int(s)]) for sc, s in zip(scs, sls) if s >= 0] for scs, sls in zip(scores, slots)]

    # ---- a store on disk: the unit rows as they stand, the ids and the payloads
    def save(self, directory):
        os.makedirs(directory, exist_ok=True)
        rows = np.empty((len(self.ids), self.dim), np.float32)
        with torch.cuda.device(self.device):
            check(_lib.load().lmx_vstore_read_host(self._handle(), 0, len(self.ids), rows.ctypes.data_as(C.c_void_p)), "lmx_vstore_read_host")
        np.save(os.path.join(directory, "vectors.npy"), rows)
        with open(os.path.join(directory, "payloads.json"), "w") as f:
            json.dump({"dim": self.dim, "ids": self.ids, "payloads": self.payloads}, f)

    @classmethod
    def load(cls, directory, device="cuda:0"):
        rows = np.ascontiguousarray(np.load(os.path.join(directory, "vectors.npy")), np.float32)
        with open(os.path.join(directory, "payloads.json")) as f:
            meta = json.load(f)
        if rows.shape != (len(meta["ids"]), meta["dim"]):
            raise LmxError(f"{directory}: vectors.npy is {rows.shape}, payloads.json lists {len(meta['ids'])} ids of {meta['dim']} elements")
        store = cls(device, capacity=max(1024, len(rows)))
        store.ensure_collection(meta["dim"])
        with torch.cuda.device(store.device):
            check(_lib.load().lmx_vstore_restore_host(store._h, rows.ctypes.data_as(C.c_void_p), len(rows)), "lmx_vstore_restore_host")
        store.ids, store.payloads = list(meta["ids"]), list(meta["payloads"])
        store.slot_of = {pid: i for i, pid in enumerate(store.ids)}
        return store


def _hit(score, payload):
    return {"video_id": payload.get("video_id", "unknown"), "score": score, "label": payload.get("label", None),
            "metadata": payload.get("metadata", {})}


class DeviceVectorStore(DeviceStore):
    """``MemoryVectorStore``'s three calls (ensure_collection, search, upsert) and the dict it returns per hit, plus the batched calls."""

    def search(self, vector, top_k=5):
        if not self.ids:
            return []
        return [_hit(sc, p) for _, sc, p in self.hits(*self.search_slots(vector, top_k))[0]]

    def search_many(self, queries, top_k=5, limits=None):
        """one launch for all the queries -> a list of hits per query"""
        if len(queries) == 0:
            return []
        return [[_hit(sc, p) for _, sc, p in row] for row in self.hits(*self.search_slots(queries, top_k, limits))]

    def search_then_append(self, pids, vectors, payloads, top_k=5):
        """What len(pids) search-then-upsert steps return and leave behind, for ids new to the store: ONE search in which query j sees
        the stored rows and the j rows in front of it, then ONE batched append."""
        if len(set(pids)) != len(pids) or any(p in self.slot_of for p in pids):
            raise LmxError("search_then_append takes ids that are new to the store and distinct")
        vectors = _raw(vectors, self.dim, "search_then_append")
        n0 = len(self.ids)
        self.append_many(pids, vectors, payloads)
        scores, slots = self.search_slots(vectors, top_k, limits=n0 + np.arange(len(pids)))
        return [[_hit(sc, p) for _, sc, p in row] for row in self.hits(scores, slots)]


class DeviceIdentityStore(DeviceStore):
    """``MemoryIdentityStore``'s five calls (ensure_collection, count, query, retrieve, upsert) under ``CowReIDMatcher``."""

    def query(self, vector, top_k=5):
        if not self.ids:
            return []
        return [(self.ids[s], sc, p) for s, sc, p in self.hits(*self.search_slots(vector, top_k))[0]]

    def retrieve(self, pid):
        slot = self.slot_of.get(pid)
        return None if slot is None else (self.vector(slot).astype(np.float64), self.payloads[slot])
