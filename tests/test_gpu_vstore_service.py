"""DINOv3Pipeline.process_videos over a DeviceVectorStore: a backlog answered by one search launch and one batched append writes the
files and sends the messages of one process_video call per clip; a batch with a repeated id takes the sequential route; a saved store
comes back with the same bytes."""
import asyncio

import numpy as np
import pytest
import torch

from lmx import services, vstore
from lmx.services import runtime as R

pytestmark = pytest.mark.gpu

D = 260


class ClipEmbedder:
    """frame -> a fixed pseudo-random embedding picked by the frame's first byte (the clip's signature)"""
    device = torch.device("cpu")

    class cfg:
        hidden = D

    table = torch.from_numpy(np.random.default_rng(31).standard_normal((256, D)).astype(np.float32))

    def embed_frames(self, frames):
        return self.table[frames[:, 0, 0, 0].long()] + 0.01 * self.table[frames[:, 0, 0, 1].long()]


def _clip(tmp_path, name, signature, n=3):
    frames = np.zeros((n, 16, 16, 3), np.uint8)
    frames[:, 0, 0, 0] = signature
    frames[:, 0, 0, 1] = np.arange(n)
    p = tmp_path / f"{name}.npz"
    R.save_npz_clip(p, frames, 1)
    return p


def _service(cuda, tmp_path, tag):
    store = vstore.DeviceVectorStore(cuda, capacity=4)
    bus = R.InProcessBus()
    svc = services.DINOv3Pipeline(ClipEmbedder(), bus, store, {"nats": {"subjects": dict(R.DEFAULT_SUBJECTS)}}, results_dir=tmp_path / tag)
    rng = np.random.default_rng(32)
    for i in range(7):  # history: noisy copies of the signatures the backlog will bring, labelled
        store.upsert(f"old{i}", (ClipEmbedder.table[i % 4].numpy() + 0.3 * rng.standard_normal(D)).tolist(),
                     {"video_id": f"old{i}", "label": i % 2, "metadata": {"n": i}})
    return svc, store, bus


def _files(tmp_path, tag):
    return {p.name: p.read_bytes() for p in sorted((tmp_path / tag).iterdir())}


@pytest.mark.parametrize("ids", [["a", "b", "c", "d", "e", "f"], ["a", "b", "a", "d", "old3", "f"]], ids=["new", "repeated"])
def test_process_videos_equals_sequential_process_video(cuda, tmp_path, ids):
    # signatures 1, 2, 1, ...: later clips of the backlog find earlier ones
    msgs = [{"video_id": vid, "processed_path": str(_clip(tmp_path, f"clip{j}", 1 + j % 2)), "filename": f"{vid}.mp4", "metadata": {"j": j}}
            for j, vid in enumerate(ids)]
    seq, seq_store, seq_bus = _service(cuda, tmp_path, "seq")
    for m in msgs:
        asyncio.run(seq.process_video(m))
    bat, bat_store, bat_bus = _service(cuda, tmp_path, "bat")
    calls = []
    inner = bat_store.search_then_append
    bat_store.search_then_append = lambda *a, **k: (calls.append(len(a[0])), inner(*a, **k))[1]
    asyncio.run(bat.process_videos(msgs))
    assert calls == ([6] if len(set(ids)) == 6 and "old3" not in ids else [])  # one batched call, or the sequential route
    a, b = _files(tmp_path, "seq"), _files(tmp_path, "bat")
    assert list(a) == list(b) and len(a) == len(set(ids)) and a == b
    strip = lambda pub: [(s, {k: (v.replace("/bat/", "/seq/") if k == "results_path" else v) for k, v in m.items()}) for s, m in pub]  # noqa: E731
    assert strip(bat_bus.published) == strip(seq_bus.published) and len(seq_bus.published) == 6
    assert bat_store.ids == seq_store.ids and bat_store.payloads == seq_store.payloads
    assert all(np.array_equal(bat_store.vector(s), seq_store.vector(s)) for s in range(seq_store.count()))


def test_save_and_load_answer_with_the_same_bytes(cuda, tmp_path):
    _, store, _ = _service(cuda, tmp_path, "s")
    rng = np.random.default_rng(33)
    queries = rng.standard_normal((5, D))
    before = store.search_slots(queries, 5)
    store.save(tmp_path / "saved")
    back = vstore.DeviceVectorStore.load(tmp_path / "saved", cuda)
    after = back.search_slots(queries, 5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert back.ids == store.ids and back.payloads == store.payloads and back.search(queries[0]) == store.search(queries[0])
    assert back.search_many(queries, 5) == [store.search(q) for q in queries]
    back.upsert("new", queries[0].tolist(), {"video_id": "new"})
    assert back.count() == store.count() + 1 and back.search(queries[0], 1)[0]["video_id"] == "new"
