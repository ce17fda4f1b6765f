"""Records tests/golden/graphgps_small_w7.npz from the REFERENCE's own EnhancedGraphGPS and GraphBuilder (services/gnn-pipeline/app/main.py),
for the machines that have no checkout of the reference: a reduced configuration (input 50, hidden 32, 2 heads, num_layers 4, pe 8), its
whole state_dict (biases and BatchNorm's running statistics randomised: the reference initialises them to nothing; the dead post-pool
half included), three graphs' inputs (features, embeddings, timestamps; one with N <= 9), what the reference's builder made of them
(edge_index, edge_attr), the raw lap_pe and rw_pe the reference computed in that forward, and its eval-mode outputs in float32:
graph_pred, node_pred and attention_weights.  Needs the checkout (tests/gnnref.reference_main), scipy and yaml.

    python tests/golden/make_golden_graphgps.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import gnnref  # noqa: E402


def main():
    ref = gnnref.reference_module()
    assert ref is not None, "no checkout of the reference, or no scipy / yaml"
    cfg = gnnref.GOLDEN_CFG
    torch.manual_seed(7)
    np.random.seed(7)  # eigsh draws its start vector from numpy's generator
    net = gnnref.reference_net(ref, cfg).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.rand_like(p) - 0.5)
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.rand_like(b) - 0.5)
            elif name.endswith("running_var"):
                b.copy_(0.5 + 1.5 * torch.rand_like(b))
    out = {"sd/" + k: v.numpy() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    for i, (N, timed) in enumerate(gnnref.GOLDEN_SIZES):
        x, emb = torch.randn((N, cfg.input_dim), generator=g).numpy(), torch.randn((N, 16), generator=g).numpy()
        # distinct (argsort has no ties) and NOT float32 numbers: the reference keeps Python floats, and so does the library
        ts = (1.7e9 + torch.randperm(N, generator=g).double() * 60123.4567).numpy() if timed else None
        data = gnnref.reference_graph(ref, x, emb, ts)
        res, lap, rw = gnnref.reference_forward(net, data)
        p = f"g{i}/"
        out.update({p + "x": x, p + "emb": emb, p + "edge_index": data.edge_index.numpy(), p + "edge_attr": data.edge_attr.numpy(), p + "lap": lap,
                    p + "rw": rw, p + "graph_pred": res["graph_pred"].reshape(()).numpy(), p + "node_pred": res["node_pred"][:, 0].numpy(),
                    p + "attw": res["attention_weights"][:, 0].numpy()})
        if timed:
            out[p + "ts"] = ts
    np.savez_compressed(gnnref.GOLDEN, **out)
    print(gnnref.GOLDEN, os.path.getsize(gnnref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
