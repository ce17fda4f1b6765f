"""Records tests/golden/graphormer_small_w5.npz from the REFERENCE's own CowLamenessGraphormer and GraphormerGraphBuilder
(services/graph-transformer-pipeline/app/model), for the machines that have no checkout of the reference: a reduced configuration
(input 50, hidden 32, 2 heads, 2 layers, FFN 64), its state_dict (biases, spd_bias and virtual nodes randomised: the reference
initialises them to nothing), three graphs' inputs (features, embeddings, timestamps), what the reference's builder made of them
(edge_index, edge_attr) and the reference's eval-mode outputs in float32: graph_pred, node_pred and the target's column of the head
average of the last layer's attention.  Needs the checkout (tests/gfmref.reference_app) and networkx.

    python tests/golden/make_golden_graphormer.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import gfmref  # noqa: E402


def main():
    ref = gfmref.reference_modules()
    assert ref is not None, "no checkout of the reference, or no networkx"
    cfg = gfmref.GOLDEN_CFG
    torch.manual_seed(5)
    net = ref.CowLamenessGraphormer(input_dim=cfg.input_dim, hidden_dim=cfg.d_model, num_layers=cfg.n_layers, num_heads=cfg.n_heads,
                                    ffn_dim=cfg.ff).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias") or "spd_bias" in name or "virtual_node" in name:
                p.copy_(torch.rand_like(p) - 0.5)
    out = {"sd/" + k: v.numpy() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    for i, (N, timed) in enumerate(gfmref.GOLDEN_SIZES):
        x, emb = torch.randn((N, cfg.input_dim), generator=g), torch.randn((N, 16), generator=g)
        ts = (1.7e9 + torch.randperm(N, generator=g).float() * 86400.0 * 0.7) if timed else None  # distinct: argsort has no ties
        data = ref.GraphormerGraphBuilder(gfmref.K_NEIGHBOURS).build_graph(x, emb, ts)
        target = N // 2
        with torch.no_grad():
            res = net(data, return_attention=True)
        p = f"g{i}/"
        out.update({p + "x": x.numpy(), p + "emb": emb.numpy(), p + "edge_index": data.edge_index.numpy(), p + "edge_attr": data.edge_attr.numpy(),
                    p + "target": np.int64(target), p + "graph_pred": res["graph_pred"].reshape(()).numpy(), p + "node_pred": res["node_pred"][:, 0].numpy(),
                    p + "attn": res["attention_weights"][-1].mean(0)[:, target].numpy()})
        if timed:
            out[p + "ts"] = ts.numpy()
    np.savez_compressed(gfmref.GOLDEN, **out)
    print(gfmref.GOLDEN, os.path.getsize(gfmref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
