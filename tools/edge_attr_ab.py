"""Diagnostic (not part of the product): the forward of R mask rows of models on graphs with edge
features (edge_attr for GINEConv) through (a) the engine (pipeline.build_plan(edge_attr=ea):
k_agg_e) and (b) pipeline.generic_outputs, the user's torch module on the batched union graph with
each kept edge's attribute row — the only other route such models have — on the same card in one
process.

  node models on the computational subgraph of one query node (the shapes of tools/weight_ab.py):
    homog   a 50k-node / 500k-edge random graph
    dense   a 3k-node / 60k-edge graph, whose 2-hop subgraph is most of the graph
      ConvStack("gine", [32, 64, 64], [64, 1], edge_dim=8)    attribute rows normal(0, 1)

R = 2,048 rows with P(bit) = 1/2.  Warm-up (3 calls), then `--reps` alternating repetitions timed
with device events (an engine repetition is `--inner` back-to-back forwards, reported per forward);
prints one JSON line with the median and min / max of both paths, their ratio, the path taken and the
largest |engine - generic| output difference.  Each shape is measured twice: layer 1 from the
plan's stored messages (k_agg_e<MSG>, the default) and in the two-row form (XPG_EFEAT_MSG=0, which
the library reads at every forward).

    python tools/edge_attr_ab.py [--rows 2048] [--reps 10] [--batch 256] [--scale 1.0]
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle  # noqa: E402
from post_ab import NODE_SHAPES, ab  # noqa: E402
from bikg_graph_explainability_public_amd import engine, pipeline  # noqa: E402
from bikg_graph_explainability_public_amd.nn import ConvStack  # noqa: E402

EDGE_DIM = 8


def scale_mlps(arch, s):
    with torch.no_grad():  # sums over many in-edges: keep the sigmoid off its tails
        for name, p in arch.named_parameters():
            if ".nn." in name and name.endswith("weight") and p.dim() == 2:
                p.mul_(s)


def node_case(scale, dev, nodes, edges):
    n, e = int(nodes * scale), int(edges * scale)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((n, 32), generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    ea = torch.randn((e, EDGE_DIM), generator=g)
    torch.manual_seed(4)
    arch = ConvStack("gine", [32, 64, 64], [64, 1], edge_dim=EDGE_DIM).eval()
    scale_mlps(arch, 0.25)
    subset, sub_ei, sub_ind, emask = oracle.comp_graph(11, 2, ei.numpy(), n)
    return (arch.to(dev), x[torch.as_tensor(subset)].to(dev), torch.as_tensor(sub_ei, device=dev),
            ea[torch.as_tensor(emask)].to(dev), int(sub_ind))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="engine forwards per timed repetition")
    ap.add_argument("--batch", type=int, default=256, help="mask rows per generic-path arch call")
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_attr_ab needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    warnings.simplefilter("ignore")
    res = {"rows": args.rows, "reps": args.reps, "engine_inner": args.inner,
           "generic_batch": args.batch}
    for shape, (nodes, edges) in NODE_SHAPES.items():
        arch, x, ei, ea, q = node_case(args.scale, dev, nodes, edges)
        plan = pipeline.build_plan(arch, x, ei, [q], edge_attr=ea)
        assert plan is not None and "efeat=k_agg_e" in plan.describe(args.rows)
        mask = (torch.rand((args.rows, x.shape[0]), generator=torch.Generator().manual_seed(5)) < 0.5).to(dev)
        bits = engine.pack_masks(mask)
        for msg in ("1", "0"):
            os.environ["XPG_EFEAT_MSG"] = msg
            r = ab(args, plan, lambda: plan.forward(bits)[:, 0],
                   lambda: pipeline.generic_outputs(arch, x, ei, mask, q, "node", batch=args.batch,
                                                    edge_attr=ea))
            res[f"{shape}/gine/msg={msg}"] = dict(r, S=int(x.shape[0]), edges=int(ei.shape[1]))
        os.environ.pop("XPG_EFEAT_MSG", None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
