"""Diagnostic (not part of the product): the forward of R mask rows of a graph-level model,
PooledModel(ConvStack("gin" | "gcn", [64, 64, 64], [64]), "add" | "mean", [64, 1]), through (a) the
engine (pipeline.build_plan: every node a target of the last layer, the readout kernels k_pool /
k_pool_finish, the head on one row per mask row) and (b) pipeline.generic_outputs, the user's torch
module on the batched union graph with a batch vector, on the same card in one process.  Two graphs:

  molecule   30 nodes / 64 edges
  medium     500 nodes / 2,000 edges

R = 2,048 rows with P(bit) = 1/2.  Warm-up (3 calls), then `--reps` alternating repetitions timed
with device events (an engine repetition is `--inner` back-to-back forwards, reported per forward);
prints one JSON line with the median and min / max of both paths, their ratio, the path taken, the
readout's kernels and the largest |engine - generic| output difference.

    python tools/pool_ab.py [--rows 2048] [--reps 10] [--batch 256]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bikg_graph_explainability_public_amd import engine, pipeline  # noqa: E402
from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel  # noqa: E402

SHAPES = {"molecule": (30, 64), "medium": (500, 2000)}
MODELS = [("gin", "add"), ("gin", "mean"), ("gcn", "add"), ("gcn", "mean")]


def case(kind, pool, dev, nodes, edges):
    g = torch.Generator().manual_seed(2)
    x = torch.randn((nodes, 64), generator=g)
    ei = torch.randint(0, nodes, (2, edges), generator=g)
    torch.manual_seed(4)
    arch = PooledModel(ConvStack(kind, [64, 64, 64], [64]), pool, [64, 1]).eval()
    with torch.no_grad():  # sums over the graph's nodes: keep the sigmoid off its tails
        for name, p in arch.encoder.named_parameters():
            if name.endswith("weight"):
                p.mul_(0.25)
        if pool == "add":
            arch.fc[0].weight.mul_(1.0 / nodes)
    return arch.to(dev), x.to(dev), ei.to(dev)


def timed(fn, reps, warm=3, inner=1):
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="engine forwards per timed repetition")
    ap.add_argument("--batch", type=int, default=256, help="mask rows per generic-path arch call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_ab needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    warnings.simplefilter("ignore")
    res = {"rows": args.rows, "reps": args.reps, "engine_inner": args.inner,
           "generic_batch": args.batch}
    for shape, (nodes, edges) in SHAPES.items():
        for kind, pool in MODELS:
            arch, x, ei = case(kind, pool, dev, nodes, edges)
            plan = pipeline.build_plan(arch, x, ei, [0])
            assert plan is not None and plan.pool is not None, "the plan was rejected"
            mask = torch.rand((args.rows, nodes), generator=torch.Generator().manual_seed(5)) < 0.5
            mask = mask.to(dev)
            bits = engine.pack_masks(mask)

            def eng():
                return plan.forward(bits)[:, 0]

            def gen():
                return pipeline.generic_outputs(arch, x, ei, mask, 0, "graph_prediction",
                                                batch=args.batch)
            te, tg = [], []
            ye = yg = None
            for i in range(args.reps):  # alternate the two paths (warm-up in the first round only)
                t, ye = timed(eng, 1, warm=3 if i == 0 else 0, inner=args.inner)
                te += t
                t, yg = timed(gen, 1, warm=3 if i == 0 else 0)
                tg += t
            me, mg = statistics.median(te), statistics.median(tg)
            last = plan._layers[len(plan._layers) - 1]
            res[f"{shape}/{kind}-{pool}"] = {
                "S": nodes, "edges": edges, "path": plan.describe(args.rows),
                "readout": engine.pool_describe(args.rows, nodes, last.f_out_pad, plan.pool),
                "engine_ms": {"median": me, "min": min(te), "max": max(te)},
                "generic_ms": {"median": mg, "min": min(tg), "max": max(tg)},
                "generic_over_engine": mg / me,
                "y_std": float(ye.std()),
                "max_abs_diff": float((ye - yg).abs().max())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
