"""Diagnostic (not part of the product): the forward of R mask rows of a 2-layer RGCN model on a
typed-edge graph through (a) the engine (pipeline.build_plan: XPG_TERM_REL, per-relation layer-1
tables, relation / basis slices at layer 2) and (b) pipeline.generic_outputs, the batched torch
path that served these models before (the 4-argument call of the module on the union graph), on
the same card in one process.  The shapes of tools/aggr_ab.py, each on the computational subgraph
of one query node, with uniformly random edge types:

  homog/8-plain     a 50k-node / 500k-edge random graph, hidden 64, 8 edge types, plain weights
  homog/64-bases8   the same graph with 64 edge types and 8 bases
  dense/64-bases8   a 3k-node / 60k-edge graph (its 2-hop subgraph is most of the graph), 64 edge
                    types and 8 bases

Warm-up (3 calls), then `--reps` alternating repetitions timed with device events (an engine
repetition is `--inner` back-to-back forwards, reported per forward); prints one JSON line with
the median and min / max of both paths, their ratio, the path taken and the largest output
difference.

    python tools/rgcn_ab.py [--rows 2048] [--reps 10] [--batch 256] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from bikg_graph_explainability_public_amd import engine, pipeline  # noqa: E402
from bikg_graph_explainability_public_amd.nn import RGCNStack  # noqa: E402

SHAPES = {"homog": (50000, 500000), "dense": (3000, 60000)}
CASES = [("homog", "8-plain", 8, None), ("homog", "64-bases8", 64, 8), ("dense", "64-bases8", 64, 8)]


def case(n_rel, bases, scale, dev, nodes, edges):
    n, e = int(nodes * scale), int(edges * scale)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((n, 64), generator=g)
    ei = torch.randint(0, n, (2, e), generator=g).numpy()
    et = torch.randint(0, n_rel, (e,), generator=g).numpy()
    torch.manual_seed(4)
    arch = RGCNStack([64, 64, 64], [64, 1], n_rel, num_bases=bases).eval()
    with torch.no_grad():  # keep the sigmoid off its tails
        for name, p in arch.conv.named_parameters():
            if name.endswith("weight") or name.endswith("root"):
                p.mul_(0.25)
    subset, sub_ei, sub_ind, emask = oracle.comp_graph(11, 2, ei, n)
    sub_et = et[np.asarray(emask, dtype=bool)]
    assert sub_et.shape[0] == np.asarray(sub_ei).shape[1]
    return (arch.to(dev), x[torch.as_tensor(subset)].to(dev), torch.as_tensor(sub_ei, device=dev),
            torch.as_tensor(sub_et, device=dev), int(sub_ind))


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
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgcn_ab needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    warnings.simplefilter("ignore")
    res = {"rows": args.rows, "reps": args.reps, "engine_inner": args.inner,
           "generic_batch": args.batch}
    for shape, label, n_rel, bases in CASES:
        nodes, edges = SHAPES[shape]
        arch, x, ei, et, q = case(n_rel, bases, args.scale, dev, nodes, edges)
        S = x.shape[0]
        nt = torch.ones(S, dtype=torch.long, device=dev)
        plan = pipeline.build_plan(arch, x, ei, [q], nt, et)
        assert plan is not None, "the plan was rejected"
        assert any(k == "rel" for low in plan.lowering for k, _, _ in low) and plan.n_rel == n_rel
        mask = torch.rand((args.rows, S), generator=torch.Generator().manual_seed(5)) < 0.5
        mask = mask.to(dev)
        bits = engine.pack_masks(mask)

        def eng():
            return plan.forward(bits)[:, 0]

        def gen():
            return pipeline.generic_outputs(arch, x, ei, mask, q, "node", nt, et, batch=args.batch)
        te, tg = [], []
        ye = yg = None
        for i in range(args.reps):  # alternate the two paths (warm-up in the first round only)
            t, ye = timed(eng, 1, warm=3 if i == 0 else 0, inner=args.inner)
            te += t
            t, yg = timed(gen, 1, warm=3 if i == 0 else 0)
            tg += t
        me, mg = statistics.median(te), statistics.median(tg)
        res[f"{shape}/{label}"] = {
            "S": int(S), "edges": int(ei.shape[1]), "n0": int(plan.n0),
            "path": plan.describe(args.rows),
            "engine_ms": {"median": me, "min": min(te), "max": max(te)},
            "generic_ms": {"median": mg, "min": min(tg), "max": max(tg)},
            "generic_over_engine": mg / me,
            "max_abs_diff": float((ye - yg).abs().max())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
