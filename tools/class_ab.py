"""Diagnostic (not part of the product): what an all-class explanation of a 7-class node classifier
costs, on the same card in one process (the method of tools/edge_attr_ab.py).

  forward of R mask rows of ConvStack("gcn", [64, 64, 64], [64, 7], final_act="softmax") on the
  computational subgraph of one query node (the shapes of tools/post_ab.py):
    homog   a 50k-node / 500k-edge random graph
    dense   a 3k-node / 60k-edge graph, whose 2-hop subgraph is most of the graph
  (a) the engine with classes="all" (k_class_out<softmax,all> after the unfused tail) against
  (b) pipeline.generic_outputs(classes="all"), the user's torch module on the batched union graph;
  beside them the same plan's forward of ONE logit column (out_col = 3, no softmax: the column
  pick fused into k_dense's HEAD epilogue), which shows what the unfused tail and the readout cost.

  Explainer.run_classes over the 7 classes against 7 separate Explainer.run calls (target_class =
  0..6) of the same query, wall-clock with a device synchronisation (both include their host work).

R = 2,048 rows with P(bit) = 1/2.  Warm-up (3 calls), then `--reps` alternating repetitions timed
with device events (an engine repetition is `--inner` back-to-back forwards, reported per forward);
prints one JSON line with the median and min / max of every path.

    python tools/class_ab.py [--rows 2048] [--reps 10] [--batch 256] [--scale 1.0]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle  # noqa: E402
from post_ab import NODE_SHAPES, ab, timed  # noqa: E402
from bikg_graph_explainability_public_amd import engine, pipeline  # noqa: E402
from bikg_graph_explainability_public_amd.explainer import Explainer  # noqa: E402
from bikg_graph_explainability_public_amd.nn import ConvStack  # noqa: E402

C = 7


def graph(scale, nodes, edges):
    n, e = int(nodes * scale), int(edges * scale)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((n, 64), generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    torch.manual_seed(4)
    arch = ConvStack("gcn", [64, 64, 64], [64, C], final_act="softmax").eval()
    return arch, x, ei


def node_case(scale, dev, nodes, edges):
    arch, x, ei = graph(scale, nodes, edges)
    subset, sub_ei, sub_ind, _ = oracle.comp_graph(11, 2, ei.numpy(), x.shape[0])
    return arch.to(dev), x[torch.as_tensor(subset)].to(dev), torch.as_tensor(sub_ei, device=dev), int(sub_ind)


def wall(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="engine forwards per timed repetition")
    ap.add_argument("--batch", type=int, default=256, help="mask rows per generic-path arch call")
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("class_ab needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    warnings.simplefilter("ignore")
    res = {"rows": args.rows, "reps": args.reps, "engine_inner": args.inner,
           "generic_batch": args.batch, "classes": C}
    for shape, (nodes, edges) in NODE_SHAPES.items():
        arch, x, ei, q = node_case(args.scale, dev, nodes, edges)
        plan = pipeline.build_plan(arch, x, ei, [q], classes="all")
        assert plan is not None and plan.describe(args.rows).endswith("class=k_class_out<softmax,all>")
        mask = (torch.rand((args.rows, x.shape[0]), generator=torch.Generator().manual_seed(5)) < 0.5).to(dev)
        bits = engine.pack_masks(mask)
        r = ab(args, plan, lambda: plan.forward(bits),
               lambda: pipeline.generic_outputs(arch, x, ei, mask, q, "node", batch=args.batch, classes="all"))
        # one logit column of the same model without its softmax: the fused HEAD tail
        logits = copy.deepcopy(arch)
        logits.fc[-1] = torch.nn.Identity()
        one = pipeline.build_plan(logits, x, ei, [q], out_col=3)
        assert one is not None and "class=" not in one.describe(args.rows)
        t1 = []
        for i in range(args.reps):
            t1 += timed(lambda: one.forward(bits), 1, warm=3 if i == 0 else 0, inner=args.inner)[0]
        res[f"{shape}/forward"] = dict(r, S=int(x.shape[0]), edges=int(ei.shape[1]),
                                       one_logit_column_ms=stats(t1), one_logit_column_path=one.describe(args.rows))
    # run_classes over the 7 classes against 7 run calls (the dense graph; node_prediction)
    arch, x, ei = graph(args.scale, *NODE_SHAPES["dense"])
    base = {"seed": 1, "interpret_samples": args.rows // 8, "epochs": 8, "optimizer": "adam", "lr": 0.01,
            "lr_patience": 10, "l1_lambda": 1e-4, "mask_sampler": "device"}
    names = [str(i) for i in range(x.shape[0])]
    exp = Explainer(x.to(dev), ei.to(dev), arch.to(dev), dict(base), names)

    def seven_runs():
        for c in range(C):
            exp.params["target_class"] = c
            exp.run("11", 1)
    ta, tb = [], []
    for i in range(args.reps):  # alternate (warm-up in the first round only: plans, programs, checks)
        ta += wall(lambda: exp.run_classes("11", None, 1), 1, 1 if i == 0 else 0)
        tb += wall(seven_runs, 1, 1 if i == 0 else 0)
    res["dense/explain"] = {"run_classes_ms": stats(ta), "seven_runs_ms": stats(tb),
                            "seven_runs_over_run_classes": statistics.median(tb) / statistics.median(ta),
                            "S": int(exp.last_run["S"]), "rows": args.rows}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
