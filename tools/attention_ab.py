"""Diagnostic (not part of the product): the forward of R mask rows of a GATConv model through
(a) the opt-in attention engine path (pipeline.build_plan(..., attention=True)) and (b)
pipeline.generic_outputs, the batched torch path that serves these models by default, on the
same card in one process.  Three shapes, each on the computational subgraph of one query node:

  multi   the 3-node-type / 5-relation random graph of the parity tests scaled to 30k / 20k /
          15k nodes, HeteroGATStack hidden 64, heads [2, 1]
  homog   a 50k-node / 500k-edge random graph, ConvStack("gat", [64, 64, 64], heads [2, 1])
  dense   the same model on a 3k-node / 60k-edge graph, whose 3-hop subgraph is most of the graph
          (the first two subgraphs are small: their times are mostly launch overheads)

Warm-up, then `--reps` alternating repetitions timed with device events (an engine repetition
is `--inner` back-to-back forwards, reported per forward); prints one JSON line
with the median and min / max of both paths, their ratio, the largest output difference, and the
attention kernels' requested bytes (computed from the plan arrays and the masks: every index,
keep-word, score and source-row load and every store of k_att_score / k_agg_att, no cache
reuse assumed) over the engine time.

    python tools/attention_ab.py [--rows 2048] [--reps 10] [--batch 256] [--scale 1.0]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from bikg_graph_explainability_public_amd import engine, pipeline  # noqa: E402
from bikg_graph_explainability_public_amd.nn import ConvStack, HeteroGATStack  # noqa: E402
from golden_utils import multi_type_setup  # noqa: E402

RELS = [("A", "ab", "B"), ("B", "ba", "A"), ("A", "aa", "A"), ("C", "ca", "A"), ("A", "ac", "C")]


def multi_case(scale, dev):
    sizes = {"A": int(30000 * scale), "B": int(20000 * scale), "C": int(15000 * scale)}
    dims = {"A": 24, "B": 16, "C": 40}
    g = torch.Generator().manual_seed(1)
    feat = {t: torch.randn(n, dims[t], generator=g).numpy() for t, n in sizes.items()}
    n_e = [int(m * 100 * scale) for m in (900, 700, 800, 400, 400)]
    ei = {r: torch.stack([torch.randint(0, sizes[r[0]], (m,), generator=g),
                          torch.randint(0, sizes[r[-1]], (m,), generator=g)]).numpy()
          for r, m in zip(RELS, n_e)}
    torch.manual_seed(3)
    arch = HeteroGATStack(RELS, dims, 64, [2, 1], [64, 16, 1]).eval().to(dev)
    names = {t: [f"{t.lower()}{i}" for i in range(n)] for t, n in sizes.items()}
    c = multi_type_setup(feat, ei, names, "b7", "B", 2,
                         {k: v.cpu().numpy() for k, v in arch.state_dict().items()}, [64, 16, 1],
                         conv="hetero_gat")
    x = torch.as_tensor(c["x"], dtype=torch.float32, device=dev)
    sub_ei = torch.as_tensor(c["ei"], device=dev)
    geo = (torch.as_tensor(c["nt"], device=dev), torch.as_tensor(c["et"], device=dev),
           c["ntypes"], c["rels"], c["pads"])
    return arch, x, sub_ei, c["sub_ind"], geo


def dense_case(scale, dev):
    return homog_case(scale, dev, 3000, 60000)


def homog_case(scale, dev, nodes=50000, edges=500000):
    n, e = int(nodes * scale), int(edges * scale)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((n, 64), generator=g)
    ei = torch.randint(0, n, (2, e), generator=g).numpy()
    torch.manual_seed(4)
    arch = ConvStack("gat", [64, 64, 64], [64, 1], heads=[2, 1]).eval().to(dev)
    subset, sub_ei, sub_ind, _ = oracle.comp_graph(11, 2, ei, n)
    return (arch, x[torch.as_tensor(subset)].to(dev), torch.as_tensor(sub_ei, device=dev),
            int(sub_ind), (None, None, None, None, None))


def requested_bytes(plan, mask):
    """Bytes k_att_score / k_agg_att ask for on this plan and these mask rows (host count)."""
    m = mask.cpu().numpy()
    fr, total = plan.frontiers, 0
    R = m.shape[0]
    for li, conv in enumerate(plan.program.convs):
        lay = plan.arrays["layers"][li]
        n_t = fr[li + 1].size
        low = plan.lowering[li]
        ptr = lay["agg_ptr"].reshape(plan.n_rel, n_t + 1)
        width = 4 * engine._rup(conv.f_out if li == 0 else plan.program.convs[li - 1].f_out, 32)
        on_t = m[:, fr[0][:n_t]]                                   # [R, n_t]
        slices = 0
        for term in [t for t in conv.terms if (t.kind, t.rel, t.dst_type) in low]:
            p = ptr[term.rel]
            tgt = np.repeat(np.arange(n_t), np.diff(p))
            src = lay["agg_f0"][p[0]:p[-1]]
            seen = int(on_t[:, tgt].sum())                          # edges walked (target kept)
            kept = int((on_t[:, tgt] & m[:, fr[0][src]]).sum())
            heads = term.heads
            slices += heads
            lanes = width // 16
            # per pass and head: index + node id + keep word per walked edge, a score per kept edge
            # (every lane of the item repeats the scalar loads); pass 2 adds the source-row chunk
            per_head = 2 * (seen * 12 + kept * 4) * lanes + kept * width
            total += per_head * (heads if li else 1)
        if li:
            n_prev = fr[li].size
            total += R * n_prev * (2 * slices) * (width + 4)        # k_att_score
            total += R * n_t * slices * width                       # GEMM-input stores
        else:
            total += R * n_t * width                                # layer-1 output stores
    return total


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
        raise SystemExit("attention_ab needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    warnings.simplefilter("ignore")
    res = {"rows": args.rows, "reps": args.reps, "engine_inner": args.inner,
           "generic_batch": args.batch}
    for name, build in (("multi", multi_case), ("homog", homog_case), ("dense", dense_case)):
        arch, x, ei, q, geo = build(args.scale, dev)
        plan = pipeline.build_plan(arch, x, ei, [q], *geo, attention=True)
        assert plan is not None, "the attention plan was rejected"
        S = x.shape[0]
        mask = torch.rand((args.rows, S), generator=torch.Generator().manual_seed(5)) < 0.5
        mask = mask.to(dev)
        bits = engine.pack_masks(mask)
        multi = geo[0] is not None

        def eng():
            return plan.forward(bits)[:, 0]

        def gen():
            return pipeline.generic_outputs(arch, x, ei, mask, q, "node", *geo, batch=args.batch,
                                            q4=not multi)
        te, tg = [], []
        ye = yg = None
        for i in range(args.reps):  # alternate the two paths (warm-up in the first round only)
            t, ye = timed(eng, 1, warm=3 if i == 0 else 0, inner=args.inner)
            te += t
            t, yg = timed(gen, 1, warm=2 if i == 0 else 0)
            tg += t
        if multi:
            ye = torch.where(pipeline.empty_copy_rows(bits, S, ei), torch.zeros_like(ye), ye)
        nbytes = requested_bytes(plan, mask)
        me, mg = statistics.median(te), statistics.median(tg)
        res[name] = {"S": int(S), "edges": int(ei.shape[1]), "n0": int(plan.n0),
                     "engine_ms": {"median": me, "min": min(te), "max": max(te)},
                     "generic_ms": {"median": mg, "min": min(tg), "max": max(tg)},
                     "generic_over_engine": mg / me,
                     "max_abs_diff": float((ye - yg).abs().max()),
                     "att_requested_bytes": int(nbytes),
                     "att_requested_GBps_over_engine_time": nbytes / (me * 1e-3) / 1e9}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
