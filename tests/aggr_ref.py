"""fp64 numpy restatement of the sum / max / mean message-passing families (SAGEConv add / max,
GraphConv, GINConv, HeteroConv-sum over them) on the reference's B-fold union graph, for
tests/test_aggr_cpu.py and tests/test_gpu_aggr.py.  It reads a module's state dict and attributes
only (never its forward): per layer and relation the aggregate with an explicit 0 fill for targets
without edges, then the linear maps."""
import numpy as np

import oracle


def aggregate(xs, src, dst, n, kind):
    """[n, F] fp64: per target the sum / mean / max of xs[src] over its in-edges (duplicates are
    separate entries); a target without edges gets 0 (also for max, where a non-empty set of
    negative rows keeps its negative maximum)."""
    xs = np.asarray(xs, dtype=np.float64)
    out = np.zeros((n, xs.shape[1]), dtype=np.float64)
    if kind == "max":
        m = np.full((n, xs.shape[1]), -np.inf)
        np.maximum.at(m, dst, xs[src])
        has = np.zeros(n, dtype=bool)
        has[dst] = True
        out[has] = m[has]
        return out
    np.add.at(out, dst, xs[src])
    if kind == "mean":
        cnt = np.zeros(n, dtype=np.float64)
        np.add.at(cnt, dst, 1.0)
        out /= np.maximum(cnt, 1.0)[:, None]
    else:
        assert kind == "sum", kind
    return out


_KIND = {"mean": "mean", "add": "sum", "sum": "sum", "max": "max"}


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def conv_spec(conv):
    """A conv module as plain fp64 arrays: {"kind", "W", "b", "root"} (SAGEConv / GraphConv) or
    {"kind": "sum", "eps", "mlp": [(W, b, act)]} (GINConv)."""
    name = type(conv).__name__
    if name == "SAGEConv":
        return {"kind": _KIND[conv.aggr], "W": _np(conv.lin_l.weight), "b": _np(conv.lin_l.bias),
                "root": _np(conv.lin_r.weight)}
    if name == "GraphConv":
        return {"kind": _KIND[conv.aggr], "W": _np(conv.lin_rel.weight), "b": _np(conv.lin_rel.bias),
                "root": _np(conv.lin_root.weight)}
    assert name == "GINConv", name
    mlp, pend = [], None
    mods = [conv.nn] if hasattr(conv.nn, "weight") else list(conv.nn.children())
    for m in mods:
        if hasattr(m, "weight"):
            if pend is not None:
                mlp.append(pend + (None,))
            pend = (_np(m.weight), _np(m.bias))
        else:
            mlp.append(pend + ({"ReLU": "relu", "Sigmoid": "sigmoid", "Tanh": "tanh"}[type(m).__name__],))
            pend = None
    if pend is not None:
        mlp.append(pend + (None,))
    return {"kind": "sum", "eps": float(_np(conv.eps).reshape(-1)[0]), "mlp": mlp}


def conv_apply(spec, xs, xd, src, dst):
    agg = aggregate(xs, src, dst, xd.shape[0], spec["kind"])
    if "mlp" in spec:
        z = agg + (1.0 + spec["eps"]) * xd
        for W, b, act in spec["mlp"]:
            z = z @ W.T + (0 if b is None else b)
            z = oracle.apply_act(z, act)
        return z
    out = agg @ spec["W"].T + xd @ spec["root"].T
    return out if spec["b"] is None else out + spec["b"]


def _head(arch, h):
    n_fc = len(arch.fc) // 2
    for i in range(n_fc):
        lin, act = arch.fc[2 * i], arch.fc[2 * i + 1]
        h = h @ _np(lin.weight).T + _np(lin.bias)
        h = oracle.apply_act(h, {"ReLU": "relu", "Sigmoid": "sigmoid", "Identity": None}[type(act).__name__])
    return h


def kept_edges(masks, rel_edges):
    """Per relation the union graph's kept (src, dst): copy b keeps (u, v) iff mask[b, u] &
    mask[b, v], node ids shifted by b * S."""
    kept = []
    for ei in rel_edges:
        keep, tiled = oracle.build_edge_mask(masks, ei)
        kept.append((tiled[0][keep], tiled[1][keep]))
    return kept


def union_outputs(arch, x, rel_edges, masks):
    """fp64 outputs [B, S] of a ConvStack (conv = [Conv or single-type HeteroConv, ReLU]*, fc =
    [Linear, act]*) on the B-fold union graph."""
    B, S = masks.shape
    h, _ = oracle.concat_features(np.asarray(x, dtype=np.float64), B)
    kept = kept_edges(masks, rel_edges)
    for li in range(len(arch.conv) // 2):
        conv = arch.conv[2 * li]
        if hasattr(conv, "convs"):
            out = 0
            for sub, (src, dst) in zip(conv.convs.values(), kept):
                out = out + conv_apply(conv_spec(sub), h, h, src, dst)
        else:
            out = conv_apply(conv_spec(conv), h, h, kept[0][0], kept[0][1])
        h = np.maximum(out, 0)
    return _head(arch, h)[:, 0].reshape(B, S)


def program_outputs(prog, x, rel_edges, masks):
    """The compiled program's layers (terms of kind root / sum / max / mean, bias, activation, then
    the head) applied by the restatement on the union graph, fp64: [B, S]."""
    B, S = masks.shape
    h, _ = oracle.concat_features(np.asarray(x, dtype=np.float64), B)
    kept = kept_edges(masks, rel_edges)
    for conv in prog.convs:
        out = np.zeros((h.shape[0], conv.f_out))
        for t in conv.terms:
            W = _np(t.weight)
            if t.kind == "root":
                out += h @ W.T
            else:
                src, dst = kept[t.rel]
                out += aggregate(h, src, dst, h.shape[0], t.kind) @ W.T
        h = oracle.apply_act(out + _np(conv.bias), conv.act)
    for hd in prog.head:
        h = h @ _np(hd.weight).T + (0 if hd.bias is None else _np(hd.bias))
        h = oracle.apply_act(h, hd.act)
    return h[:, 0].reshape(B, S)


def multi_type_copy_outputs(arch, c, masks):
    """Model.predict_hetero_output per mask row for a multi-node-type stack of SAGEConv /
    GraphConv relations (oracle.hetero_multi_copy_outputs with the relation's own aggregation):
    a copy without edges outputs 0, else HeteroConv-sum per destination type, ReLU, the head on
    the first output type, value out[sub_ind, 0].  `c`: golden_utils.multi_type_setup's dict."""
    x, nt, ei, et = (np.asarray(c[k]) for k in ("x", "nt", "ei", "et"))
    names, rels, pads = c["ntypes"], c["rels"], c["pads"]
    m = np.asarray(masks, dtype=bool)
    pointers = [int(np.where(nt == i)[0][0]) for i in range(len(names))]
    blocks = {}
    for i, name in enumerate(names):
        blk = x[nt == i].astype(np.float64)
        blocks[name] = blk[:, :-pads[i]] if pads[i] > 0 else blk
    specs = [{tuple(k.split("__")): conv_spec(sub) for k, sub in arch.conv[2 * li].convs.items()}
             for li in range(len(arch.conv) // 2)]
    out = np.zeros(m.shape[0])
    for b in range(m.shape[0]):
        keep = m[b, ei[0]] & m[b, ei[1]]
        if not keep.any():
            continue
        h = dict(blocks)
        for layer in specs:
            nxt = {}
            for k, rel in enumerate(rels):
                if rel not in layer:
                    continue
                sel = keep & (et == k)
                src = ei[0, sel] - pointers[names.index(rel[0])]
                dst = ei[1, sel] - pointers[names.index(rel[-1])]
                o = conv_apply(layer[rel], h[rel[0]], h[rel[-1]], src, dst)
                nxt[rel[-1]] = o if rel[-1] not in nxt else nxt[rel[-1]] + o
            h = {k: np.maximum(v, 0) for k, v in nxt.items()}
        out[b] = _head(arch, h[next(iter(h))])[c["sub_ind"], 0]
    return out
