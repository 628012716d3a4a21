"""fp64 numpy restatement of RGCNConv / FastRGCNConv (PyG 2.0.4) stacks on the reference's B-fold
union graph, for tests/test_rgcn_cpu.py and tests/test_gpu_rgcn.py.  It reads a module's state
dict and attributes only (never its forward, and not nn.RGCNConv's helpers): per layer and
relation an explicit mean or sum with a 0 fill for targets without an in-edge of that relation,
then the linear maps (W_r is [in, out])."""
import numpy as np

import oracle


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def relation_aggregate(xs, src, dst, n, kind):
    """[n, F] fp64: per target the sum / mean of xs[src] over the given edges (duplicates are
    separate entries); a target without one gets 0."""
    xs = np.asarray(xs, dtype=np.float64)
    out = np.zeros((n, xs.shape[1]), dtype=np.float64)
    cnt = np.zeros(n, dtype=np.float64)
    np.add.at(out, dst, xs[src])
    np.add.at(cnt, dst, 1.0)
    if kind == "mean":
        nz = cnt > 0
        out[nz] /= cnt[nz][:, None]
    else:
        assert kind in ("add", "sum"), kind
    return out


def conv_spec(conv):
    """An RGCNConv as plain fp64 arrays: {"W": [R, in, out], "root", "b", "kind"}."""
    w = _np(conv.weight)
    R = int(conv.num_relations)
    if getattr(conv, "num_bases", None) is not None:
        comp = _np(conv.comp)
        W = np.zeros((R,) + w.shape[1:])
        for r in range(R):
            for b in range(w.shape[0]):
                W[r] += comp[r, b] * w[b]
    elif getattr(conv, "num_blocks", None) is not None:
        nb, bi, bo = w.shape[1:]
        W = np.zeros((R, nb * bi, nb * bo))
        for r in range(R):
            for k in range(nb):
                W[r, k * bi:(k + 1) * bi, k * bo:(k + 1) * bo] = w[r, k]
    else:
        W = w
    assert W.shape[0] == R
    return {"W": W, "root": _np(getattr(conv, "root", None)), "b": _np(getattr(conv, "bias", None)),
            "kind": conv.aggr}


def conv_apply(spec, x, src, dst, et):
    n = x.shape[0]
    out = np.zeros((n, spec["W"].shape[2]))
    et = np.asarray(et)
    for r in range(spec["W"].shape[0]):
        sel = et == r
        if sel.any():
            out += relation_aggregate(x, src[sel], dst[sel], n, spec["kind"]) @ spec["W"][r]
    if spec["root"] is not None:
        out += x @ spec["root"]
    if spec["b"] is not None:
        out += spec["b"]
    return out


_ACT = {"ReLU": "relu", "Sigmoid": "sigmoid", "Identity": None, "Tanh": "tanh"}


def _head(arch, h):
    for i in range(len(arch.fc) // 2):
        lin, act = arch.fc[2 * i], arch.fc[2 * i + 1]
        h = h @ _np(lin.weight).T + _np(lin.bias)
        h = oracle.apply_act(h, _ACT[type(act).__name__])
    return h


def kept_union(masks, ei, et):
    """The union graph's kept edges (src, dst, type): copy b keeps (u, v) iff mask[b, u] &
    mask[b, v], node ids shifted by b * S; the perturbed edge types follow the kept edges."""
    keep, tiled = oracle.build_edge_mask(masks, ei)
    types = np.tile(np.asarray(et), masks.shape[0])
    return tiled[0][keep], tiled[1][keep], types[keep]


def union_outputs(arch, x, ei, et, masks, with_peak=False):
    """fp64 outputs [B, S] of an RGCNStack-shaped module (conv = [RGCNConv, act]*, fc = [Linear,
    act]*) on the B-fold union graph.  with_peak: also the largest |pre-activation| of any conv
    layer at any node of the union graph."""
    B, S = masks.shape
    h, _ = oracle.concat_features(np.asarray(x, dtype=np.float64), B)
    src, dst, types = kept_union(masks, ei, et)
    peak = 0.0
    for li in range(len(arch.conv) // 2):
        out = conv_apply(conv_spec(arch.conv[2 * li]), h, src, dst, types)
        peak = max(peak, float(np.abs(out).max()))
        h = oracle.apply_act(out, _ACT[type(arch.conv[2 * li + 1]).__name__])
    y = _head(arch, h)[:, 0].reshape(B, S)
    return (y, peak) if with_peak else y


def program_outputs(prog, x, ei, et, masks):
    """The compiled program's layers ("rel" and "root" terms, bias, activation, then the head)
    evaluated on the union graph in fp64: [B, S]."""
    B, S = masks.shape
    h, _ = oracle.concat_features(np.asarray(x, dtype=np.float64), B)
    src, dst, types = kept_union(masks, ei, et)
    n = h.shape[0]
    for conv in prog.convs:
        out = np.zeros((n, conv.f_out))
        for t in conv.terms:
            W = _np(t.weight)
            if t.kind == "root":
                out += h @ W.T
                continue
            assert t.kind == "rel"
            aggs = []
            for r in range(t.num_relations):
                sel = types == r
                aggs.append(relation_aggregate(h, src[sel], dst[sel], n, t.norm))
            coef = np.eye(t.num_relations) if t.coef is None else _np(t.coef)
            assert coef.shape == (t.num_relations, t.slices) and W.shape[0] == t.slices
            for s in range(t.slices):
                blk = sum(coef[r, s] * aggs[r] for r in range(t.num_relations))
                out += blk @ W[s].T
        h = oracle.apply_act(out + _np(conv.bias), conv.act)
    for hd in prog.head:
        h = h @ _np(hd.weight).T + (0 if hd.bias is None else _np(hd.bias))
        h = oracle.apply_act(h, hd.act)
    return h[:, 0].reshape(B, S)


def segments_brute(rel_edges, targets):
    """Per target (a list of node ids) the ascending relations that have an in-edge or a self-loop
    at it: (seg_ptr, seg_rel) by a plain loop."""
    seg_ptr, seg_rel = [0], []
    for t in targets:
        for r, e in enumerate(rel_edges):
            if any(int(d) == int(t) for d in np.asarray(e[1]).tolist()):
                seg_rel.append(r)
        seg_ptr.append(len(seg_rel))
    return np.asarray(seg_ptr, dtype=np.int64), np.asarray(seg_rel, dtype=np.int64)
