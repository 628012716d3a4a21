"""fp64 NumPy restatement of GATv2Conv (PyG 2.0.4) for the GATv2 tests: one Python loop over the
targets, each over its own kept edge set, on the B-fold union graph of the reference (features
tiled, copy b keeps edge (u, v) iff mask[b, u] & mask[b, v], node ids shifted by b * S).  It is
deliberately not the vectorised scatter form of nn.GATv2Conv, so the two can disagree."""
import functools

import numpy as np
import torch

import oracle
import pool_ref

QUERIES = [0, 7, 399]


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def conv_params(conv):
    shared = conv.lin_r is conv.lin_l
    return {"Wl": _np(conv.lin_l.weight), "bl": _np(conv.lin_l.bias),
            "Wr": None if shared else _np(conv.lin_r.weight),
            "br": None if shared else _np(conv.lin_r.bias),
            "att": _np(conv.att).reshape(conv.heads, conv.out_channels), "bias": _np(conv.bias),
            "concat": bool(conv.concat), "slope": float(conv.negative_slope),
            "self_loops": bool(conv.add_self_loops)}


def gatv2_conv(h, src, dst, p):
    """out [N, H * C] (or [N, C] with concat False): per target t the softmax over its in-edges of
    z = sum_c att[h, c] * leaky_relu(XL[u, h, c] + XR[t, h, c]); alpha = exp(z - max) / (sum +
    1e-16); out[t, h] = sum alpha XL[u, h]; a target without an edge gets 0; then + bias."""
    att = p["att"]
    H, C = att.shape
    n = h.shape[0]
    xl = h @ p["Wl"].T + (0 if p["bl"] is None else p["bl"])
    xr = xl if p["Wr"] is None else h @ p["Wr"].T + (0 if p["br"] is None else p["br"])
    xl, xr = xl.reshape(n, H, C), xr.reshape(n, H, C)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if p["self_loops"]:  # existing loops removed, exactly one added per node
        keep = src != dst
        loop = np.arange(n, dtype=np.int64)
        src, dst = np.concatenate([src[keep], loop]), np.concatenate([dst[keep], loop])
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    tgts, lo = np.unique(dst, return_index=True)
    hi = np.append(lo[1:], dst.size)
    out = np.zeros((n, H, C))
    slope = p["slope"]
    for t, a, b in zip(tgts, lo, hi):
        xs = xl[src[a:b]]                                   # [E_t, H, C]
        s = xs + xr[t]
        z = (att * np.where(s > 0, s, slope * s)).sum(-1)   # [E_t, H]
        pe = np.exp(z - z.max(0))
        alpha = pe / (pe.sum(0) + 1e-16)
        out[t] = (alpha[:, :, None] * xs).sum(0)
    out = out.reshape(n, H * C) if p["concat"] else out.mean(1)
    return out if p["bias"] is None else out + p["bias"]


def _one_conv(conv, h, src, dst):
    name = type(conv).__name__
    if name == "GATv2Conv":
        return gatv2_conv(h, src, dst, conv_params(conv))
    if name == "GCNConv":
        return oracle.gcn_conv(h, src, dst, h.shape[0], _np(conv.lin.weight), _np(conv.bias))
    raise ValueError(name)


def kept_edges(masks, rel_edges):
    out = []
    for ei in rel_edges:
        keep, tiled = oracle.build_edge_mask(masks, ei)
        out.append((tiled[0][keep], tiled[1][keep]))
    return out


def encoder_rows(encoder, x, rel_edges, masks, uniform=False):
    """h [B * S, C] fp64 after the conv layers ([Conv or single-type HeteroConv, ReLU]*).
    `uniform`: every GATv2Conv's att replaced by 0 (uniform attention), for the sensitivity checks."""
    B = masks.shape[0]
    h, _ = oracle.concat_features(np.asarray(x, dtype=np.float64), B)
    kept = kept_edges(masks, rel_edges)

    def run(conv, h, src, dst):
        if uniform and type(conv).__name__ == "GATv2Conv":
            p = conv_params(conv)
            p["att"] = np.zeros_like(p["att"])
            return gatv2_conv(h, src, dst, p)
        return _one_conv(conv, h, src, dst)
    for li in range(len(encoder.conv) // 2):
        conv = encoder.conv[2 * li]
        if hasattr(conv, "convs"):
            out = 0
            for sub, (src, dst) in zip(conv.convs.values(), kept):
                out = out + run(sub, h, src, dst)
        else:
            out = run(conv, h, kept[0][0], kept[0][1])
        h = np.maximum(out, 0)
    return h


def head(fc, h):
    """The [Linear, act]* list `fc` (ReLU / Sigmoid / Identity) in fp64."""
    for m in fc:
        name = type(m).__name__
        if name == "Linear":
            h = h @ _np(m.weight).T + (0 if m.bias is None else _np(m.bias))
        else:
            h = oracle.apply_act(h, {"ReLU": "relu", "Sigmoid": "sigmoid", "Identity": None}[name])
    return h


def union_outputs(arch, x, rel_edges, masks, uniform=False):
    """fp64 outputs [B, S] (column 0) of a ConvStack-shaped arch on the union graph."""
    masks = np.asarray(masks, dtype=bool)
    h = encoder_rows(arch, x, rel_edges, masks, uniform)
    return head(arch.fc, h)[:, 0].reshape(masks.shape)


def pooled_outputs(arch, x, rel_edges, masks):
    """fp64 outputs [B] (column 0) of nn.PooledModel(ConvStack("gatv2", ...), pool, fc)."""
    masks = np.asarray(masks, dtype=bool)
    h = encoder_rows(arch.encoder, x, rel_edges, masks)
    return head(arch.fc, pool_ref.pool_rows(h, masks.shape[0], arch.pool))[:, 0]


# ------------------------------------------------------------------ shared inputs (GPU parity cases)
def hub_graph(S=400, seed=0):
    """The hub graph of tests/test_gpu_attention.py: ~2,400 random edges, 5 explicit self-loops,
    20 duplicated edges, node 0 a hub target with 300 extra in-edges."""
    g = np.random.default_rng(seed)
    ei = g.integers(0, S, (2, 2400))
    ei = ei[:, ei[0] != ei[1]]
    loops = np.array([0, 7, 33, 200, 399])
    dup = ei[:, g.choice(ei.shape[1], 20, replace=False)]
    hub = np.stack([g.choice(np.arange(1, S), 300, replace=False), np.zeros(300, np.int64)])
    ei = np.concatenate([ei, np.stack([loops, loops]), dup, hub], 1)
    return ei[:, g.permutation(ei.shape[1])].astype(np.int64)


def row_masks(rows, S, seed, queries=(0,)):
    """Per-row keep probability uniform in (0, 1); row 0 all-off, row 1 all-on, then one row per
    query with the query itself masked."""
    g = np.random.default_rng(seed)
    m = g.random((rows, S)) < g.uniform(0.0, 1.0, (rows, 1))
    m[0], m[1] = False, True
    for r, q in enumerate(queries, 2):
        m[r] = g.random(S) < 0.7
        m[r, q] = False
    return m


def features(S=400, f=16):
    return torch.randn((S, f), generator=torch.Generator().manual_seed(21))


def scale_att(arch, s):
    with torch.no_grad():
        for m in arch.modules():
            if type(m).__name__ == "GATv2Conv":
                m.att.mul_(s)


@functools.lru_cache(maxsize=None)
def hub_case(self_loops, att_scale=1.0):
    """ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1]) on the hub graph, 64 mask rows, queries
    [0, 7, 399]; the reference [64, 3] and the same model under uniform attention (att = 0)."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    S = 400
    x, ei = features(S), hub_graph(S)
    torch.manual_seed(17)
    arch = ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1], add_self_loops=self_loops).eval()
    scale_att(arch, att_scale)
    m = row_masks(64, S, 3, QUERIES)
    ref = union_outputs(arch, x.numpy(), [ei], m)[:, QUERIES]
    uni = union_outputs(arch, x.numpy(), [ei], m, uniform=True)[:, QUERIES]
    return {"S": S, "x": x, "ei": ei, "arch": arch, "masks": m, "ref": ref, "uniform": uni}
