"""fp64 numpy restatement of a typed link model (an RGCNConv encoder + a DistMult or dot-product
decoder, nn.RelLinkModel) on the B-fold union graph of Data.perturb_edge, for
tests/test_rel_edge_cpu.py and tests/test_gpu_rel_edge.py: copy b keeps edge e iff mask[b, e], node
ids shifted by b * N, the kept edges' types follow the kept edges, features are never masked.  It
reads state dicts and attributes only (never a module's forward); the conv maths is
tests/rgcn_ref.py's."""
import numpy as np

import oracle
from rgcn_ref import _ACT, _head, _np, conv_apply, conv_spec, relation_aggregate  # noqa: F401


def _sigmoid(s):
    return 0.5 * (1.0 + np.tanh(0.5 * s))  # 1 / (1 + exp(-s)) without the overflow at large -s


def kept_union_edges(masks, ei, et, n):
    """(src, dst, type) of the union graph's kept edges, copy-major, each copy in edge order."""
    masks = np.asarray(masks, dtype=bool)
    rows, cols = np.nonzero(masks)
    ei = np.asarray(ei)
    return ei[0][cols] + rows * n, ei[1][cols] + rows * n, np.asarray(et)[cols]


def encoder_outputs(enc, x, ei, et, masks, with_peak=False):
    """z [B, N, C] fp64 of an RGCNStack-shaped encoder (conv = [RGCNConv, act]*, fc = [Linear,
    act]*) on the union graph; with_peak: also the largest |conv pre-activation|."""
    B = np.asarray(masks).shape[0]
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    h = np.tile(x, (B, 1))
    src, dst, types = kept_union_edges(masks, ei, et, n)
    peak = 0.0
    for li in range(len(enc.conv) // 2):
        out = conv_apply(conv_spec(enc.conv[2 * li]), h, src, dst, types)
        peak = max(peak, float(np.abs(out).max()))
        h = oracle.apply_act(out, _ACT[type(enc.conv[2 * li + 1]).__name__])
    z = _head(enc, h).reshape(B, n, -1)
    return (z, peak) if with_peak else z


def decode(model, z, u, v, label_type, act=True):
    """[B] fp64 scores of edge (u, v) with type label_type in every copy."""
    zu, zv = z[:, u, :], z[:, v, :]
    emb = getattr(model, "rel_emb", None)
    s = zu * zv if emb is None else zu * _np(emb)[int(label_type)][None, :] * zv
    s = s.sum(-1)
    if act and model.act == "sigmoid":
        s = _sigmoid(s)
    return s


def edge_outputs(model, x, ei, et, masks, u, v, label_type, with_peak=False):
    """[B] fp64: the model's score of query edge (u, v, label_type) per mask row."""
    z, peak = encoder_outputs(model.encoder, x, ei, et, masks, True)
    y = decode(model, z, u, v, label_type)
    return (y, peak) if with_peak else y


def all_edge_outputs(model, x, ei, et, label_index=None, label_type=None):
    """[n_label] fp64 of the unmasked graph: the module's forward with its defaults (every edge
    with its own type) or an explicit label index / type."""
    ei = np.asarray(ei)
    z = encoder_outputs(model.encoder, x, ei, et, np.ones((1, ei.shape[1]), dtype=bool))[0]
    li = ei if label_index is None else np.asarray(label_index)
    lt = np.asarray(et) if label_type is None else np.asarray(label_type)
    emb = getattr(model, "rel_emb", None)
    s = z[li[0]] * z[li[1]]
    if emb is not None:
        s = s * _np(emb)[lt]
    s = s.sum(-1)
    return _sigmoid(s) if model.act == "sigmoid" else s


# ------------------------------------------------------------------ shared inputs of both suites
def typed_hub_graph(R, seed=0):
    """120 nodes, ~510 typed edges (shuffled): node 0 a hub with 300 in-edges over types 0, 1, 2
    (sources repeat: duplicates of one type and of two types); nodes 10..14 with 1, 3, 4, 5 and 9
    in-edges of type 0 only (the rounds of 4 edges and their tails); 12 random edges duplicated
    with their own type and 12 with another; node 7 with two type-0 self-loops (distinct columns)
    and one type-1 self-loop; node 20 seeing relation 1 only; relation R - 1 absent (R >= 4).
    Returns (edge_index [2, E], edge_type [E], info)."""
    g = np.random.default_rng(seed)
    S = 120
    Ru = max(1, min(R - 1, 3)) if R >= 4 else R  # types in use
    src, dst, typ = [], [], []

    def add(u, v, t):
        src.append(int(u))
        dst.append(int(v))
        typ.append(int(t))
    for k in range(300):                                   # the hub
        add(g.integers(1, S), 0, k % min(3, Ru))
    for node, deg in zip((10, 11, 12, 13, 14), (1, 3, 4, 5, 9)):
        for u in g.choice(np.arange(30, S), deg, replace=False):
            add(u, node, 0)
    n_rand = 150
    for _ in range(n_rand):
        u, v = g.integers(0, S), g.integers(21, S)
        if u != v:
            add(u, v, g.integers(0, Ru))
    base = len(src)
    for k in g.choice(np.arange(322, base), 24, replace=False):
        add(src[k], dst[k], typ[k] if len(src) % 2 else (typ[k] + 1) % Ru)
    for t in (0, 0, min(1, Ru - 1)):
        add(7, 7, t)
    for u in (3, 40, 41):                                  # node 20: relation 1 only
        add(u, 20, min(1, Ru - 1))
    add(20, 7, 0)
    add(7, 25, 0)
    add(0, 7, min(2, Ru - 1))
    add(10, 20, min(1, Ru - 1))
    ei = np.array([src, dst], dtype=np.int64)
    et = np.array(typ, dtype=np.int64)
    perm = g.permutation(ei.shape[1])
    ei, et = ei[:, perm], et[perm]

    def find(u, v, t=None):
        hit = np.nonzero((ei[0] == u) & (ei[1] == v) & ((et == t) if t is not None else True))[0]
        return [int(i) for i in hit]
    info = {"S": S, "loops7_t0": find(7, 7, 0), "regular": find(20, 7)[0], "loop": find(7, 7, 0)[0],
            "into_hub": int(np.nonzero(ei[1] == 0)[0][5])}
    return ei, et, info


def hub_masks(ei, et, info, query, rows=70, seed=3):
    """70 rows over the edge columns: row 0 all on, row 1 all off, row 2 drops every in-edge of
    the query's source and keeps the rest, row 3 keeps exactly one of node 7's two type-0
    self-loops (all else on), the others with P(bit) drawn per row in [0.2, 0.9]."""
    g = np.random.default_rng(seed)
    E = ei.shape[1]
    m = g.random((rows, E)) < g.uniform(0.2, 0.9, (rows, 1))
    m[0], m[1] = True, False
    if rows > 2:
        m[2] = ei[1] != ei[0][query]
    if rows > 3:
        m[3] = True
        m[3, info["loops7_t0"][1]] = False
    return m
