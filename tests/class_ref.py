"""fp64 NumPy restatement of the class readout of a multi-class model (none / softmax / log_softmax
over the C real output columns) for tests/test_classes_cpu.py and tests/test_gpu_classes.py, and
the shared inputs of the two files, so the CPU file asserts its non-vacuity conditions on the very
inputs the GPU file uses.  It shares no code with nn.py or engine.py: the rows a model's head reads
come from the existing restatements (gatv2_ref, pool_ref, block_ref, edge_weight_ref, edge_attr_ref,
oracle.gcn_conv), the head and the readout are restated here.  It reads a module's state and
attributes only, never its forward (module_outputs, which defines e32, is the one exception)."""
import copy
import functools

import numpy as np
import torch

import block_ref
import edge_attr_ref
import edge_weight_ref
import gatv2_ref
import oracle
import pool_ref

QUERIES = [0, 7, 399]
ROWS = 64
KINDS = ("softmax", "log_softmax")
NAMES = ["gcn", "sage-max", "gin", "gatv2", "gine", "gcn-weighted", "block-layer", "pooled-mean", "headless"]
CLASSES = [2, 7, 33]
_np = block_ref._np


# ------------------------------------------------------------------ the readout
def class_out(z, kind, n_real=None):
    """z [..., ld] -> fp64 [..., C]: columns [0, C) of z (kind None), their softmax or their
    log_softmax; columns past C (padding) never take part."""
    z = np.asarray(z, dtype=np.float64)
    z = z[..., :z.shape[-1] if n_real is None else n_real]
    if kind is None:
        return z.copy()
    d = z - z.max(-1, keepdims=True)
    s = np.exp(d).sum(-1, keepdims=True)
    return np.exp(d) / s if kind == "softmax" else d - np.log(s)


def head_rows(fc, h):
    """The units `fc` ([Linear, act]* with an optional last Softmax / LogSoftmax) on rows h in
    fp64: (z, kind) with z the last linear output (after element-wise activations) and kind the
    readout that follows it (None, "softmax", "log_softmax")."""
    kind = None
    for m in fc:
        name = type(m).__name__
        assert kind is None, "a unit after the softmax"
        if name == "Linear":
            h = h @ _np(m.weight).T + (0 if m.bias is None else _np(m.bias))
        elif name in ("Softmax", "LogSoftmax"):
            assert m.dim in (-1, 1)
            kind = "softmax" if name == "Softmax" else "log_softmax"
        else:
            h = oracle.apply_act(h, {"ReLU": "relu", "Sigmoid": "sigmoid", "Identity": None}[name])
    return h, kind


class HeadlessGCN(torch.nn.Module):
    """conv = [GCNConv, ReLU, GCNConv], then LogSoftmax / Softmax: a node classifier without a head."""

    def __init__(self, dims, out):
        super().__init__()
        from bikg_graph_explainability_public_amd import nn as xnn
        self.conv = torch.nn.ModuleList([xnn.GCNConv(dims[0], dims[1]), torch.nn.ReLU(),
                                         xnn.GCNConv(dims[1], dims[2])])
        self.out = torch.nn.LogSoftmax(dim=-1) if out == "log_softmax" else torch.nn.Softmax(dim=1)

    def forward(self, x, edge_index):
        for i, c in enumerate(self.conv):
            x = c(x, edge_index) if i % 2 == 0 else c(x)
        return self.out(x)


def encoder_rows(name, arch, x, ei, masks, w=None, ea=None):
    """h [B * S, F] fp64: the rows the head (or, headless, the readout) of model family `name`
    reads, one per (mask row, node); the pooled family: [B, F] after the mean readout."""
    masks = np.asarray(masks, dtype=bool)
    if name in ("gcn", "gatv2"):
        return gatv2_ref.encoder_rows(arch, x, [ei], masks)
    if name in ("sage-max", "gin"):
        return pool_ref.encoder_rows(arch, x, [ei], masks)[0]
    if name == "gine":
        return edge_attr_ref.encoder_rows(arch, x, ei, ea, masks)
    if name == "gcn-weighted":
        return edge_weight_ref.encoder_rows(arch, x, ei, w, masks)
    if name == "block-layer":
        return block_ref.encoder_rows(arch, x, ei, masks)
    if name == "pooled-mean":
        return pool_ref.pool_rows(gatv2_ref.encoder_rows(arch.encoder, x, [ei], masks), masks.shape[0], "mean")
    assert name == "headless", name
    (src, dst), = gatv2_ref.kept_edges(masks, [ei])
    h = np.tile(np.asarray(x, dtype=np.float64), (masks.shape[0], 1))
    c0, c2 = arch.conv[0], arch.conv[2]
    h = np.maximum(oracle.gcn_conv(h, src, dst, h.shape[0], _np(c0.lin.weight), _np(c0.bias)), 0)
    return oracle.gcn_conv(h, src, dst, h.shape[0], _np(c2.lin.weight), _np(c2.bias))


def outputs(name, arch, h, masks):
    """fp64 model outputs from the encoder rows h: [B, Q, C] at QUERIES (pooled: [B, 1, C])."""
    B, S = masks.shape
    if name == "headless":
        out = class_out(h, "softmax" if type(arch.out).__name__ == "Softmax" else "log_softmax")
    else:
        z, kind = head_rows(arch.fc, h)
        out = class_out(z, kind)
    if name == "pooled-mean":
        return out.reshape(B, 1, -1)
    return out.reshape(B, S, -1)[:, QUERIES]


def module_outputs(name, arch, x, ei, masks, w=None, ea=None, dtype=torch.float32):
    """The module's own forward on the union graph in `dtype`, shaped like `outputs`, as float64: in
    float32 its distance from the restatement is e32, the error float32 arithmetic alone gives on
    these inputs."""
    masks = np.asarray(masks, dtype=bool)
    B, S = masks.shape
    keep, tiled = oracle.build_edge_mask(masks, np.asarray(ei))
    m = copy.deepcopy(arch).to(dtype).eval()
    xt = torch.as_tensor(np.asarray(x)).to(dtype).repeat(B, 1)
    kw = {}
    if w is not None:
        kw["edge_weight"] = torch.as_tensor(np.tile(w, B)[keep]).to(dtype)
    if ea is not None:
        kw["edge_attr"] = torch.as_tensor(np.tile(ea, (B, 1))[keep]).to(dtype)
    eit = torch.as_tensor(tiled[:, keep])
    with torch.no_grad():
        if name == "pooled-mean":
            return m(xt, eit, torch.arange(B).repeat_interleave(S), **kw).double().numpy().reshape(B, 1, -1)
        return m(xt, eit, **kw).double().numpy().reshape(B, S, -1)[:, QUERIES]


# ------------------------------------------------------------------ shared inputs
def build(name, C, out):
    """Model family `name` with C classes ending in `out` (softmax / log_softmax); the conv
    parameters are drawn first from one seed, so they are the same for every (C, out)."""
    from bikg_graph_explainability_public_amd import nn as xnn
    torch.manual_seed(17)
    if name == "headless":
        return HeadlessGCN([16, 8, C], out).eval()
    if name == "pooled-mean":
        return xnn.PooledModel(xnn.ConvStack("gcn", [16, 8, 8], [8]), "mean", [8, C], final_act=out).eval()
    if name == "block-layer":
        arch = xnn.BlockStack("gcn", [16, 8, 8], [8, C], norm="layer", final_act=out)
        return block_ref.randomise_norms(arch, 6).eval()
    kw = {"heads": [2, 1]} if name == "gatv2" else {"edge_dim": 5} if name == "gine" else {}
    kind = "gcn" if name == "gcn-weighted" else name
    return xnn.ConvStack(kind, [16, 8, 8], [8, C], final_act=out, **kw).eval()


def _conv_weights(arch):
    enc = arch.encoder if hasattr(arch, "encoder") else arch
    return [p for n, p in enc.conv.named_parameters() if n.endswith("weight") and p.dim() == 2]


def scale_convs(arch, s):
    with torch.no_grad():
        for p in _conv_weights(arch):
            p.mul_(s)


def scale_head(arch, s):
    """The last linear map of the model: the head's last Linear, headless the last conv."""
    last = arch.conv[2].lin if not hasattr(arch, "fc") else [m for m in arch.fc if type(m).__name__ == "Linear"][-1]
    with torch.no_grad():
        last.weight.mul_(s)
        if getattr(last, "bias", None) is not None:
            last.bias.mul_(s)


def explained_class(C):
    """The class the one-class checks explain: the middle column (never 0)."""
    return max(1, C // 2)


def sensitive(ref, kind, c, bar=1e-5):
    """The two non-vacuity conditions on a reference [B, Q, C] of readout `kind`: at least half of
    the explained-class probabilities in (0.02, 0.98), and on at least half of the rows class c's
    output more than 100 x bar from class 0's."""
    p = np.exp(ref[..., c]) if kind == "log_softmax" else ref[..., c]
    return bool(np.mean((p > 0.02) & (p < 0.98)) >= 0.5 and
                np.mean(np.abs(ref[..., c] - ref[..., 0]) > 100 * bar) >= 0.5)


_LADDER = [1.0, 0.5, 2.0, 0.25, 4.0, 0.125, 8.0, 1 / 16, 16.0, 1 / 32, 32.0, 1 / 64, 64.0, 1 / 256, 256.0]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    S = 400
    x = torch.randn((S, 16), generator=torch.Generator().manual_seed(21))
    ei = pool_ref.hub_graph(S)
    w = edge_weight_ref.hub_weights(ei) if name == "gcn-weighted" else None
    ea = edge_attr_ref.hub_attrs(ei, 5) if name == "gine" else None
    masks = gatv2_ref.row_masks(ROWS, S, 3, QUERIES)
    assert masks[1].all() and not masks[0].any()
    return S, x, ei, w, ea, masks


@functools.lru_cache(maxsize=None)
def _conv_scale(name):
    """Halve the conv weights until no row the head reads exceeds 8 in magnitude (sums over the
    300-edge hub otherwise give logits whose float32 rounding alone passes the softmax bar).  Read
    from the fp64 rows alone; the same for every (C, out)."""
    if name == "headless":
        return 1.0
    S, x, ei, w, ea, masks = _inputs(name)
    arch, s = build(name, 2, "softmax"), 1.0
    for _ in range(16):
        if np.abs(encoder_rows(name, arch, x.numpy(), ei, masks, w, ea)).max() <= 8:
            return s
        scale_convs(arch, 0.5)
        s *= 0.5
    raise AssertionError("no conv scale bounds the encoder rows")


@functools.lru_cache(maxsize=None)
def _rows(name, C):
    """The encoder rows of a family (they do not depend on the head: shared by every C and out;
    the headless family's last conv has C columns)."""
    S, x, ei, w, ea, masks = _inputs(name)
    arch = build(name, C, "softmax")
    scale_convs(arch, _conv_scale(name))
    return encoder_rows(name, arch, x.numpy(), ei, masks, w, ea)


@functools.lru_cache(maxsize=None)
def case(name, C, out):
    """The GPU parity case (family, C, readout) on the 400-node hub graph, 64 mask rows (row 0
    all-off, row 1 all-on), queries [0, 7, 399] (pooled: the one graph row).  The last linear map
    is scaled along a fixed ladder until `sensitive` holds for both readouts of the family on the
    fp64 reference (as pool_ref.fit_scale fits its scale: from the reference alone).  Returns the
    inputs, the reference [64, Q, C] and the explained class."""
    S, x, ei, w, ea, masks = _inputs(name)
    c = explained_class(C)
    for s in _LADDER:
        archs = {}
        for k in KINDS:
            a = build(name, C, k)
            scale_convs(a, _conv_scale(name))
            scale_head(a, s)
            archs[k] = a
        if name == "headless":  # the scaled map is a conv: its rows change with it
            hs = {k: encoder_rows(name, archs[k], x.numpy(), ei, masks) for k in KINDS}
        else:
            hs = {k: _rows(name, C) for k in KINDS}
        refs = {k: outputs(name, archs[k], hs[k], masks) for k in KINDS}
        if all(sensitive(refs[k], k, c) for k in KINDS):
            return {"name": name, "S": S, "x": x, "ei": ei, "w": w, "ea": ea, "masks": masks, "C": C,
                    "arch": archs[out], "ref": refs[out], "c": c, "head_scale": s, "kind": out,
                    "queries": [0] if name == "pooled-mean" else QUERIES}
    raise AssertionError(f"{name}, C = {C}: no head scale makes the reference sensitive to the class")
