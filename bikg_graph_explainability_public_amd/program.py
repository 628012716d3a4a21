"""Compile a black-box GNN `arch` (nn.Module) into the engine's layer program.

The reference treats `arch` as a black box and calls `arch(feat, edge_index)` on the B-fold
union graph (model.py:62-116).  The engine instead recognises the supported module family —
GCNConv / SAGEConv (mean, add, max) / GraphConv / GINConv / HeteroConv(sum) conv layers, stacks of RGCNConv / FastRGCNConv on a
typed-edge graph (and, with `attention=True`, GATConv, GATv2Conv and TransformerConv),
each optionally followed by an elementwise activation, then Linear layers with activations (the
layout of tests/test_utils.py:10-83 and the notebooks) — and lowers it to:

    ConvLayer(terms=[(kind, relation, W_k)], bias_sum, act)   per conv layer
    HeadLayer(W, b, act)                                       per Linear

Blocks `[conv norm? act?]+ [Linear norm? act?]*`: a BatchNorm1d in eval mode folds into the linear
map before it where that map is the last thing the layer does (every term kind but attention, the
first Linear of a GINConv MLP, a head Linear); after an attention layer it becomes the layer's
post-op affine, a torch.nn.LayerNorm after a conv the post-op's norm (ConvLayer.post, PostOp).
nn.BlockStack(residual=True), matched by class name, adds the skip to the post-op.

Multi-node-type graphs (HeteroConv over relations (src, rel, dst) between several node types,
model.py:118-253): every term carries its relation's destination type (the engine applies it
only to targets of that type), SAGE root weights and biases are summed per destination type,
and layer-1 weights are zero-padded to the widest input (the homogenised features are padded the
same way, data.py:825-878).  The head reads the first output node type of the last HeteroConv
(the `x[list(x.keys())[0]]` convention of the reference's hetero archs, tests/test_utils.py:176-178).

Modules are matched by class name + attributes, so both torch_geometric 2.0.4 modules and
bikg_graph_explainability_public_amd.nn modules compile.  Anything else raises
UnsupportedArch (callers then use the generic torch path, model.py).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import torch
from torch import nn


class UnsupportedArch(ValueError):
    pass


@dataclass
class Term:
    kind: str          # "gcn" | "mean" | "sum" | "max" | "root" | "att" | "rel" | "att2" | "qkv"
    rel: int           # relation index (ignored for root and rel)
    weight: torch.Tensor  # [f_out, f_in] (att: W_src, [heads * head_ch, f_in]; rel: [slices, f_out, f_in])
    dst_type: int = -1    # multi-node-type: destination node type of the relation
    # kind "att" (GATConv, PyG 2.0.4): one term per relation
    heads: int = 1
    head_ch: int = 0
    att_src: Optional[torch.Tensor] = None     # [heads, head_ch]
    att_dst: Optional[torch.Tensor] = None     # [heads, head_ch]
    weight_dst: Optional[torch.Tensor] = None  # bipartite relations: W_dst; None: W_src for both ends
    neg_slope: float = 0.2
    self_loops: bool = False
    # kind "att2" (GATv2Conv, PyG 2.0.4): one term per relation; weight = W_l, heads / head_ch /
    # neg_slope / self_loops as for "att"
    weight_r: Optional[torch.Tensor] = None    # W_r [heads * head_ch, f_in]; None: shared (W_l)
    bias_l: Optional[torch.Tensor] = None      # lin_l.bias [heads * head_ch] (inside the messages)
    bias_r: Optional[torch.Tensor] = None      # lin_r.bias
    att: Optional[torch.Tensor] = None         # [heads, head_ch]
    # kind "qkv" (TransformerConv, PyG 2.0.4): one term per relation; weight = W_key, bias_l =
    # lin_key.bias, heads / head_ch as for "att"; the logit of (u -> t) is <Q[t], K[u]> / sqrt(head_ch),
    # the messages are rows of V; the edge set is the given edges (self_loops False)
    weight_v: Optional[torch.Tensor] = None    # lin_value.weight [heads * head_ch, f_in]
    weight_q: Optional[torch.Tensor] = None    # lin_query.weight
    weight_s: Optional[torch.Tensor] = None    # lin_skip.weight; None: root_weight=False
    bias_v: Optional[torch.Tensor] = None
    bias_q: Optional[torch.Tensor] = None
    bias_s: Optional[torch.Tensor] = None      # lin_skip.bias (None with bias=False)
    # the gate of beta=True, sigmoid(<gate_out, out> + <gate_r, x_r>): lin_beta.weight = [w1 | w2 |
    # w3] over [out, x_r, out - x_r] folded to gate_out = w1 + w3, gate_r = w2 - w3 (fp64, rounded
    # once); both None: out + x_r
    gate_out: Optional[torch.Tensor] = None    # [heads * head_ch]
    gate_r: Optional[torch.Tensor] = None
    # kind "rel" (RGCNConv / FastRGCNConv, PyG 2.0.4): one term per conv layer, over every edge
    # type of the graph.  Per relation r the mean (norm "mean": over that relation's kept in-edges,
    # 0 without one) or sum (norm "sum") A_r of the source rows; the term adds sum_s B_s weight[s]^T
    # with B_s = A_s (coef None: slices == num_relations, weight[r] = W_r^T, block-diagonal weights
    # expanded) or B_s = sum_r coef[r, s] A_r (basis decomposition: weight[s] = V_s^T, coef = comp)
    num_relations: int = 0
    norm: str = "mean"
    slices: int = 0
    coef: Optional[torch.Tensor] = None        # [num_relations, slices]
    # kind "sum" of a GINEConv (PyG 2.0.4; programs marked `edge_featured`): the messages are
    # relu(x_j + e_ji) with e = edge_attr edge_lin_w^T + edge_lin_b (GINEConv.lin; both None with
    # edge_dim=None: the attribute rows themselves, of the layer's input width)
    edge_lin_w: Optional[torch.Tensor] = None  # [f_in, D]
    edge_lin_b: Optional[torch.Tensor] = None  # [f_in]


@dataclass
class PostOp:
    """What follows a conv layer's bias, row by row (xpgnn.h, xpg_post_desc), in this order:
    v * scale + shift, the norm (v - mean) / sqrt(var + eps) * gamma + beta over the f_out columns,
    act, + the target's own input row (residual).  fp32 [f_out] tensors; None = 1 / 0 / no norm."""
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    norm: Optional[str] = None          # None | "layer"
    gamma: Optional[torch.Tensor] = None
    beta: Optional[torch.Tensor] = None
    eps: float = 0.0
    act: Optional[str] = None
    residual: bool = False


@dataclass
class ConvLayer:
    terms: List[Term]
    bias: torch.Tensor    # [f_out] (sum over relations); multi-node-type: [n_types, f_out]
    act: Optional[str]    # None when `post` is set: the activation is the post-op's
    f_in: int
    f_out: int
    post: Optional[PostOp] = None


@dataclass
class HeadLayer:
    weight: torch.Tensor  # [n, k]
    bias: Optional[torch.Tensor]
    act: Optional[str]


@dataclass
class ModelProgram:
    convs: List[ConvLayer] = field(default_factory=list)
    head: List[HeadLayer] = field(default_factory=list)
    out_col: int = 0
    n_types: int = 1               # > 1: multi-node-type program (node-type-gated terms)
    out_type: Optional[int] = None  # multi-node-type: node type whose rows feed the head
    link_act: Optional[str] = None  # LinkModel: the program is its encoder; decoder act(<z_u, z_v>)
    # RelLinkModel's DistMult decoder: fp32 [num_relations, C] relation embeddings, the score of a
    # type-r edge is act(sum_f z_u[f] link_rel[r][f] z_v[f]); None: the plain dot product
    link_rel: Optional[torch.Tensor] = None
    # ROOT-only conv layers that are the second Linear of a GINConv MLP: no message passing of
    # their own (the module's hop count, count_message_passing, does not include them)
    extra_layers: int = 0
    # PooledModel: the convs are its encoder's, the head its `fc`; between them each graph's node
    # rows reduce to one row ("mean" | "sum" | "max"), and the program has one output per graph
    pool: Optional[str] = None
    # compiled for a weighted graph (compile_arch(edge_weight=True)): every conv is a GCNConv or a
    # GraphConv, the two convs of PyG 2.0.4 that take an edge_weight; the plan then needs the weights
    weighted: bool = False
    # compiled for a graph with edge features (compile_arch(edge_attr=True)): every conv is a
    # GINEConv; the plan then needs the attribute rows
    edge_featured: bool = False
    # a classifier's last unit, nn.Softmax / nn.LogSoftmax over the class dimension: None |
    # "softmax" | "log_softmax" over the columns of the last head layer (headless: the last conv),
    # which then carries no activation of its own; the class readout (xpgnn.h, xpg_class_out)
    out_norm: Optional[str] = None

    @property
    def n_classes(self):
        """Output columns C: the last head layer's, or the last conv's of a headless program."""
        return int(self.head[-1].weight.shape[0]) if self.head else int(self.convs[-1].f_out)

    @property
    def hops(self):
        return len(self.convs) - self.extra_layers

    @property
    def has_post(self):
        return any(c.post is not None for c in self.convs)


_ACTS = {"ReLU": "relu", "Sigmoid": "sigmoid", "Tanh": "tanh", "ELU": "elu",
         "LeakyReLU": "leaky_relu"}
_SKIP = {"Dropout", "Identity", "AlphaDropout"}


def _act_name(m):
    name = type(m).__name__
    if name not in _ACTS:
        return None
    if name == "LeakyReLU" and abs(getattr(m, "negative_slope", 0.01) - 0.01) > 0:
        raise UnsupportedArch("LeakyReLU(negative_slope != 0.01)")
    if name == "ELU" and getattr(m, "alpha", 1.0) != 1.0:
        raise UnsupportedArch("ELU(alpha != 1)")
    return _ACTS[name]


_OUT_NORMS = {"Softmax": "softmax", "LogSoftmax": "log_softmax"}


def _is_out_norm(m):
    return type(m).__name__ in _OUT_NORMS and hasattr(m, "dim")


def _is_gat(m):
    return type(m).__name__ == "GATConv" and all(
        hasattr(m, a) for a in ("lin_src", "lin_dst", "att_src", "att_dst", "heads", "out_channels"))


def _is_gatv2(m):
    return type(m).__name__ == "GATv2Conv" and all(
        hasattr(m, a) for a in ("lin_l", "lin_r", "att", "heads", "out_channels"))


def _is_transformer(m):
    return type(m).__name__ == "TransformerConv" and all(
        hasattr(m, a) for a in ("lin_key", "lin_query", "lin_value", "heads", "out_channels"))


def _is_graphconv(m):
    return type(m).__name__ == "GraphConv" and hasattr(m, "lin_rel") and hasattr(m, "lin_root")


def _is_gin(m):
    return type(m).__name__ == "GINConv" and hasattr(m, "nn") and hasattr(m, "eps")


def _is_gine(m):
    return type(m).__name__ == "GINEConv" and hasattr(m, "nn") and hasattr(m, "eps") and hasattr(m, "lin")


_RGCN_NAMES = ("RGCNConv", "FastRGCNConv")


def _is_rgcn(m):
    return type(m).__name__ in _RGCN_NAMES and hasattr(m, "weight") and hasattr(m, "num_relations")


def _is_conv(m, attention=False):
    return type(m).__name__ in ("GCNConv", "SAGEConv", "HeteroConv") or _is_graphconv(m) or _is_gin(m) \
        or _is_gine(m) or _is_rgcn(m) or (attention and (_is_gat(m) or _is_gatv2(m) or _is_transformer(m)))


def _is_linear(m):
    return type(m).__name__ == "Linear" and hasattr(m, "weight")


def _is_bn(m):
    return type(m).__name__ == "BatchNorm1d" and hasattr(m, "running_mean") and hasattr(m, "eps")


def _is_ln(m):
    return type(m).__name__ == "LayerNorm"


def _is_norm(m):
    return _is_bn(m) or _is_ln(m)


def _bn_affine(bn, width):
    """BatchNorm1d in eval mode as the per-column affine v * s + t, s = gamma / sqrt(var + eps),
    t = beta - mean * s (fp64).  Training mode or no running statistics: its statistics would be
    those of the whole B-fold union graph."""
    if bn.training:
        raise UnsupportedArch("BatchNorm1d in training mode (batch statistics over the union graph)")
    if not getattr(bn, "track_running_stats", True) or bn.running_mean is None or bn.running_var is None:
        raise UnsupportedArch("BatchNorm1d without running statistics")
    if int(bn.num_features) != int(width):
        raise UnsupportedArch(f"BatchNorm1d({bn.num_features}) after a layer of width {width}")
    s = (bn.running_var.detach().double() + float(bn.eps)).rsqrt()
    if getattr(bn, "weight", None) is not None:
        s = s * bn.weight.detach().double()
    t = -bn.running_mean.detach().double() * s
    if getattr(bn, "bias", None) is not None:
        t = t + bn.bias.detach().double()
    return s, t


def _fold_rows(w, s):
    """diag(s) w, in fp64 and rounded once; the leading dimensions of `w` are kept."""
    return (s.reshape(-1, 1) * w.detach().double()).to(torch.float32)


def _fold_bias(b, s, t, width):
    b = torch.zeros(width, dtype=torch.float64) if b is None else b.detach().double()
    return (s * b + t).to(torch.float32)


def _layer_norm_post(ln, width):
    if not isinstance(ln, nn.LayerNorm):
        raise UnsupportedArch(f"a LayerNorm that is not torch.nn.LayerNorm ({type(ln).__module__})")
    shape = tuple(ln.normalized_shape)
    if len(shape) != 1 or int(shape[0]) != int(width):
        raise UnsupportedArch(f"LayerNorm{shape} after a layer of width {width} (last dimension only)")
    return PostOp(norm="layer", eps=float(ln.eps),
                  gamma=_f32(ln.weight) if getattr(ln, "weight", None) is not None else None,
                  beta=_f32(ln.bias) if getattr(ln, "bias", None) is not None else None)


_FOLD_KINDS = ("gcn", "mean", "sum", "max", "root")


def _norm_conv_layer(layer, norm):
    """Apply the norm module that follows conv layer `layer` (before its activation): fold, or a
    post-op that takes the activation with it."""
    kinds = {t.kind for t in layer.terms}
    if "rel" in kinds:
        raise UnsupportedArch(f"{type(norm).__name__} after RGCNConv")
    if layer.bias.dim() != 1:
        raise UnsupportedArch(f"{type(norm).__name__} on a multi-node-type graph")
    if _is_bn(norm):
        s, t = _bn_affine(norm, layer.f_out)
        if kinds <= set(_FOLD_KINDS):
            # the layer ends in its linear maps: sum_k (diag(s) W_k) agg_k + (s b + t); the
            # aggregations (max included) come before them, so the sign of s does not matter
            for term in layer.terms:
                term.weight = _fold_rows(term.weight, s)
            layer.bias = _fold_bias(layer.bias, s, t, layer.f_out)
            return
        # attention: the scores read the transformed rows, which must stay as they are
        layer.post = PostOp(scale=s.to(torch.float32), shift=t.to(torch.float32), act=layer.act)
    else:
        layer.post = _layer_norm_post(norm, layer.f_out)
        layer.post.act = layer.act
    layer.act = None


def _leaf_units(module, attention=False):
    """Registration-order walk yielding conv / linear / norm / activation units (convs not entered)."""
    for child in module.children():
        if _is_gatv2(child) and not attention:
            raise UnsupportedArch("GATv2Conv without the attention opt-in (attention=True)")
        if _is_transformer(child) and not attention:
            raise UnsupportedArch("TransformerConv without the attention opt-in (attention=True)")
        if _is_conv(child, attention) or _is_linear(child) or _act_name(child) is not None \
                or _is_norm(child) or _is_out_norm(child):
            yield child
        elif type(child).__name__ in _SKIP:
            continue
        elif len(list(child.children())) == 0:
            if any(True for _ in child.parameters(recurse=False)):
                raise UnsupportedArch(f"unsupported parameterised module {type(child).__name__}")
            continue
        else:
            yield from _leaf_units(child, attention)


def _f32(t):
    return t.detach().to(torch.float32)


def _gat_terms(conv, rel, bipartite):
    """One GATConv relation as an "att" term.  A same-type relation is handed a Tensor by
    HeteroConv and 2.0.4 then transforms both ends with lin_src, even when a separate lin_dst
    exists; lin_dst is used by bipartite relations only."""
    H, C = int(conv.heads), int(conv.out_channels)
    concat = bool(getattr(conv, "concat", True))
    if not concat and H > 1:
        raise UnsupportedArch("GATConv(concat=False) with several heads")
    if getattr(conv, "edge_dim", None) is not None or getattr(conv, "lin_edge", None) is not None:
        raise UnsupportedArch("GATConv with edge_dim")
    for lin in (conv.lin_src, conv.lin_dst):
        if isinstance(getattr(lin, "weight", None), nn.parameter.UninitializedParameter):
            raise UnsupportedArch("GATConv with uninitialised (lazy) weights")
        if getattr(lin, "bias", None) is not None:
            raise UnsupportedArch("GATConv.lin_src / lin_dst with bias")
    W = _f32(conv.lin_src.weight)
    if W.shape[0] != H * C:
        raise UnsupportedArch("GATConv weight shape does not match heads * out_channels")
    Wd = None
    if bipartite and conv.lin_dst is not conv.lin_src:
        Wd = _f32(conv.lin_dst.weight)
        if Wd.shape[0] != H * C:
            raise UnsupportedArch("GATConv lin_dst shape does not match heads * out_channels")
    b = _f32(conv.bias) if getattr(conv, "bias", None) is not None else None
    term = Term("att", rel, W, heads=H, head_ch=C,
                att_src=_f32(conv.att_src).reshape(H, C), att_dst=_f32(conv.att_dst).reshape(H, C),
                weight_dst=Wd, neg_slope=float(getattr(conv, "negative_slope", 0.2)),
                self_loops=bool(getattr(conv, "add_self_loops", True)))
    return [term], b, None, W.shape[1], H * C


def _gatv2_terms(conv, rel, bipartite):
    """One GATv2Conv relation as an "att2" term: W_l / b_l (the messages), W_r / b_r (None when the
    conv shares lin_l), att [heads, head_ch]; the conv's own bias is the layer's."""
    H, C = int(conv.heads), int(conv.out_channels)
    if not bool(getattr(conv, "concat", True)) and H > 1:
        raise UnsupportedArch("GATv2Conv(concat=False) with several heads")
    if getattr(conv, "edge_dim", None) is not None or getattr(conv, "lin_edge", None) is not None:
        raise UnsupportedArch("GATv2Conv with edge_dim")
    if (H * C + 31) // 32 * 32 > 256:
        raise UnsupportedArch("GATv2Conv wider than 256 columns (heads * out_channels, padded to 32)")
    if bipartite or not isinstance(getattr(conv, "in_channels", 0), int):
        raise UnsupportedArch("GATv2Conv on a bipartite relation / with tuple in_channels")
    if _lazy(conv.lin_l) or _lazy(conv.lin_r):
        raise UnsupportedArch("GATv2Conv with uninitialised (lazy) weights")
    shared = conv.lin_r is conv.lin_l
    Wl = _f32(conv.lin_l.weight)
    Wr = None if shared else _f32(conv.lin_r.weight)
    if Wl.shape[0] != H * C or (Wr is not None and Wr.shape != Wl.shape):
        raise UnsupportedArch("GATv2Conv weight shape does not match heads * out_channels")
    if tuple(conv.att.shape)[-2:] != (H, C) or conv.att.numel() != H * C:
        raise UnsupportedArch("GATv2Conv att shape does not match heads x out_channels")
    bl = _f32(conv.lin_l.bias) if getattr(conv.lin_l, "bias", None) is not None else None
    br = bl if shared else \
        (_f32(conv.lin_r.bias) if getattr(conv.lin_r, "bias", None) is not None else None)
    b = _f32(conv.bias) if getattr(conv, "bias", None) is not None else None
    term = Term("att2", rel, Wl, heads=H, head_ch=C, weight_r=Wr, bias_l=bl, bias_r=br,
                att=_f32(conv.att).reshape(H, C),
                neg_slope=float(getattr(conv, "negative_slope", 0.2)),
                self_loops=bool(getattr(conv, "add_self_loops", True)))
    return [term], b, None, Wl.shape[1], H * C


def _transformer_terms(conv, rel, bipartite):
    """One TransformerConv relation as a "qkv" term: the key / value / query maps with their biases,
    the skip map when root_weight, and the beta gate folded to two vectors.  The conv has no bias
    of its own, so the layer's is None."""
    H, C = int(conv.heads), int(conv.out_channels)
    if not bool(getattr(conv, "concat", True)) and H > 1:
        raise UnsupportedArch("TransformerConv(concat=False) with several heads")
    if getattr(conv, "edge_dim", None) is not None or getattr(conv, "lin_edge", None) is not None:
        raise UnsupportedArch("TransformerConv with edge_dim")
    if (H * C + 31) // 32 * 32 > 256:
        raise UnsupportedArch("TransformerConv wider than 256 columns (heads * out_channels, padded to 32)")
    if bipartite or not isinstance(getattr(conv, "in_channels", 0), int):
        raise UnsupportedArch("TransformerConv on a bipartite relation / with tuple in_channels")
    root = bool(getattr(conv, "root_weight", True))
    lins = [conv.lin_key, conv.lin_value, conv.lin_query] + ([conv.lin_skip] if root else [])
    if any(_lazy(lin) for lin in lins):
        raise UnsupportedArch("TransformerConv with uninitialised (lazy) weights")
    Ws = [_f32(lin.weight) for lin in lins]
    if any(W.shape != (H * C, Ws[0].shape[1]) for W in Ws):
        raise UnsupportedArch("TransformerConv weight shape does not match heads * out_channels")
    bs = [_f32(lin.bias) if getattr(lin, "bias", None) is not None else None for lin in lins]
    g_out = g_r = None
    lin_beta = getattr(conv, "lin_beta", None) if root and getattr(conv, "beta", False) else None
    if lin_beta is not None:
        if _lazy(lin_beta):
            raise UnsupportedArch("TransformerConv with uninitialised (lazy) weights")
        if tuple(lin_beta.weight.shape) != (1, 3 * H * C) or getattr(lin_beta, "bias", None) is not None:
            raise UnsupportedArch("TransformerConv lin_beta is not Linear(3 * heads * out_channels, 1, bias=False)")
        w1, w2, w3 = lin_beta.weight.detach().double().reshape(3, H * C)
        g_out, g_r = (w1 + w3).to(torch.float32), (w2 - w3).to(torch.float32)
    term = Term("qkv", rel, Ws[0], heads=H, head_ch=C, bias_l=bs[0], weight_v=Ws[1], bias_v=bs[1],
                weight_q=Ws[2], bias_q=bs[2], weight_s=Ws[3] if root else None,
                bias_s=bs[3] if root else None, gate_out=g_out, gate_r=g_r, self_loops=False)
    return [term], None, None, Ws[0].shape[1], H * C


def fold_attention(term):
    """The attention vectors of an "att" term folded through its weights: (v_s, v_d), each
    [heads, f_in], with v_s[h] = W_src[hC:(h+1)C, :]^T att_src[h] (v_d likewise, with W_dst for
    bipartite relations), so that v_s[h] . x == att_src[h] . (W_src x)[hC:(h+1)C]: the scores of
    layer-input rows without the transformed rows.  Pure torch, any device / dtype."""
    H, C = term.heads, term.head_ch
    Ws = term.weight
    Wd = term.weight_dst if term.weight_dst is not None else Ws
    att_s = term.att_src.to(Ws.dtype).to(Ws.device)
    att_d = term.att_dst.to(Wd.dtype).to(Wd.device)
    v_s = torch.einsum("hcf,hc->hf", Ws.reshape(H, C, -1), att_s)
    v_d = torch.einsum("hcf,hc->hf", Wd.reshape(H, C, -1), att_d)
    return v_s, v_d


def stack_attention(terms, f_in_pad, f_out_pad):
    """The dense weight and padded score vectors of an all-"att" layer past the first, which
    keeps the engine's aggregate-then-transform form: the layer's dense input holds one
    f_in_pad-wide slice per (term, head), slice (k, h) = sum_e alpha_e^h (input row of e's
    source), and Wc [f_out_pad, slices * f_in_pad] has W_src[hC:(h+1)C, :] in rows hC..(h+1)C of
    slice (k, h) and zeros elsewhere, so Wc times the slices equals the per-head transform of the
    aggregates (= aggregating the transformed rows).  Returns (Wc, [(v_s, v_d)] per term, each
    [heads, f_in_pad], zero-padded `fold_attention` vectors).  Pure torch, dtype of the weights."""
    n_sl = sum(t.heads for t in terms)
    W0 = terms[0].weight
    wc = torch.zeros((f_out_pad, n_sl * f_in_pad), dtype=W0.dtype, device=W0.device)
    vecs, sl = [], 0
    for term in terms:
        C, W = term.head_ch, term.weight
        f_in = W.shape[1]
        for h in range(term.heads):
            wc[h * C:(h + 1) * C, sl * f_in_pad:sl * f_in_pad + f_in] = W[h * C:(h + 1) * C]
            sl += 1
        pair = []
        for v in fold_attention(term):
            vp = torch.zeros((term.heads, f_in_pad), dtype=v.dtype, device=v.device)
            vp[:, :f_in] = v
            pair.append(vp)
        vecs.append(tuple(pair))
    return wc, vecs


def _check_unmixed(terms):
    for kind, name in (("att", "GATConv"), ("att2", "GATv2Conv"), ("qkv", "TransformerConv")):
        if any(t.kind == kind for t in terms) and not all(t.kind == kind for t in terms):
            raise UnsupportedArch(f"a conv layer mixing {name} with other relations")


_AGGR_KIND = {"mean": "mean", "add": "sum", "sum": "sum", "max": "max"}


def _aggr_kind(conv, default):
    aggr = getattr(conv, "aggr", default)
    if not isinstance(aggr, str) or aggr not in _AGGR_KIND:
        raise UnsupportedArch(f"{type(conv).__name__}(aggr={aggr!r})")
    return _AGGR_KIND[aggr]


def _lazy(lin):
    return isinstance(getattr(lin, "weight", None), nn.parameter.UninitializedParameter)


def _gin_terms(conv, rel):
    """GINConv: nn((1 + eps) x + sum_j x_j).  nn = Linear(W, b): a "sum" term W, the root
    (1 + eps) W and bias b.  nn = Sequential(Linear, act, Linear[, act]): that layer with the
    inner activation, then (returned as `extra`) the second Linear and the trailing activation
    (None: the one that follows the conv) for a ROOT-only layer.  A BatchNorm1d (eval mode)
    between the first Linear and the inner activation folds into that Linear."""
    eps = conv.eps
    eps = float(eps.detach().reshape(-1)[0]) if isinstance(eps, torch.Tensor) else float(eps)
    mlp = conv.nn
    extra = bn = None
    if _is_linear(mlp):
        lin = mlp
    else:
        units = [m for m in mlp.children() if type(m).__name__ not in _SKIP] \
            if type(mlp).__name__ == "Sequential" else []
        shape = [("L" if _is_linear(m) else "A" if _act_name(m) is not None else
                  "N" if _is_bn(m) else "?") for m in units]
        if "".join(shape) not in ("LAL", "LALA", "LNAL", "LNALA"):
            raise UnsupportedArch("GINConv.nn other than Linear or Sequential(Linear, [BatchNorm1d,] "
                                  "act, Linear[, act])")
        lin = units[0]
        if shape[1] == "N":
            bn, units = units[1], units[:1] + units[2:]
        extra = (units[2], _act_name(units[1]), _act_name(units[3]) if len(units) == 4 else None)
    if _lazy(lin) or (extra is not None and _lazy(extra[0])):
        raise UnsupportedArch("GINConv.nn with uninitialised (lazy) weights")
    W = _f32(lin.weight)
    b = _f32(lin.bias) if getattr(lin, "bias", None) is not None else None
    root = ((1.0 + eps) * lin.weight.detach().double()).to(torch.float32)  # folded in fp64, rounded once
    if bn is not None:
        s, t = _bn_affine(bn, W.shape[0])
        root = _fold_rows((1.0 + eps) * lin.weight.detach().double(), s)
        W, b = _fold_rows(W, s), _fold_bias(b, s, t, W.shape[0])
    return [Term("sum", rel, W)], b, root, W.shape[1], W.shape[0], extra


def _gine_terms(conv, rel):
    """GINEConv: _gin_terms' lowering (the same MLP shapes, root and BatchNorm folds); the "sum"
    term carries the edge map GINEConv.lin (None with edge_dim=None)."""
    out = _gin_terms(conv, rel)
    term, f_in = out[0][0], out[3]
    lin = getattr(conv, "lin", None)
    if lin is not None:
        if _lazy(lin):
            raise UnsupportedArch("GINEConv.lin with uninitialised (lazy) weights")
        w = _f32(lin.weight)
        if w.dim() != 2 or w.shape[0] != f_in:
            raise UnsupportedArch(f"GINEConv.lin of {tuple(w.shape)} on an input of width {f_in}")
        term.edge_lin_w = w
        term.edge_lin_b = _f32(lin.bias) if getattr(lin, "bias", None) is not None else torch.zeros(f_in)
    return out


_REL_NORM = {"mean": "mean", "add": "sum", "sum": "sum"}


def _rgcn_terms(conv):
    """RGCNConv / FastRGCNConv as one "rel" term (+ root weight and bias).  W_r is [in, out] in
    the module; the term holds the transposes.  Folds (the block-diagonal expansion) are done in
    fp64 and rounded once."""
    name = type(conv).__name__
    aggr = getattr(conv, "aggr", "mean")
    if not isinstance(aggr, str) or aggr not in _REL_NORM:
        raise UnsupportedArch(f"{name}(aggr={aggr!r})")
    w = conv.weight
    if isinstance(w, nn.parameter.UninitializedParameter) or \
            isinstance(getattr(conv, "root", None), nn.parameter.UninitializedParameter):
        raise UnsupportedArch(f"{name} with uninitialised (lazy) weights")
    R = int(conv.num_relations)
    nb, nk = getattr(conv, "num_bases", None), getattr(conv, "num_blocks", None)
    w = w.detach().double()
    coef = None
    if nb is not None:
        comp = getattr(conv, "comp", None)
        if comp is None or w.dim() != 3 or tuple(comp.shape) != (R, w.shape[0]):
            raise UnsupportedArch(f"{name}: comp does not match num_relations x num_bases")
        coef = _f32(comp).contiguous()
        W = w.transpose(1, 2)                                  # [B, out, in]
    elif nk is not None:
        if w.dim() != 4 or w.shape[0] != R:
            raise UnsupportedArch(f"{name}: block weight shape")
        W = torch.stack([torch.block_diag(*w[r]) for r in range(R)]).transpose(1, 2)
    else:
        if w.dim() != 3 or w.shape[0] != R:
            raise UnsupportedArch(f"{name}: weight shape does not match num_relations")
        W = w.transpose(1, 2)                                  # [R, out, in]
    W = W.to(torch.float32).contiguous()
    root = getattr(conv, "root", None)
    root = _f32(root).t().contiguous() if root is not None else None
    if root is not None and tuple(root.shape) != tuple(W.shape[1:]):
        raise UnsupportedArch(f"{name}: root shape does not match the relation weights (bipartite input)")
    b = _f32(conv.bias) if getattr(conv, "bias", None) is not None else None
    term = Term("rel", -1, W, num_relations=R, norm=_REL_NORM[aggr], slices=int(W.shape[0]), coef=coef)
    return [term], b, root, int(W.shape[2]), int(W.shape[1])


def relation_weights(term):
    """The dense effective weights [num_relations, f_out, f_in] of a "rel" term: its own, or the
    bases folded with their coefficients in fp64 and rounded once (layer-1 tables)."""
    if term.coef is None:
        return term.weight
    return torch.einsum("rb,boi->roi", term.coef.double(), term.weight.double()).to(torch.float32)


def check_rel_features(prog, feat):
    """Featureless RGCN (node indices in place of a feature matrix) has no lowering."""
    if any(t.kind == "rel" for c in prog.convs for t in c.terms) and \
            (feat is None or not torch.is_floating_point(feat)):
        raise UnsupportedArch("featureless RGCNConv (x as node indices)")


def _single_conv_terms(conv, rel, attention=False, bipartite=False):
    name = type(conv).__name__
    if _is_rgcn(conv):
        raise UnsupportedArch(f"{name} inside HeteroConv")
    if attention and _is_gat(conv):
        return _gat_terms(conv, rel, bipartite)
    if attention and _is_gatv2(conv):
        return _gatv2_terms(conv, rel, bipartite)
    if attention and _is_transformer(conv):
        return _transformer_terms(conv, rel, bipartite)
    if name == "GCNConv":
        if getattr(conv, "improved", False) or not getattr(conv, "add_self_loops", True) \
                or not getattr(conv, "normalize", True):
            raise UnsupportedArch("GCNConv with improved/add_self_loops=False/normalize=False")
        W = _f32(conv.lin.weight)
        if getattr(conv.lin, "bias", None) is not None:
            raise UnsupportedArch("GCNConv.lin with bias")
        b = _f32(conv.bias) if getattr(conv, "bias", None) is not None else None
        return [Term("gcn", rel, W)], b, None, W.shape[1], W.shape[0]
    if name == "SAGEConv":
        if getattr(conv, "normalize", False) or not getattr(conv, "root_weight", True) \
                or getattr(conv, "project", False):
            raise UnsupportedArch("SAGEConv with normalize / project / root_weight=False")
        kind = _aggr_kind(conv, "mean")
        Wl = _f32(conv.lin_l.weight)
        bl = _f32(conv.lin_l.bias) if getattr(conv.lin_l, "bias", None) is not None else None
        Wr = _f32(conv.lin_r.weight)
        return [Term(kind, rel, Wl)], bl, Wr, Wl.shape[1], Wl.shape[0]
    if _is_graphconv(conv):
        if getattr(conv.lin_root, "bias", None) is not None:
            raise UnsupportedArch("GraphConv.lin_root with bias")
        if _lazy(conv.lin_rel) or _lazy(conv.lin_root):
            raise UnsupportedArch("GraphConv with uninitialised (lazy) weights")
        kind = _aggr_kind(conv, "add")
        W = _f32(conv.lin_rel.weight)
        b = _f32(conv.lin_rel.bias) if getattr(conv.lin_rel, "bias", None) is not None else None
        return [Term(kind, rel, W)], b, _f32(conv.lin_root.weight), W.shape[1], W.shape[0]
    if _is_gine(conv):
        raise UnsupportedArch("GINEConv inside HeteroConv")
    if _is_gin(conv):
        t, b, root, f_in, f_out, extra = _gin_terms(conv, rel)
        if extra is not None:
            raise UnsupportedArch("GINConv with an MLP inside HeteroConv")
        return t, b, root, f_in, f_out
    raise UnsupportedArch(f"unsupported conv {name}")


def _conv_layer(conv, rel_index, attention=False):
    """Lower one conv (or HeteroConv) to terms.  rel_index maps edge-type tuples to relations."""
    if type(conv).__name__ == "HeteroConv":
        if getattr(conv, "aggr", "sum") != "sum":
            raise UnsupportedArch("HeteroConv(aggr != 'sum')")
        if rel_index is None:
            raise UnsupportedArch("HeteroConv on a homogeneous graph")
        terms, bias, root = [], None, None
        f_in = f_out = None
        for key, sub in conv.convs.items():
            et = tuple(key.split("__"))
            if et not in rel_index:
                continue  # relation absent from the graph: HeteroConv skips it too
            if et[0] != et[-1]:
                raise UnsupportedArch("bipartite relations need the multi-node-type path")
            t, b, wr, fi, fo = _single_conv_terms(sub, rel_index[et], attention)
            if f_out is not None and fo != f_out and \
                    (t[0].kind in ("att", "att2", "qkv") or terms[0].kind in ("att", "att2", "qkv")):
                raise UnsupportedArch("HeteroConv relations with different output widths")
            terms += t
            if b is not None:
                bias = b.clone() if bias is None else bias + b
            if wr is not None:
                root = wr.clone() if root is None else root + wr
            f_in, f_out = fi, fo
        if not terms:
            raise UnsupportedArch("HeteroConv with no relation present in the graph")
    elif _is_rgcn(conv):
        # typed edges: the relations are the conv's own (edge_type), whatever the graph names
        terms, bias, root, f_in, f_out = _rgcn_terms(conv)
    else:
        if rel_index is not None and len(rel_index) != 1:
            raise UnsupportedArch("homogeneous conv on a multi-relation graph")
        if _is_gin(conv) or _is_gine(conv):
            terms, bias, root, f_in, f_out, extra = (_gine_terms if _is_gine(conv) else _gin_terms)(conv, 0)
            if extra is not None:
                terms.append(Term("root", -1, root))
                return terms, (torch.zeros(f_out) if bias is None else bias), f_in, f_out, extra
        else:
            terms, bias, root, f_in, f_out = _single_conv_terms(conv, 0, attention)
    _check_unmixed(terms)
    if root is not None:
        terms.append(Term("root", -1, root))
    if bias is None:
        bias = torch.zeros(f_out)
    return terms, bias, f_in, f_out, None


def _pad_cols(w, n):
    return w if w.shape[1] == n else torch.nn.functional.pad(w, (0, n - w.shape[1]))


def _conv_layer_multi(conv, rel_index, node_type_names, attention=False):
    """HeteroConv over several node types: terms gated by destination type, SAGE root weights
    and biases summed per destination type.  Returns (terms, bias [n_types, f_out], f_in, f_out,
    destination type of the first present relation)."""
    if type(conv).__name__ != "HeteroConv" or getattr(conv, "aggr", "sum") != "sum":
        raise UnsupportedArch("multi-node-type graphs need HeteroConv(aggr='sum') layers")
    nt = len(node_type_names)
    terms, roots, biases = [], {}, {}
    f_out, first_dst, f_ins = None, None, []
    for key, sub in conv.convs.items():
        et = tuple(key.split("__"))
        if et not in rel_index:
            continue
        s_t, d_t = node_type_names.index(et[0]), node_type_names.index(et[-1])
        if type(sub).__name__ == "GCNConv" and s_t != d_t:
            raise UnsupportedArch("GCNConv on a bipartite relation")
        if _is_gatv2(sub):
            raise UnsupportedArch("GATv2Conv on a multi-node-type graph")
        if _is_transformer(sub):
            raise UnsupportedArch("TransformerConv on a multi-node-type graph")
        t, b, wr, fi, fo = _single_conv_terms(sub, rel_index[et], attention, s_t != d_t)
        if t[0].kind == "att" and t[0].self_loops:
            raise UnsupportedArch("GATConv(add_self_loops=True) on a multi-node-type graph")
        if f_out is not None and fo != f_out:
            raise UnsupportedArch("HeteroConv relations with different output widths")
        f_out = fo
        first_dst = d_t if first_dst is None else first_dst
        for term in t:
            term.dst_type = d_t
            f_ins.append(term.weight.shape[1])
            if term.weight_dst is not None:
                f_ins.append(term.weight_dst.shape[1])
        terms += t
        if b is not None:
            biases[d_t] = b.clone() if d_t not in biases else biases[d_t] + b
        if wr is not None:
            f_ins.append(wr.shape[1])
            if d_t in roots and roots[d_t].shape != wr.shape:
                raise UnsupportedArch("root weights of one destination type differ in shape")
            roots[d_t] = wr.clone() if d_t not in roots else roots[d_t] + wr
    if not terms:
        raise UnsupportedArch("HeteroConv with no relation present in the graph")
    _check_unmixed(terms)
    # HeteroConv's output dict is keyed in edge_index_dict order (the graph's relation order)
    for et in rel_index:
        if "__".join(et) in conv.convs:
            first_dst = node_type_names.index(et[-1])
            break
    for d_t in sorted(roots):
        terms.append(Term("root", -1, roots[d_t], d_t))
    f_in = max(f_ins)
    for term in terms:
        term.weight = _pad_cols(term.weight, f_in)
        if term.weight_dst is not None:
            term.weight_dst = _pad_cols(term.weight_dst, f_in)
    bias = torch.zeros(nt, f_out)
    for d_t, b in biases.items():
        bias[d_t] = b
    return terms, bias, f_in, f_out, first_dst


def _head_layers(prog, units, i):
    """Append the [Linear act?]* run of `units` starting at i to prog.head; returns the index of
    the first unit past it."""
    while i < len(units) and _is_linear(units[i]):
        lin = units[i]
        act = norm = None
        if i + 1 < len(units) and _is_norm(units[i + 1]):
            norm = units[i + 1]
            i += 1
        if i + 1 < len(units) and _act_name(units[i + 1]) is not None:
            act = _act_name(units[i + 1])
            i += 1
        W = _f32(lin.weight)
        b = _f32(lin.bias) if getattr(lin, "bias", None) is not None else None
        if norm is not None:
            if not _is_bn(norm):
                raise UnsupportedArch("LayerNorm after a head Linear")
            s, t = _bn_affine(norm, W.shape[0])
            W, b = _fold_rows(W, s), _fold_bias(b, s, t, W.shape[0])
        prog.head.append(HeadLayer(W, b, act))
        i += 1
    return i


def _out_norm(prog, units, i):
    """nn.Softmax / nn.LogSoftmax as the LAST unit, after a head Linear (or a headless model's last
    conv) that has no activation of its own: sets prog.out_norm and returns the index past it.  Any
    other place is left to the caller's "unexpected module order"."""
    if i != len(units) - 1 or not _is_out_norm(units[i]):
        return i
    m = units[i]
    if m.dim not in (-1, 1):
        raise UnsupportedArch(f"{type(m).__name__}(dim={m.dim!r}): the class dimension (-1 or 1) only")
    if prog.n_types > 1:
        raise UnsupportedArch(f"{type(m).__name__} on a multi-node-type graph")
    last = prog.head[-1] if prog.head else prog.convs[-1]
    act = last.act if prog.head or last.post is None else last.post.act
    if act is not None:
        raise UnsupportedArch(f"{type(m).__name__} after an activation ({act})")
    prog.out_norm = _OUT_NORMS[type(m).__name__]
    return i + 1


def _check_widths(prog):
    """Width consistency of the conv layers and the head."""
    prev = prog.convs[0].f_in
    for c in prog.convs:
        if c.f_in != prev:
            raise UnsupportedArch("conv widths do not chain")
        prev = c.f_out
    for h in prog.head:
        if h.weight.shape[1] != prev:
            raise UnsupportedArch("head widths do not chain")
        prev = h.weight.shape[0]


POOL_KIND = {"mean": "mean", "add": "sum", "sum": "sum", "max": "max"}


def _compile_pooled(arch, edge_type_names, node_type_names, attention, edge_weight=False,
                    edge_attr=False):
    """nn.PooledModel (matched by class name + `encoder`, `pool`, `fc`): the encoder's conv
    layers, the readout, then the Linear / activation units of `fc` as the head."""
    pool = arch.pool
    if not isinstance(pool, str) or pool not in POOL_KIND:
        raise UnsupportedArch(f"PooledModel(pool={pool!r})")
    if node_type_names is not None and len(node_type_names) >= 2:
        raise UnsupportedArch("PooledModel on a multi-node-type graph")
    prog = compile_arch(arch.encoder, edge_type_names, node_type_names, attention, edge_weight,
                        edge_attr)
    if prog.link_act is not None:
        raise UnsupportedArch("PooledModel over an edge-level (link) encoder")
    if prog.pool is not None:
        raise UnsupportedArch("PooledModel over a pooled encoder")
    if prog.head:
        raise UnsupportedArch("PooledModel encoder with Linear layers after its convs (a head "
                              "belongs after the readout, in fc)")
    if any(t.kind == "rel" for c in prog.convs for t in c.terms):
        raise UnsupportedArch("PooledModel over RGCNConv layers (typed graphs need the "
                              "4-argument call)")
    if prog.n_types > 1:
        raise UnsupportedArch("PooledModel on a multi-node-type program")
    if prog.out_norm is not None:
        raise UnsupportedArch("PooledModel encoder ending in Softmax / LogSoftmax")
    units = list(_leaf_units(arch.fc, attention))
    i = _head_layers(prog, units, 0)
    i = _out_norm(prog, units, i)
    if i != len(units):
        raise UnsupportedArch(f"unexpected module order at {type(units[i]).__name__} in PooledModel.fc")
    _check_widths(prog)
    prog.pool = POOL_KIND[pool]
    return prog


def compile_arch(arch: nn.Module, edge_type_names=None, node_type_names=None,
                 attention=False, edge_weight=False, edge_attr=False) -> ModelProgram:
    """Lower `arch` to a ModelProgram.  `edge_type_names` (list of (src, rel, dst) tuples in
    homogenised edge-type order, data.py:743-822) enables HeteroConv relations;
    `node_type_names` with two or more types selects the multi-node-type lowering.
    `attention=True` (opt-in) also lowers GATConv relations, to "att" terms, and GATv2Conv
    relations, to "att2" terms, and TransformerConv relations, to "qkv" terms; by default an arch
    with any of them raises UnsupportedArch.
    `edge_weight=True`: the arch will be called with an edge_weight.  Only GCNConv and GraphConv take
    one in PyG 2.0.4, so every conv must be one of the two (inside a ConvStack, a BlockStack or a
    PooledModel encoder alike); the program is marked `weighted`.
    `edge_attr=True`: the arch will be called with an edge_attr.  Every conv must be a GINEConv (the
    same three containers); the program is marked `edge_featured` and its "sum" terms carry the
    convs' edge maps.  Without the flag a GINEConv raises UnsupportedArch: it cannot run without
    its attributes."""
    if edge_attr:
        if edge_weight:
            raise UnsupportedArch("edge_attr together with edge_weight")
        if type(arch).__name__ in ("LinkModel", "RelLinkModel"):
            raise UnsupportedArch("edge_attr with an edge-level (link) model")
        if edge_type_names is not None or node_type_names is not None:
            raise UnsupportedArch("edge_attr on a heterogeneous (typed) graph")
    if edge_weight:
        if type(arch).__name__ in ("LinkModel", "RelLinkModel"):
            raise UnsupportedArch("edge_weight with an edge-level (link) model")
        if edge_type_names is not None or node_type_names is not None:
            raise UnsupportedArch("edge_weight on a heterogeneous (typed) graph")
    if type(arch).__name__ == "LinkModel" and hasattr(arch, "encoder"):
        prog = compile_arch(arch.encoder, edge_type_names, node_type_names, attention)
        if prog.pool is not None:
            raise UnsupportedArch("LinkModel over a pooled encoder")
        if prog.out_norm is not None:
            raise UnsupportedArch("LinkModel over an encoder ending in Softmax / LogSoftmax")
        if prog.has_post:
            raise UnsupportedArch("LinkModel over an encoder with post-ops (LayerNorm, residual, "
                                  "BatchNorm after attention)")
        prog.link_act = getattr(arch, "act", "identity") or "identity"
        return prog
    if type(arch).__name__ == "RelLinkModel" and hasattr(arch, "encoder"):
        prog = compile_arch(arch.encoder, edge_type_names, node_type_names, attention)
        if not all(any(t.kind == "rel" for t in c.terms) for c in prog.convs):
            raise UnsupportedArch("RelLinkModel needs an encoder of RGCNConv layers")
        if prog.out_norm is not None:
            raise UnsupportedArch("RelLinkModel over an encoder ending in Softmax / LogSoftmax")
        prog.link_act = getattr(arch, "act", "identity") or "identity"
        emb = getattr(arch, "rel_emb", None)
        if emb is not None:
            width = prog.head[-1].weight.shape[0] if prog.head else prog.convs[-1].f_out
            if emb.dim() != 2 or emb.shape[1] != width:
                raise UnsupportedArch(f"rel_emb of width {tuple(emb.shape)[-1]} on an encoder "
                                      f"output of width {width}")
            prog.link_rel = _f32(emb)
        return prog
    if type(arch).__name__ == "PooledModel" and all(hasattr(arch, a) for a in ("encoder", "pool", "fc")):
        return _compile_pooled(arch, edge_type_names, node_type_names, attention, edge_weight, edge_attr)
    rel_index = None
    if edge_type_names is not None:
        rel_index = {tuple(et): i for i, et in enumerate(edge_type_names)}
    multi = node_type_names is not None and len(node_type_names) >= 2
    if multi and rel_index is None:
        raise UnsupportedArch("multi-node-type graphs need edge types")
    units = list(_leaf_units(arch, attention))
    prog = ModelProgram()
    if multi:
        prog.n_types = len(node_type_names)
    i = 0
    while i < len(units) and _is_conv(units[i], attention):
        if edge_weight and not (type(units[i]).__name__ == "GCNConv" or _is_graphconv(units[i])):
            raise UnsupportedArch(f"{type(units[i]).__name__} takes no edge_weight (GCNConv and "
                                  "GraphConv do)")
        if edge_attr and not _is_gine(units[i]):
            raise UnsupportedArch(f"{type(units[i]).__name__} takes no edge_attr (GINEConv does)")
        if _is_gine(units[i]) and not edge_attr:
            raise UnsupportedArch("GINEConv needs edge_attr")
        if multi:
            terms, bias, f_in, f_out, prog.out_type = _conv_layer_multi(
                units[i], rel_index, list(node_type_names), attention)
            extra = None
        else:
            terms, bias, f_in, f_out, extra = _conv_layer(units[i], rel_index, attention)
        act = norm = None
        if i + 1 < len(units) and _is_norm(units[i + 1]):
            if multi or type(units[i]).__name__ == "HeteroConv":
                raise UnsupportedArch(f"{type(units[i + 1]).__name__} after HeteroConv")
            norm = units[i + 1]
            i += 1
        if i + 1 < len(units) and _act_name(units[i + 1]) is not None:
            act = _act_name(units[i + 1])
            i += 1
        if extra is not None:
            # GINConv over an MLP: the conv layer ends in the MLP's inner activation; its second
            # Linear follows as a ROOT-only layer (each target's own row), whose activation is the
            # MLP's trailing one, else the one after the conv
            lin2, act_in, act_out = extra
            prog.convs.append(ConvLayer(terms, bias, act_in, f_in, f_out))
            W2 = _f32(lin2.weight)
            b2 = _f32(lin2.bias) if getattr(lin2, "bias", None) is not None else torch.zeros(W2.shape[0])
            if act_out is not None and act is not None:
                raise UnsupportedArch("two activations after a GINConv MLP")
            prog.convs.append(ConvLayer([Term("root", -1, W2)], b2, act_out or act, W2.shape[1], W2.shape[0]))
            prog.extra_layers += 1
        else:
            prog.convs.append(ConvLayer(terms, bias, act, f_in, f_out))
        if norm is not None:
            _norm_conv_layer(prog.convs[-1], norm)
        i += 1
    if not prog.convs:
        raise UnsupportedArch("arch has no GCNConv/SAGEConv/HeteroConv layer first")
    typed = [any(t.kind == "rel" for t in c.terms) for c in prog.convs]
    if any(typed) and not all(typed):
        raise UnsupportedArch("a model mixing RGCNConv with another conv kind")
    i = _head_layers(prog, units, i)
    i = _out_norm(prog, units, i)
    if i != len(units):
        raise UnsupportedArch(f"unexpected module order at {type(units[i]).__name__}")
    _check_widths(prog)
    if type(arch).__name__ == "BlockStack" and getattr(arch, "residual", False):
        _add_residuals(prog)
    prog.weighted = bool(edge_weight)
    prog.edge_featured = bool(edge_attr)
    return prog


def _add_residuals(prog):
    """nn.BlockStack(residual=True): block i adds its input row to its output where the two widths
    are equal.  The skip joins the layer's post-op (which takes the activation with it)."""
    if prog.extra_layers:
        raise UnsupportedArch("BlockStack(kind='gin', residual=True): the skip would span two program layers")
    if any(t.kind == "rel" for c in prog.convs for t in c.terms) or prog.n_types > 1:
        raise UnsupportedArch("residual blocks on typed-relation / multi-node-type programs")
    for li, c in enumerate(prog.convs):
        if c.f_in != c.f_out:
            continue
        if li == 0:
            raise UnsupportedArch("a residual on the first block (its input rows are the raw features)")
        if c.post is None:
            c.post, c.act = PostOp(act=c.act), None
        c.post.residual = True


def count_message_passing(arch: nn.Module) -> int:
    """PyG get_num_hops (model.py:52): number of MessagePassing modules."""
    n = 0
    for m in arch.modules():
        if any(c.__name__ == "MessagePassing" for c in type(m).__mro__):
            n += 1
        elif type(m).__name__ in ("GCNConv", "SAGEConv", "GATConv", "GATv2Conv", "TransformerConv", "GINConv", "GINEConv", "GraphConv") + _RGCN_NAMES:
            n += 1
    return n
