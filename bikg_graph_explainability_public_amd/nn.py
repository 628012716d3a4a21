"""PyG-2.0.4-compatible graph layers (GCNConv, SAGEConv, GraphConv, GINConv, GATConv, GATv2Conv,
TransformerConv, RGCNConv, HeteroConv, Linear).

PyTorch Geometric is not available on ROCm boxes here; these modules carry the same
`state_dict` keys as torch_geometric 2.0.4 (`lin.weight` / `bias` for GCNConv, `lin_l.*` /
`lin_r.weight` for SAGEConv, `lin_rel.*` / `lin_root.weight` for GraphConv, `nn.*` / `eps` for
GINConv, `weight` / `comp` / `root` / `bias` for RGCNConv, `convs.<src>__<rel>__<dst>.*` for
HeteroConv, `weight` / `bias` for Linear) so the reference checkpoints (test_data/*.pth.tar, tests/test_utils.py:10-83) load
unchanged.  Their torch `forward` is the semantics the HIP engine compiles (engine.py); the
engine recognises these classes and the real PyG classes by name and attributes.  The model
families built from them (ConvStack, BlockStack with norm layers and skips, RGCNStack, the hetero
stacks, LinkModel / RelLinkModel, PooledModel) follow the registration order the lowering walks.
"""
import math

import torch
from torch import nn
import torch.nn.functional as F

from .program import POOL_KIND as _POOLS  # readout names: "add" is "sum"


class MessagePassing(nn.Module):
    """Marker base class: `Model.get_hops` counts instances (PyG get_num_hops semantics)."""


def _uniform_(t, bound):
    with torch.no_grad():
        t.uniform_(-bound, bound)


class Linear(nn.Module):
    """PyG Linear; in_channels <= 0 is lazy (shape taken from the first input or checkpoint)."""

    def __init__(self, in_channels, out_channels, bias=True, weight_initializer=None,
                 bias_initializer=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight_initializer, self.bias_initializer = weight_initializer, bias_initializer
        if in_channels > 0:
            self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        else:
            self.weight = nn.parameter.UninitializedParameter()
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        if in_channels > 0:
            self.reset_parameters()
        elif self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def reset_parameters(self):
        fan_in = self.weight.shape[1]
        if self.weight_initializer == "glorot":
            _uniform_(self.weight, math.sqrt(6.0 / (fan_in + self.out_channels)))
        else:
            _uniform_(self.weight, 1.0 / math.sqrt(max(fan_in, 1)))
        if self.bias is not None:
            if self.bias_initializer == "zeros":
                with torch.no_grad():
                    self.bias.zero_()
            else:
                _uniform_(self.bias, 1.0 / math.sqrt(max(fan_in, 1)))

    def _materialize(self, in_channels, device, dtype):
        if isinstance(self.weight, nn.parameter.UninitializedParameter):
            self.weight.materialize((self.out_channels, in_channels), device=device, dtype=dtype)
            self.in_channels = in_channels
            self.reset_parameters()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + "weight")
        if w is not None:
            self._materialize(w.shape[1], w.device, w.dtype)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        self._materialize(x.shape[-1], x.device, x.dtype)
        return F.linear(x, self.weight, self.bias)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, bias={self.bias is not None}"


class GCNConv(MessagePassing):
    """GCNConv(normalize=True, add_self_loops=True): D^-1/2 (A + I) D^-1/2 X W^T + b, where
    existing self-loops are replaced by one weight-1 loop per node.  With an `edge_weight` (one
    weight >= 0 per edge) A holds the weights and a node that has self-loops keeps, instead of the
    weight-1 loop, one loop of its LAST self-loop's weight (gcn_norm's add_remaining_self_loops
    with fill_value 1); "last" is taken from the edge position, so the result does not depend on
    how a duplicate-index assignment is ordered on the device."""

    def __init__(self, in_channels, out_channels, bias=True, improved=False, cached=False,
                 add_self_loops=True, normalize=True, **kwargs):
        super().__init__()
        if improved or not add_self_loops or not normalize:
            raise NotImplementedError("only GCNConv(improved=False, add_self_loops=True, "
                                      "normalize=True) is supported")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.add_self_loops, self.normalize = improved, add_self_loops, normalize
        self.lin = Linear(in_channels, out_channels, bias=False, weight_initializer="glorot")
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x, edge_index, edge_weight=None):
        if edge_weight is not None:
            return self._forward_weighted(x, edge_index, edge_weight)
        n = x.size(0)
        ei = edge_index.long()
        keep = ei[0] != ei[1]
        src = torch.cat([ei[0][keep], torch.arange(n, device=x.device)])
        dst = torch.cat([ei[1][keep], torch.arange(n, device=x.device)])
        deg = torch.zeros(n, dtype=x.dtype, device=x.device)
        deg.index_add_(0, dst, torch.ones_like(dst, dtype=x.dtype))
        dis = deg.pow(-0.5)
        dis.masked_fill_(torch.isinf(dis), 0)
        xw = self.lin(x)
        out = torch.zeros_like(xw)
        out.index_add_(0, dst, (dis[src] * dis[dst]).unsqueeze(1) * xw[src])
        if self.bias is not None:
            out = out + self.bias
        return out

    def _forward_weighted(self, x, edge_index, edge_weight):
        n = x.size(0)
        ei = edge_index.long()
        w = edge_weight.reshape(-1).to(x.dtype)
        keep = ei[0] != ei[1]
        # loop weight: the last self-loop of each node by edge position, 1 for a node without one.
        # The loops (ascending positions) are grouped by node with a stable sort; the last entry of
        # each group is written, so no index is assigned twice
        loops = torch.nonzero(~keep).reshape(-1)
        lw = torch.ones(n, dtype=x.dtype, device=x.device)
        if loops.numel():
            order = torch.argsort(ei[0][loops], stable=True)
            ns, pos = ei[0][loops][order], loops[order]
            is_last = torch.ones_like(ns, dtype=torch.bool)
            is_last[:-1] = ns[:-1] != ns[1:]
            lw[ns[is_last]] = w[pos[is_last]]
        ar = torch.arange(n, device=x.device)
        src, dst = torch.cat([ei[0][keep], ar]), torch.cat([ei[1][keep], ar])
        ew = torch.cat([w[keep], lw])
        deg = torch.zeros(n, dtype=x.dtype, device=x.device)
        deg.index_add_(0, dst, ew)
        dis = deg.pow(-0.5)
        dis.masked_fill_(torch.isinf(dis), 0)
        xw = self.lin(x)
        out = torch.zeros_like(xw)
        out.index_add_(0, dst, (dis[src] * ew * dis[dst]).unsqueeze(1) * xw[src])
        if self.bias is not None:
            out = out + self.bias
        return out

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}"


_AGGRS = {"mean": "mean", "add": "sum", "sum": "sum", "max": "max"}


def aggregate(xs, edge_index, n, aggr, edge_weight=None):
    """[n, F]: per target the mean / sum / max of the source rows xs[edge_index[0]] over its
    in-edges (duplicates as separate entries), 0 for a target without edges — the scatter-based
    aggregation of PyG 2.0.4's MessagePassing (torch_scatter fills empty segments with 0, also
    for max, where a non-empty segment of negative rows keeps its negative maximum).
    `edge_weight` [E]: the messages are w_e * x_j (GraphConv's); the mean still divides by the
    COUNT of in-edges."""
    ei = edge_index.long()
    src, dst = ei[0], ei[1]
    kind = _AGGRS[aggr]
    msg = xs[src] if edge_weight is None else edge_weight.reshape(-1, 1).to(xs.dtype) * xs[src]
    if kind == "max":
        idx = dst.unsqueeze(1).expand(-1, xs.size(1))
        return torch.zeros((n, xs.size(1)), dtype=xs.dtype, device=xs.device).scatter_reduce(
            0, idx, msg, reduce="amax", include_self=False)
    s = torch.zeros((n, xs.size(1)), dtype=xs.dtype, device=xs.device)
    s.index_add_(0, dst, msg)
    if kind == "sum":
        return s
    cnt = torch.zeros(n, dtype=xs.dtype, device=xs.device)
    cnt.index_add_(0, dst, torch.ones(ei.size(1), dtype=xs.dtype, device=xs.device))
    return s / cnt.clamp(min=1).unsqueeze(1)


class SAGEConv(MessagePassing):
    """SAGEConv(root_weight=True, normalize=False): lin_l(aggr_j x_j) + lin_r(x) with `aggr` in
    mean / add (= sum) / max."""

    def __init__(self, in_channels, out_channels, bias=True, normalize=False, root_weight=True,
                 aggr="mean", **kwargs):
        super().__init__()
        if normalize or not root_weight or aggr not in _AGGRS:
            raise NotImplementedError("only SAGEConv(aggr in mean / add / sum / max, "
                                      "root_weight=True, normalize=False) is supported")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggr, self.root_weight, self.normalize = aggr, root_weight, normalize
        self.lin_l = Linear(in_channels[0], out_channels, bias=bias)
        self.lin_r = Linear(in_channels[1], out_channels, bias=False)

    def forward(self, x, edge_index):
        xs, xd = (x, x) if isinstance(x, torch.Tensor) else x
        return self.lin_l(aggregate(xs, edge_index, xd.size(0), self.aggr)) + self.lin_r(xd)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}"


class GraphConv(MessagePassing):
    """GraphConv (PyG 2.0.4): lin_rel(aggr_j w_ji x_j) + lin_root(x) with `aggr` in add (= sum) /
    mean / max and w_ji the optional `edge_weight` (1 without one; any finite value, self-loops
    are ordinary edges); lin_rel carries the bias, lin_root has none.  Tuple inputs (x_src, x_dst)
    for bipartite relations."""

    def __init__(self, in_channels, out_channels, aggr="add", bias=True, **kwargs):
        super().__init__()
        if aggr not in _AGGRS:
            raise NotImplementedError("only GraphConv(aggr in add / sum / mean / max) is supported")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.lin_rel = Linear(in_channels[0], out_channels, bias=bias)
        self.lin_root = Linear(in_channels[1], out_channels, bias=False)

    def forward(self, x, edge_index, edge_weight=None):
        xs, xd = (x, x) if isinstance(x, torch.Tensor) else x
        return self.lin_rel(aggregate(xs, edge_index, xd.size(0), self.aggr, edge_weight)) + self.lin_root(xd)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}"


class GINConv(MessagePassing):
    """GINConv (PyG 2.0.4): nn((1 + eps) x + sum_j x_j); `eps` is a buffer, or a parameter with
    train_eps.  Tuple inputs (x_src, x_dst) for bipartite relations."""

    def __init__(self, nn, eps=0.0, train_eps=False, **kwargs):
        super().__init__()
        self.nn = nn
        self.initial_eps, self.aggr = float(eps), "add"
        if train_eps:
            self.eps = torch.nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))

    def forward(self, x, edge_index):
        xs, xd = (x, x) if isinstance(x, torch.Tensor) else x
        return self.nn(aggregate(xs, edge_index, xd.size(0), "add") + (1 + self.eps) * xd)

    def extra_repr(self):
        return f"nn={self.nn}"


class GINEConv(MessagePassing):
    """GINEConv (PyG 2.0.4): nn((1 + eps) x_t + sum over in-edges (j -> t) of relu(x_j + e_jt)),
    e = lin(edge_attr) with lin = Linear(edge_dim, in_channels) when `edge_dim` is given, else
    the attribute rows themselves (their width must be x's).  No self-loops are added: a self-loop
    and a duplicate edge are messages of their own, each with its own attribute row.  `eps` is a
    buffer, or a parameter with train_eps.  The input width is read off the first Linear of `nn`
    (its in_features / in_channels), as PyG does."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None, **kwargs):
        super().__init__()
        self.nn = nn
        self.initial_eps, self.aggr = float(eps), "add"
        if train_eps:
            self.eps = torch.nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))
        self.lin = None
        if edge_dim is not None:
            first = nn[0] if isinstance(nn, torch.nn.Sequential) else nn
            if hasattr(first, "in_features"):
                in_channels = first.in_features
            elif hasattr(first, "in_channels"):
                in_channels = first.in_channels
            else:
                raise ValueError("Could not infer input channels from `nn`.")
            self.lin = Linear(edge_dim, in_channels)

    def forward(self, x, edge_index, edge_attr=None):
        if edge_attr is None:
            raise ValueError("GINEConv needs an edge_attr")
        ea = edge_attr.reshape(-1, 1) if edge_attr.dim() == 1 else edge_attr
        ea = ea.to(x.dtype)
        if self.lin is not None:
            ea = self.lin(ea)
        if ea.size(-1) != x.size(-1):
            raise ValueError("Node and edge feature dimensionalities do not match. Consider setting "
                             "the 'edge_dim' attribute of 'GINEConv'")
        ei = edge_index.long()
        out = torch.zeros_like(x)
        out.index_add_(0, ei[1], torch.relu(x[ei[0]] + ea))
        return self.nn(out + (1 + self.eps) * x)

    def extra_repr(self):
        return f"nn={self.nn}"


class GATConv(MessagePassing):
    """GATConv (PyG 2.0.4): h = x W (W_src / W_dst for bipartite inputs), attention
    softmax over each target's in-edges of leaky_relu(a_src . h_j + a_dst . h_i, 0.2), heads
    concatenated (or averaged), + bias.  The conv of the reference's multi-node-type test arch
    (tests/test_utils.py:86-182: HeteroConv of GATConv((-1, -1), c, add_self_loops=False)).
    By default archs using it run on the generic (batched) torch path; with the opt-in
    (Explainer params["attention_engine"] = True, program.compile_arch(..., attention=True)) the
    engine compiles it to its masked-attention HIP kernels (concat=True, or concat=False with
    one head; no edge_dim)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2,
                 dropout=0.0, add_self_loops=True, bias=True, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops = add_self_loops
        if isinstance(in_channels, int):
            self.lin_src = Linear(in_channels, heads * out_channels, bias=False,
                                  weight_initializer="glorot")
            self.lin_dst = self.lin_src
        else:
            self.lin_src = Linear(in_channels[0], heads * out_channels, bias=False,
                                  weight_initializer="glorot")
            self.lin_dst = Linear(in_channels[1], heads * out_channels, bias=False,
                                  weight_initializer="glorot")
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        _uniform_(self.att_src, math.sqrt(6.0 / (heads + out_channels)))
        _uniform_(self.att_dst, math.sqrt(6.0 / (heads + out_channels)))
        n_bias = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(n_bias)) if bias else None

    def forward(self, x, edge_index):
        H, C = self.heads, self.out_channels
        # gat_conv.py (2.0.4): a Tensor input is transformed by lin_src for BOTH ends, also when a
        # separate lin_dst exists (tuple in_channels: HeteroConv hands same-type relations a
        # Tensor); a tuple input by lin_src / lin_dst
        if isinstance(x, torch.Tensor):
            hs = hd = self.lin_src(x).view(-1, H, C)
        else:
            hs = self.lin_src(x[0]).view(-1, H, C)
            hd = self.lin_dst(x[1]).view(-1, H, C)
        a_s = (hs * self.att_src).sum(-1)
        a_d = (hd * self.att_dst).sum(-1)
        ei = edge_index.long()
        n = hd.size(0)
        if self.add_self_loops:
            loop = torch.arange(min(hs.size(0), n), device=ei.device)
            ei = torch.cat([ei[:, ei[0] != ei[1]], torch.stack([loop, loop])], 1)
        src, dst = ei[0], ei[1]
        alpha = F.leaky_relu(a_s[src] + a_d[dst], self.negative_slope)          # [E, H]
        idx = dst.unsqueeze(1).expand(-1, H)
        amax = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).scatter_reduce(
            0, idx, alpha, reduce="amax", include_self=False)
        ex = (alpha - amax[dst]).exp()
        den = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).index_add_(0, dst, ex)
        alpha = ex / (den[dst] + 1e-16)
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        out = torch.zeros((n, H, C), dtype=hs.dtype, device=hs.device)
        out.index_add_(0, dst, hs[src] * alpha.unsqueeze(-1))
        out = out.reshape(n, H * C) if self.concat else out.mean(dim=1)
        if self.bias is not None:
            out = out + self.bias
        return out

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}"


class GATv2Conv(MessagePassing):
    """GATv2Conv (PyG 2.0.4), "dynamic" attention: x_l = lin_l(x), x_r = lin_r(x) (lin_r is lin_l
    with share_weights), logit of edge (u -> t), head h: att[h] . leaky_relu(x_l[u, h] + x_r[t, h],
    negative_slope), softmax over each target's in-edges, out[t, h] = sum alpha x_l[u, h] (the
    lin_l bias travels inside the messages), heads concatenated (or averaged), + bias.  State-dict
    keys lin_l.weight / lin_l.bias / lin_r.weight / lin_r.bias / att / bias.  Archs using it run on
    the generic torch path unless the attention opt-in is set (Explainer
    params["attention_engine"] = True, program.compile_arch(..., attention=True)): then the engine
    compiles it to its dynamic-attention HIP kernel (concat=True, or concat=False with one head; no
    edge_dim; Tensor input, int in_channels)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2,
                 dropout=0.0, add_self_loops=True, bias=True, share_weights=False, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("GATv2Conv takes an int in_channels (Tensor input)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops, self.share_weights = add_self_loops, share_weights
        self.lin_l = Linear(in_channels, heads * out_channels, bias=bias, weight_initializer="glorot",
                            bias_initializer="zeros")
        self.lin_r = self.lin_l if share_weights else \
            Linear(in_channels, heads * out_channels, bias=bias, weight_initializer="glorot",
                   bias_initializer="zeros")
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        _uniform_(self.att, math.sqrt(6.0 / (heads + out_channels)))
        n_bias = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(n_bias)) if bias else None

    def forward(self, x, edge_index):
        H, C = self.heads, self.out_channels
        xl = self.lin_l(x).view(-1, H, C)
        xr = xl if self.share_weights else self.lin_r(x).view(-1, H, C)
        ei = edge_index.long()
        n = xl.size(0)
        if self.add_self_loops:
            loop = torch.arange(n, device=ei.device)
            ei = torch.cat([ei[:, ei[0] != ei[1]], torch.stack([loop, loop])], 1)
        src, dst = ei[0], ei[1]
        e = F.leaky_relu(xl[src] + xr[dst], self.negative_slope)
        alpha = (e * self.att).sum(-1)                                           # [E, H]
        idx = dst.unsqueeze(1).expand(-1, H)
        amax = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).scatter_reduce(
            0, idx, alpha, reduce="amax", include_self=False)
        ex = (alpha - amax[dst]).exp()
        den = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).index_add_(0, dst, ex)
        alpha = ex / (den[dst] + 1e-16)
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        out = torch.zeros((n, H, C), dtype=xl.dtype, device=xl.device)
        out.index_add_(0, dst, xl[src] * alpha.unsqueeze(-1))
        out = out.reshape(n, H * C) if self.concat else out.mean(dim=1)
        if self.bias is not None:
            out = out + self.bias
        return out

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, heads={self.heads}, "
                f"share_weights={self.share_weights}")


class TransformerConv(MessagePassing):
    """TransformerConv (PyG 2.0.4, the UniMP layer), scaled dot-product attention: Q = lin_query(x),
    K = lin_key(x), V = lin_value(x) viewed as [n, heads, out_channels]; logit of edge (u -> t),
    head h: <Q[t, h], K[u, h]> / sqrt(out_channels); softmax over each target's in-edges (exactly
    the given edges: no self-loops are added or removed; a target without an in-edge gets 0);
    out[t, h] = sum alpha V[u, h]; heads concatenated (or averaged).  With `root_weight`
    x_r = lin_skip(x)[t] is added, or, with `beta`, mixed in through the learned gate
    g = sigmoid(lin_beta([out, x_r, out - x_r])): out = g x_r + (1 - g) out.  There is no separate
    bias parameter; `bias` is lin_skip's.  State-dict keys lin_key.* / lin_query.* / lin_value.* /
    lin_skip.* / lin_beta.weight.  Archs using it run on the generic torch path unless the
    attention opt-in is set (Explainer params["attention_engine"] = True,
    program.compile_arch(..., attention=True)): then the engine compiles it to its dot-product
    attention HIP kernel (concat=True, or concat=False with one head; no edge_dim; Tensor input,
    int in_channels)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0,
                 edge_dim=None, bias=True, root_weight=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("TransformerConv takes an int in_channels (Tensor input)")
        if edge_dim is not None:
            raise NotImplementedError("TransformerConv with edge_dim is not supported")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.dropout, self.edge_dim = concat, dropout, None
        self.root_weight, self.beta = root_weight, bool(beta and root_weight)
        self.lin_key = Linear(in_channels, heads * out_channels)
        self.lin_query = Linear(in_channels, heads * out_channels)
        self.lin_value = Linear(in_channels, heads * out_channels)
        self.lin_edge = None
        skip = heads * out_channels if concat else out_channels
        self.lin_skip = Linear(in_channels, skip, bias=bias)
        self.lin_beta = Linear(3 * skip, 1, bias=False) if self.beta else None

    def forward(self, x, edge_index):
        H, C = self.heads, self.out_channels
        q = self.lin_query(x).view(-1, H, C)
        k = self.lin_key(x).view(-1, H, C)
        v = self.lin_value(x).view(-1, H, C)
        ei = edge_index.long()
        src, dst = ei[0], ei[1]
        n = q.size(0)
        alpha = (q[dst] * k[src]).sum(-1) / math.sqrt(C)                         # [E, H]
        idx = dst.unsqueeze(1).expand(-1, H)
        amax = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).scatter_reduce(
            0, idx, alpha, reduce="amax", include_self=False)
        ex = (alpha - amax[dst]).exp()
        den = torch.zeros((n, H), dtype=alpha.dtype, device=alpha.device).index_add_(0, dst, ex)
        alpha = ex / (den[dst] + 1e-16)
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        out = torch.zeros((n, H, C), dtype=v.dtype, device=v.device)
        out.index_add_(0, dst, v[src] * alpha.unsqueeze(-1))
        out = out.reshape(n, H * C) if self.concat else out.mean(dim=1)
        if self.root_weight:
            x_r = self.lin_skip(x)
            if self.lin_beta is not None:
                g = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
                out = g * x_r + (1 - g) * out
            else:
                out = out + x_r
        return out

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, heads={self.heads}, beta={self.beta}, "
                f"root_weight={self.root_weight}")


class RGCNConv(MessagePassing):
    """RGCNConv (PyG 2.0.4, dense features): out[t] = sum_r AGG_{e = (u -> t), type(e) = r} x_u W_r
    + x_t root + bias, W_r [in, out] (not Linear's [out, in]).  `aggr` = mean (the default; per
    relation over that relation's in-edges of t, a relation without in-edge adds 0) or add / sum.
    Weight forms: plain `weight` [R, in, out]; `num_bases` = B: `weight` [B, in, out] and `comp`
    [R, B], W_r = sum_b comp[r, b] weight[b]; `num_blocks` = nb: `weight` [R, nb, in / nb, out / nb],
    W_r block-diagonal.  No self-loop handling: a (t -> t) edge of type r is an ordinary edge of
    relation r.  FastRGCNConv has the same parameters and the same maths."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, num_blocks=None,
                 aggr="mean", root_weight=True, bias=True, **kwargs):
        super().__init__()
        if aggr not in ("mean", "add", "sum"):
            raise NotImplementedError("only RGCNConv(aggr in mean / add / sum) is supported")
        if num_bases is not None and num_blocks is not None:
            raise ValueError("Can not apply both basis-decomposition and block-diagonal-decomposition "
                             "at the same time.")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.in_channels_l = in_channels[0]
        self.num_relations, self.num_bases, self.num_blocks = num_relations, num_bases, num_blocks
        self.aggr, self.root_weight = aggr, root_weight
        f_in = in_channels[0]
        if num_bases is not None:
            self.weight = nn.Parameter(torch.empty(num_bases, f_in, out_channels))
            self.comp = nn.Parameter(torch.empty(num_relations, num_bases))
        elif num_blocks is not None:
            if f_in % num_blocks or out_channels % num_blocks:
                raise ValueError("Channels must be divisible by num_blocks")
            self.weight = nn.Parameter(torch.empty(num_relations, num_blocks, f_in // num_blocks,
                                                   out_channels // num_blocks))
            self.register_parameter("comp", None)
        else:
            self.weight = nn.Parameter(torch.empty(num_relations, f_in, out_channels))
            self.register_parameter("comp", None)
        if root_weight:
            self.root = nn.Parameter(torch.empty(in_channels[1], out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        for p in (self.weight, self.comp, self.root):  # glorot
            if p is not None:
                _uniform_(p, math.sqrt(6.0 / (p.size(-2) + p.size(-1))))

    def relation_weights(self):
        """The effective dense W_r: [R, in, out]."""
        w = self.weight
        if self.num_bases is not None:
            return (self.comp @ w.reshape(self.num_bases, -1)).reshape(
                self.num_relations, w.size(1), w.size(2))
        if self.num_blocks is not None:
            return torch.stack([torch.block_diag(*w[r]) for r in range(self.num_relations)])
        return w

    def forward(self, x, edge_index, edge_type):
        xs, xd = (x, x) if isinstance(x, torch.Tensor) or x is None else x
        if xs is None or not torch.is_floating_point(xs):
            raise NotImplementedError("featureless RGCNConv (node indices as x) is not supported")
        ei, et = edge_index.long(), edge_type.long()
        n = xd.size(0)
        W = self.relation_weights()
        out = torch.zeros((n, self.out_channels), dtype=xs.dtype, device=xs.device)
        for r in range(self.num_relations):
            sel = et == r
            out = out + aggregate(xs, ei[:, sel], n, self.aggr) @ W[r]
        if self.root is not None:
            out = out + xd @ self.root
        if self.bias is not None:
            out = out + self.bias
        return out

    def extra_repr(self):
        return f"{self.in_channels[0]}, {self.out_channels}, num_relations={self.num_relations}"


class FastRGCNConv(RGCNConv):
    """PyG's FastRGCNConv: RGCNConv's parameters and maths (a different evaluation order there)."""


class HeteroConv(nn.Module):
    """HeteroConv(convs, aggr='sum'): per edge type conv, outputs summed per destination type."""

    def __init__(self, convs, aggr="sum"):
        super().__init__()
        if aggr != "sum":
            raise NotImplementedError("only HeteroConv(aggr='sum') is supported")
        self.convs = nn.ModuleDict({"__".join(k): v for k, v in convs.items()})
        self.aggr = aggr

    def forward(self, x_dict, edge_index_dict):
        out = {}
        for et, ei in edge_index_dict.items():
            key = "__".join(et)
            if key not in self.convs:
                continue
            src, _, dst = et
            conv = self.convs[key]
            o = conv(x_dict[src], ei) if src == dst else conv((x_dict[src], x_dict[dst]), ei)
            out[dst] = o if dst not in out else out[dst] + o
        return out


def _edge_kwargs(edge_weight, edge_attr):
    """The keyword a stack hands to every conv: edge_weight, edge_attr or none (not both)."""
    if edge_weight is not None and edge_attr is not None:
        raise ValueError("edge_attr and edge_weight together are not supported")
    if edge_weight is not None:
        return {"edge_weight": edge_weight}
    return {} if edge_attr is None else {"edge_attr": edge_attr}


def _final_act(final_act):
    """The unit after a stack's last Linear: "sigmoid", a multi-class classifier's "softmax" /
    "log_softmax" over the class (last) dimension, anything else the identity."""
    if final_act == "sigmoid":
        return nn.Sigmoid()
    if final_act == "softmax":
        return nn.Softmax(dim=-1)
    if final_act == "log_softmax":
        return nn.LogSoftmax(dim=-1)
    return nn.Identity()


class ConvStack(nn.Module):
    """Model family of the reference tests/notebooks (tests/test_utils.py:10-83,
    examples/toy_example-caseA.ipynb cell 9): `conv` = ModuleList[Conv, ReLU]*, `fc` =
    ModuleList[Linear, act]* ending in Sigmoid.  `kind` in {"gcn", "sage", "gat"} or one of the
    sum / max families "sage-add", "sage-max", "graphconv" (add), "graphconv-max" and "gin"
    (GINConv over Sequential(Linear, ReLU, Linear)), or "gine" (GINEConv over the same MLP, with
    `edge_dim` handed to it; forward then takes the edge attributes as `edge_attr=`); `hetero_rels`
    wraps each conv in HeteroConv over the given edge types (single node type).  "gat":
    GATConv layers with `heads[i]` concatenated heads of dims[i + 1] channels (default all 1), so
    layer i reads dims[i] * heads[i - 1] columns and the head reads dims[-1] * heads[-1].
    "gatv2": the same with GATv2Conv layers; `share_weights` is handed to them.  "transformer":
    the same widths with TransformerConv layers; `beta` and `root_weight` are handed to them."""

    def __init__(self, kind, dims, fc_dims, hetero_rels=None, final_act="sigmoid", heads=None,
                 add_self_loops=True, share_weights=False, edge_dim=None, beta=False, root_weight=True):
        super().__init__()
        n_conv = len(dims) - 1
        if edge_dim is not None and kind != "gine":
            raise ValueError("edge_dim applies to kind='gine' only")
        if beta and kind != "transformer":
            raise ValueError("beta applies to kind='transformer' only")
        if not root_weight and kind != "transformer":
            raise ValueError("root_weight applies to kind='transformer' only")
        if kind in ("gat", "gatv2", "transformer"):
            heads = [1] * n_conv if heads is None else [int(h) for h in heads]
            if len(heads) != n_conv:
                raise ValueError("heads must give one entry per conv layer")
            if share_weights and kind != "gatv2":
                raise ValueError("share_weights applies to kind='gatv2' only")

            def mk(f_in, f_out, i):
                f_in = f_in * (heads[i - 1] if i else 1)
                if kind == "transformer":
                    return TransformerConv(f_in, f_out, heads=heads[i], beta=beta, root_weight=root_weight)
                if kind == "gatv2":
                    return GATv2Conv(f_in, f_out, heads=heads[i], add_self_loops=add_self_loops,
                                     share_weights=share_weights)
                return GATConv(f_in, f_out, heads=heads[i], add_self_loops=add_self_loops)
        else:
            if heads is not None:
                raise ValueError("heads applies to kind='gat' / 'gatv2' only")
            if share_weights:
                raise ValueError("share_weights applies to kind='gatv2' only")
            makers = {
                "gcn": GCNConv, "sage": SAGEConv,
                "sage-add": lambda i, o: SAGEConv(i, o, aggr="add"),
                "sage-max": lambda i, o: SAGEConv(i, o, aggr="max"),
                "graphconv": GraphConv,
                "graphconv-max": lambda i, o: GraphConv(i, o, aggr="max"),
                "gin": lambda i, o: GINConv(nn.Sequential(Linear(i, o), nn.ReLU(), Linear(o, o))),
                "gine": lambda i, o: GINEConv(nn.Sequential(Linear(i, o), nn.ReLU(), Linear(o, o)),
                                              edge_dim=edge_dim),
            }
            if kind not in makers:
                raise ValueError(f"unknown ConvStack kind {kind!r}")
            cls = makers[kind]

            def mk(f_in, f_out, i):
                return cls(f_in, f_out)
        convs = []
        for i in range(n_conv):
            if hetero_rels is not None:
                convs.append(HeteroConv({tuple(r): mk(dims[i], dims[i + 1], i)
                                         for r in hetero_rels}))
            else:
                convs.append(mk(dims[i], dims[i + 1], i))
            convs.append(nn.ReLU())
        self.conv = nn.ModuleList(convs)
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            last = i == len(fc_dims) - 2
            fcs.append(_final_act(final_act) if last else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index, edge_weight=None, edge_attr=None):
        kw = _edge_kwargs(edge_weight, edge_attr)
        for i, c in enumerate(self.conv):
            if i % 2 == 0:
                x = c(x, edge_index, **kw)
            elif isinstance(x, dict):
                x = {k: c(v) for k, v in x.items()}
            else:
                x = c(x)
        if isinstance(x, dict):
            x = x[list(x.keys())[0]]
        for layer in self.fc:
            x = layer(x)
        return x


class BlockStack(nn.Module):
    """Normalised / residual model family on a homogeneous graph: `conv` = ModuleList[Conv, norm?,
    ReLU]*, `fc` = ModuleList[Linear, act]* as in ConvStack (fc_dims of at most one width: no head,
    e.g. as a PooledModel encoder).  Block i: z = conv_i(h, edge_index); z = norm_i(z); z = relu(z);
    h = z + h with `residual` where z and h have the same width (a block that changes the width,
    normally block 0, takes no skip), else h = z.

    `kind`: every ConvStack kind.  `norm`: None, "batch" (torch.nn.BatchNorm1d(width)) or "layer"
    (torch.nn.LayerNorm(width)); `width` = dims[i + 1] * heads[i] for "gat" / "gatv2" /
    "transformer" (whose `beta` and `root_weight` are handed to TransformerConv).  kind "gin"
    (and "gine", with `edge_dim` and forward's `edge_attr=`) with norm "batch" is the textbook GIN
    block GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear)) with no norm after the conv; with norm "layer" the LayerNorm follows the conv.

    The engine lowers this family by class name plus the `residual` attribute (program.compile_arch):
    BatchNorm in eval mode folds into the weights (a post-op affine after attention layers),
    LayerNorm and the skip are the layer's post-op (k_post in csrc/xpgnn.hip)."""

    def __init__(self, kind, dims, fc_dims, norm=None, residual=False, final_act="sigmoid", heads=None,
                 add_self_loops=True, share_weights=False, edge_dim=None, beta=False, root_weight=True):
        super().__init__()
        if norm not in (None, "batch", "layer"):
            raise ValueError("BlockStack norm must be None, 'batch' or 'layer'")
        if edge_dim is not None and kind != "gine":
            raise ValueError("edge_dim applies to kind='gine' only")
        if beta and kind != "transformer":
            raise ValueError("beta applies to kind='transformer' only")
        if not root_weight and kind != "transformer":
            raise ValueError("root_weight applies to kind='transformer' only")
        n_conv = len(dims) - 1
        attn = kind in ("gat", "gatv2", "transformer")
        if attn:
            heads = [1] * n_conv if heads is None else [int(h) for h in heads]
            if len(heads) != n_conv:
                raise ValueError("heads must give one entry per conv layer")
        elif heads is not None:
            raise ValueError("heads applies to kind='gat' / 'gatv2' only")
        if share_weights and kind != "gatv2":
            raise ValueError("share_weights applies to kind='gatv2' only")
        self.kind, self.norm, self.residual = kind, norm, bool(residual)

        def gin(i, o):
            mlp = [Linear(i, o)] + ([nn.BatchNorm1d(o)] if norm == "batch" else []) + \
                [nn.ReLU(), Linear(o, o)]
            if kind == "gine":
                return GINEConv(nn.Sequential(*mlp), edge_dim=edge_dim)
            return GINConv(nn.Sequential(*mlp))
        makers = {
            "gcn": GCNConv, "sage": SAGEConv,
            "sage-add": lambda i, o: SAGEConv(i, o, aggr="add"),
            "sage-max": lambda i, o: SAGEConv(i, o, aggr="max"),
            "graphconv": GraphConv,
            "graphconv-max": lambda i, o: GraphConv(i, o, aggr="max"),
            "gin": gin, "gine": gin,
        }
        if not attn and kind not in makers:
            raise ValueError(f"unknown BlockStack kind {kind!r}")
        convs = []
        self.block_len = 2 + (norm is not None and not (kind in ("gin", "gine") and norm == "batch"))
        for i in range(n_conv):
            f_in, f_out = dims[i], dims[i + 1]
            if attn:
                f_in, width = f_in * (heads[i - 1] if i else 1), f_out * heads[i]
                if kind == "transformer":
                    convs.append(TransformerConv(f_in, f_out, heads=heads[i], beta=beta,
                                                 root_weight=root_weight))
                elif kind == "gatv2":
                    convs.append(GATv2Conv(f_in, f_out, heads=heads[i], add_self_loops=add_self_loops,
                                           share_weights=share_weights))
                else:
                    convs.append(GATConv(f_in, f_out, heads=heads[i], add_self_loops=add_self_loops))
            else:
                width = f_out
                convs.append(makers[kind](f_in, f_out))
            if self.block_len == 3:
                convs.append(nn.BatchNorm1d(width) if norm == "batch" else nn.LayerNorm(width))
            convs.append(nn.ReLU())
        self.conv = nn.ModuleList(convs)
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            last = i == len(fc_dims) - 2
            fcs.append(_final_act(final_act) if last else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index, edge_weight=None, edge_attr=None):
        n = self.block_len
        kw = _edge_kwargs(edge_weight, edge_attr)
        for i in range(0, len(self.conv), n):
            z = self.conv[i](x, edge_index, **kw)
            for m in self.conv[i + 1:i + n]:
                z = m(z)
            x = z + x if self.residual and z.shape[-1] == x.shape[-1] else z
        for layer in self.fc:
            x = layer(x)
        return x


class RGCNStack(nn.Module):
    """Relational model family on a typed-edge graph, called with the reference's 4-argument
    convention `arch(x, edge_index, node_types, edge_types)` (model.py:102-112): `conv` =
    ModuleList[RGCNConv, ReLU]*, `fc` = ModuleList[Linear, act]* ending in Sigmoid (or Identity) —
    the registration order program.compile_arch walks.  `node_types` is accepted and unused (one
    node type)."""

    def __init__(self, dims, fc_dims, num_relations, num_bases=None, num_blocks=None, aggr="mean",
                 final_act="sigmoid", root_weight=True, bias=True):
        super().__init__()
        convs = []
        for i in range(len(dims) - 1):
            convs.append(RGCNConv(dims[i], dims[i + 1], num_relations, num_bases=num_bases,
                                  num_blocks=num_blocks, aggr=aggr, root_weight=root_weight, bias=bias))
            convs.append(nn.ReLU())
        self.conv = nn.ModuleList(convs)
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            last = i == len(fc_dims) - 2
            fcs.append(_final_act(final_act) if last else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index, node_types, edge_types):
        for i, c in enumerate(self.conv):
            x = c(x, edge_index, edge_types) if i % 2 == 0 else c(x)
        for layer in self.fc:
            x = layer(x)
        return x


class HeteroSageStack(nn.Module):
    """Multi-node-type model family: [HeteroConv({(src, rel, dst): SAGEConv}) -> ReLU]* then
    Linear layers on the first output node type — the layout of the reference's multi-type
    test arch (tests/test_utils.py:86-182) with SAGEConv relations (bipartite layer-1 inputs
    (F_src, F_dst)).  state_dict keys: conv.<2l>.convs.<src>__<rel>__<dst>.lin_l/lin_r.*,
    fc.<2i>.weight/bias."""

    def __init__(self, rels, in_dims, hidden, n_layers, fc_dims):
        super().__init__()
        convs = []
        for li in range(n_layers):
            convs.append(HeteroConv({tuple(r): SAGEConv((in_dims[r[0]], in_dims[r[-1]])
                                                        if li == 0 else (hidden, hidden), hidden)
                                     for r in rels}))
            convs.append(nn.ReLU())
        self.conv = nn.ModuleList(convs)
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            fcs.append(nn.Sigmoid() if i == len(fc_dims) - 2 else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index):
        for i, c in enumerate(self.conv):
            x = c(x, edge_index) if i % 2 == 0 else {k: c(v) for k, v in x.items()}
        x = x[list(x.keys())[0]]
        for layer in self.fc:
            x = layer(x)
        return x


class HeteroGATStack(nn.Module):
    """Multi-node-type model family of the reference's own multi-type test arch
    (tests/test_utils.py:86-182: HeteroConv({(src, rel, dst): GATConv((-1, -1), c,
    add_self_loops=False)}, aggr="sum") -> ReLU, then Linear layers on the first output node
    type), with explicit input widths per layer and `heads` per layer (concatenated).  It runs
    on the generic (batched) torch path unless the attention engine is opted into
    (params["attention_engine"] = True; add_self_loops=False only on multi-type graphs).
    state_dict keys:
    conv.<2l>.convs.<src>__<rel>__<dst>.{lin_src,lin_dst}.weight / att_src / att_dst / bias."""

    def __init__(self, rels, in_dims, hidden, heads, fc_dims, add_self_loops=False):
        super().__init__()
        convs, width = [], None
        for li, h in enumerate(heads):
            convs.append(HeteroConv({tuple(r): GATConv((in_dims[r[0]], in_dims[r[-1]]) if li == 0
                                                       else (width, width), hidden, heads=h,
                                                       add_self_loops=add_self_loops)
                                     for r in rels}))
            convs.append(nn.ReLU())
            width = hidden * h
        self.conv = nn.ModuleList(convs)
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            fcs.append(nn.Sigmoid() if i == len(fc_dims) - 2 else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index):
        for i, c in enumerate(self.conv):
            x = c(x, edge_index) if i % 2 == 0 else {k: c(v) for k, v in x.items()}
        x = x[list(x.keys())[0]]
        for layer in self.fc:
            x = layer(x)
        return x


class LinkModel(nn.Module):
    """Edge-level model for edge problems: a node encoder (e.g. ConvStack with
    final_act="identity") and a dot-product link decoder, score(u, v) = act(<z_u, z_v>).

    forward(x, edge_index, edge_label_index=None) runs the encoder's message passing over
    `edge_index` and scores the edges of `edge_label_index` (default: every edge of
    `edge_index`) — the per-edge output the reference's edge problem extracts
    (model.py:295-328).  Scoring a separate label index keeps the query edge's output defined
    when Data.perturb_edge (data.py:500-554) removes that edge from the message passing."""

    def __init__(self, encoder, act="sigmoid"):
        super().__init__()
        if act not in ("sigmoid", "identity", None):
            raise ValueError("LinkModel act must be 'sigmoid' or 'identity'")
        self.encoder = encoder
        self.act = act or "identity"

    def forward(self, x, edge_index, edge_label_index=None):
        z = self.encoder(x, edge_index)
        eli = edge_index if edge_label_index is None else edge_label_index
        s = (z[eli[0]] * z[eli[1]]).sum(-1, keepdim=True)
        return torch.sigmoid(s) if self.act == "sigmoid" else s


class RelLinkModel(nn.Module):
    """Edge-level model of a typed-edge graph (the knowledge-graph link predictor): a relational
    encoder called `encoder(x, edge_index, node_types, edge_types)` (e.g. RGCNStack with
    final_act="identity"; fc_dims of one width = no head) and a DistMult decoder,
    score(u, r, v) = act(sum_f z_u[f] rel_emb[r][f] z_v[f]), or decoder="dot" (no `rel_emb`, the
    factor is 1).

    forward(x, edge_index, node_types, edge_types, edge_label_index=None, edge_label_type=None)
    scores the edges of `edge_label_index` with types `edge_label_type` (defaults: every edge of
    `edge_index` with its own type) -> [n_label, 1].  As with LinkModel, a separate label index
    keeps the query edge's score defined when its own column is masked out."""

    def __init__(self, encoder, num_relations, decoder="distmult", act="sigmoid"):
        super().__init__()
        if act not in ("sigmoid", "identity", None):
            raise ValueError("RelLinkModel act must be 'sigmoid' or 'identity'")
        if decoder not in ("distmult", "dot"):
            raise ValueError("RelLinkModel decoder must be 'distmult' or 'dot'")
        self.encoder = encoder
        self.num_relations = int(num_relations)
        self.decoder = decoder
        self.act = act or "identity"
        if decoder == "distmult":
            width = None
            for m in encoder.modules():  # the encoder's output width: its last Linear / RGCNConv
                if hasattr(m, "out_channels"):
                    width = int(m.out_channels)
            if width is None:
                raise ValueError("RelLinkModel cannot tell the encoder's output width")
            self.rel_emb = nn.Parameter(torch.empty(self.num_relations, width))
            _uniform_(self.rel_emb, math.sqrt(6.0 / (self.num_relations + width)))  # glorot
        else:
            self.register_parameter("rel_emb", None)

    def forward(self, x, edge_index, node_types, edge_types, edge_label_index=None,
                edge_label_type=None):
        z = self.encoder(x, edge_index, node_types, edge_types)
        eli = edge_index if edge_label_index is None else edge_label_index
        s = z[eli[0].long()]
        if self.rel_emb is not None:
            elt = edge_types if edge_label_type is None else edge_label_type
            s = s * self.rel_emb[elt.reshape(-1).long()]
        s = (s * z[eli[1].long()]).sum(-1, keepdim=True)
        return torch.sigmoid(s) if self.act == "sigmoid" else s


def global_pool(h, batch, kind, size=None):
    """Graph-level readout (PyG global_mean_pool / global_add_pool / global_max_pool): the rows of
    `h` [n, C] reduced per graph, `batch` [n] giving each row's graph (None: one graph), to
    [size, C] (`size` default: batch.max() + 1).  Plain torch: index_add_ for the sums (mean = sum /
    count) and scatter_reduce(..., "amax", include_self=False) for max; a graph without a node
    gives 0."""
    if kind not in _POOLS:
        raise ValueError(f"unknown pool {kind!r}: one of {sorted(_POOLS)}")
    kind = _POOLS[kind]
    if batch is None:
        batch = torch.zeros(h.shape[0], dtype=torch.long, device=h.device)
    batch = batch.reshape(-1).long()
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() else 1
    if kind == "max":
        out = torch.zeros((size, h.shape[1]), dtype=h.dtype, device=h.device)
        return out.scatter_reduce(0, batch[:, None].expand(-1, h.shape[1]), h, "amax",
                                  include_self=False)
    out = torch.zeros((size, h.shape[1]), dtype=h.dtype, device=h.device).index_add_(0, batch, h)
    if kind == "mean":
        cnt = torch.zeros(size, dtype=h.dtype, device=h.device).index_add_(
            0, batch, torch.ones(batch.numel(), dtype=h.dtype, device=h.device))
        out = out / cnt.clamp(min=1)[:, None]
    return out


class PooledModel(nn.Module):
    """Graph-level model (graph classifier / regressor): a node encoder, a global readout and an
    MLP head, out = fc(pool(encoder(x, edge_index), batch)) -> [n_graphs, fc_dims[-1]].

    `encoder`: a module whose leaf units follow the `[conv act?]+` rule with no Linear after them,
    e.g. ConvStack(kind, dims, [dims[-1]]) (an empty `fc`).  `pool` in {"mean", "add", "sum",
    "max"}; `fc` = ModuleList[Linear, act]* as in ConvStack.  forward(x, edge_index, batch=None):
    `batch` [n] is each node's graph (None: one graph); the explainer passes it to keep the B
    perturbed copies of the union graph apart.

    The engine lowers this family by class name plus the attributes `encoder`, `pool` and `fc`
    (program.compile_arch, as LinkModel is matched): a model that calls PyG's functional
    global_mean_pool / global_add_pool / global_max_pool in its own forward is explained on the
    engine by wrapping its encoder and head in this class."""

    def __init__(self, encoder, pool, fc_dims, final_act="sigmoid"):
        super().__init__()
        if pool not in _POOLS:
            raise ValueError(f"PooledModel pool must be one of {sorted(_POOLS)}")
        self.encoder = encoder
        self.pool = pool
        fcs = []
        for i in range(len(fc_dims) - 1):
            fcs.append(Linear(fc_dims[i], fc_dims[i + 1]))
            last = i == len(fc_dims) - 2
            fcs.append(_final_act(final_act) if last else nn.ReLU())
        self.fc = nn.ModuleList(fcs)

    def forward(self, x, edge_index, batch=None, edge_weight=None, edge_attr=None):
        h = self.encoder(x, edge_index, **_edge_kwargs(edge_weight, edge_attr))
        h = global_pool(h, batch, self.pool)
        for layer in self.fc:
            h = layer(h)
        return h
