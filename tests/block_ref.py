"""fp64 reference of the normalised / residual blocks (nn.BlockStack, and PooledModel over one) for
the block tests, on the B-fold union graph of the reference (features tiled, copy b keeps edge
(u, v) iff mask[b, u] & mask[b, v], oracle.build_edge_mask).  The conv modules themselves run in
double (`.double().eval()`); everything around them is restated here in NumPy and does not go
through BlockStack.forward: BatchNorm1d (eval) and LayerNorm from their state, the ReLU, the skip
rule (equal widths only), the head, the readout.  `post_rows` restates the engine's row op
(xpgnn.h, xpg_post_desc) for the kernel's unit test."""
import copy

import numpy as np
import torch

import gatv2_ref
import oracle
import pool_ref

QUERIES = gatv2_ref.QUERIES


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def randomise_norms(arch, seed):
    """Every BatchNorm1d / LayerNorm of `arch` away from its defaults: gamma in U(0.5, 1.5) with
    every third entry (the first included) negated, beta and the running mean in U(-0.5, 0.5), the
    running variance in U(0.5, 2).  A fresh BatchNorm in eval mode is almost the identity."""
    g = torch.Generator().manual_seed(seed)

    def u(n, lo, hi):
        return torch.rand(n, generator=g) * (hi - lo) + lo
    with torch.no_grad():
        for m in arch.modules():
            name = type(m).__name__
            if name not in ("BatchNorm1d", "LayerNorm"):
                continue
            if getattr(m, "weight", None) is not None:
                w = u(m.weight.numel(), 0.5, 1.5)
                w[::3] *= -1
                m.weight.copy_(w.to(m.weight.dtype))
                m.bias.copy_(u(m.bias.numel(), -0.5, 0.5).to(m.bias.dtype))
            if name == "BatchNorm1d" and m.running_mean is not None:
                m.running_mean.copy_(u(m.running_mean.numel(), -0.5, 0.5).to(m.running_mean.dtype))
                m.running_var.copy_(u(m.running_var.numel(), 0.5, 2.0).to(m.running_var.dtype))
    return arch


def norm_rows(m, z):
    """BatchNorm1d in eval mode / LayerNorm over the last dimension, from the module's state."""
    if type(m).__name__ == "BatchNorm1d":
        z = (z - _np(m.running_mean)) / np.sqrt(_np(m.running_var) + m.eps)
    else:
        mu = z.mean(-1, keepdims=True)
        z = (z - mu) / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + m.eps)
    if getattr(m, "weight", None) is not None:
        z = z * _np(m.weight) + _np(m.bias)
    return z


def _strip_norms(mod):
    """Norm layers inside a conv (the BatchNorm1d of a GIN MLP) replaced by the identity."""
    for name, child in list(mod.named_children()):
        if type(child).__name__ in ("BatchNorm1d", "LayerNorm"):
            setattr(mod, name, torch.nn.Identity())
        else:
            _strip_norms(child)


def encoder_rows(enc, x, ei, masks, drop_norm=False, drop_residual=False):
    """h [B * S, C] fp64 after the blocks of BlockStack `enc`.  drop_norm / drop_residual: the same
    model without its outer norms / its skips (the sensitivity checks)."""
    masks = np.asarray(masks, dtype=bool)
    B = masks.shape[0]
    keep, tiled = oracle.build_edge_mask(masks, np.asarray(ei))
    eit = torch.as_tensor(tiled[:, keep])
    h = np.tile(np.asarray(x, dtype=np.float64), (B, 1))
    mods = list(copy.deepcopy(enc).double().eval().conv)
    if drop_norm:
        for m in mods:
            _strip_norms(m)
    i = 0
    while i < len(mods):
        with torch.no_grad():
            z = mods[i](torch.as_tensor(h), eit).numpy()
        i += 1
        while i < len(mods) and type(mods[i]).__name__ in ("BatchNorm1d", "LayerNorm", "ReLU"):
            if type(mods[i]).__name__ == "ReLU":
                z = np.maximum(z, 0)
            elif not drop_norm:
                z = norm_rows(mods[i], z)
            i += 1
        skip = enc.residual and not drop_residual and z.shape[1] == h.shape[1]
        h = z + h if skip else z
    return h


def union_outputs(arch, x, ei, masks, **drop):
    """fp64 outputs [B, S] (column 0) of a BlockStack on the union graph."""
    masks = np.asarray(masks, dtype=bool)
    return gatv2_ref.head(arch.fc, encoder_rows(arch, x, ei, masks, **drop))[:, 0].reshape(masks.shape)


def pooled_outputs(arch, x, ei, masks, **drop):
    """fp64 outputs [B] (column 0) of nn.PooledModel(BlockStack(...), pool, fc)."""
    masks = np.asarray(masks, dtype=bool)
    h = encoder_rows(arch.encoder, x, ei, masks, **drop)
    return gatv2_ref.head(arch.fc, pool_ref.pool_rows(h, masks.shape[0], arch.pool))[:, 0]


def module_outputs(arch, x, ei, masks, dtype=torch.float64):
    """The module's own forward on the union graph in `dtype`: [B, S] (BlockStack) or [B]
    (PooledModel), column 0, as float64."""
    masks = np.asarray(masks, dtype=bool)
    B, S = masks.shape
    keep, tiled = oracle.build_edge_mask(masks, np.asarray(ei))
    m = copy.deepcopy(arch).to(dtype).eval()
    xt = torch.as_tensor(np.asarray(x)).to(dtype).repeat(B, 1)
    eit = torch.as_tensor(tiled[:, keep])
    with torch.no_grad():
        if hasattr(arch, "pool"):
            return m(xt, eit, torch.arange(B).repeat_interleave(S))[:, 0].double().numpy()
        return m(xt, eit)[:, 0].double().numpy().reshape(B, S)


def post_rows(h, f_out, scale=None, shift=None, norm=None, gamma=None, beta=None, eps=1e-5, act=None,
              hprev=None, tgt_prev=None):
    """The engine's post-op on rows h [M, ld] in fp64: v = h * scale + shift over the f_out real
    columns, LayerNorm (biased variance) with gamma / beta, act, + hprev[r, tgt_prev[t]] for row
    m = r * n_tgt + t, columns f_out.. = 0."""
    h = np.asarray(h, dtype=np.float64)
    M, ld = h.shape
    v = h[:, :f_out].copy()
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float64)
    if shift is not None:
        v = v + np.asarray(shift, dtype=np.float64)
    if norm == "layer":
        mu = v.mean(1, keepdims=True)
        v = (v - mu) / np.sqrt(((v - mu) ** 2).mean(1, keepdims=True) + eps)
        if gamma is not None:
            v = v * np.asarray(gamma, dtype=np.float64)
        if beta is not None:
            v = v + np.asarray(beta, dtype=np.float64)
    v = oracle.apply_act(v, act)
    if hprev is not None:
        hp = np.asarray(hprev, dtype=np.float64)
        tp = np.asarray(tgt_prev)
        v = v + hp[:, tp, :f_out].reshape(M, f_out)
    out = np.zeros((M, ld))
    out[:, :f_out] = v
    return out


# ------------------------------------------------------------------ shared inputs (GPU parity cases)
S = 400
ROWS = 64


def _build(name):
    from bikg_graph_explainability_public_amd.nn import BlockStack, PooledModel
    if name == "sage_ln_res":
        return BlockStack("sage", [16, 8, 8, 8], [8, 1], norm="layer", residual=True)
    if name == "gcn_ln":
        return BlockStack("gcn", [16, 8, 8], [8, 1], norm="layer")
    if name == "sagemax_bn":
        return BlockStack("sage-max", [16, 8, 8], [8, 1], norm="batch")
    if name == "gin_bn":
        return BlockStack("gin", [16, 8, 8], [8, 1], norm="batch")
    if name in ("gat_bn", "gatv2_bn"):
        return BlockStack(name[:-3], [16, 8, 8], [8, 1], heads=[2, 1], norm="batch")
    if name in ("gat_ln_res", "gatv2_ln_res"):
        return BlockStack(name[:-7], [16, 4, 4], [8, 1], heads=[2, 2], norm="layer", residual=True)
    if name == "nohead":  # the last conv layer's post-op ends the model: output = its column 0
        return BlockStack("sage", [16, 8, 8, 8], [8], norm="layer", residual=True)
    if name == "identity":
        return BlockStack("sage", [16, 8, 8, 8], [8, 1], norm="layer", residual=True, final_act="identity")
    if name == "gcn_bn2":
        return BlockStack("gcn", [16, 8, 8], [8, 1], norm="batch")
    if name == "sage_bn2":
        return BlockStack("sage", [16, 8, 8], [8, 1], norm="batch")
    if name == "pooled_gin_bn":
        return PooledModel(BlockStack("gin", [16, 8, 8], [8], norm="batch"), "mean", [8, 1])
    if name == "pooled_sage_ln_res":
        return PooledModel(BlockStack("sage", [16, 8, 8], [8], norm="layer", residual=True), "mean", [8, 1])
    raise KeyError(name)


PLAN_CASES = ["sage_ln_res", "gcn_ln", "sagemax_bn", "gin_bn", "gat_bn", "gatv2_bn", "gat_ln_res",
              "gatv2_ln_res", "nohead", "identity"]
PATH_CASES = ["gcn_bn2", "sage_bn2"]
POOLED_CASES = ["pooled_gin_bn", "pooled_sage_ln_res"]
IDENTITY_OUT = {"nohead", "identity"}  # no sigmoid: the bar is max(1e-5, 4 e32)
_CASES = {}


def case(name):
    """The model of a GPU case (norm state randomised, attention biases given values), the hub
    graph inputs of tests/test_gpu_gatv2.py and the fp64 reference: [64, 3] at the queries, or [64]
    for a pooled model.  Computed once per session."""
    if name in _CASES:
        return _CASES[name]
    seed = sorted(PLAN_CASES + PATH_CASES + POOLED_CASES).index(name)
    torch.manual_seed(40 + seed)
    arch = randomise_norms(_build(name).eval(), 60 + seed)
    g = torch.Generator().manual_seed(80 + seed)
    with torch.no_grad():
        for m in arch.modules():
            if type(m).__name__ in ("GATConv", "GATv2Conv", "GCNConv"):
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    x, ei = gatv2_ref.features(S), gatv2_ref.hub_graph(S)
    masks = gatv2_ref.row_masks(ROWS, S, 3, QUERIES)
    pooled = hasattr(arch, "pool")
    full = (pooled_outputs if pooled else union_outputs)(arch, x.numpy(), ei, masks)
    c = {"name": name, "arch": arch, "x": x, "ei": ei, "masks": masks, "pooled": pooled,
         "full": full, "ref": full if pooled else full[:, QUERIES]}
    _CASES[name] = c
    return c
