"""Normalised / residual blocks without a GPU: nn.BlockStack against the fp64 restatement of
tests/block_ref.py, the lowering of BatchNorm1d / LayerNorm / skips (program.compile_arch), every
refusal, the additive C-ABI (`_post` symbols, host checks and describe texts on synthetic
descriptors) and, on the reference alone, that the GPU cases of tests/test_gpu_blocks.py move with
the masks, with their norms and with their skips."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import block_ref
import gatv2_ref
from test_dispatch_cpu import ENV, GCN, PTR, SAGE, describe, make_plan

from bikg_graph_explainability_public_amd import _lib
from bikg_graph_explainability_public_amd import nn as xnn
from bikg_graph_explainability_public_amd.nn import BlockStack, ConvStack, LinkModel, PooledModel
from bikg_graph_explainability_public_amd.program import (UnsupportedArch, compile_arch,
                                                          count_message_passing)

KINDS = ["gcn", "sage", "sage-add", "sage-max", "graphconv", "graphconv-max", "gin", "gat", "gatv2"]
NORMS = [None, "batch", "layer"]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _small_graph(n=30, e=120, f=6, seed=0):
    g = np.random.default_rng(seed)
    ei = g.integers(0, n, (2, e))
    x = torch.randn((n, f), generator=torch.Generator().manual_seed(seed + 1))
    m = g.random((5, n)) < 0.7
    m[0], m[1] = False, True
    return x, ei, m


def _stack(kind, norm, residual, dims=(6, 8, 8, 8), seed=0, **kw):
    torch.manual_seed(seed)
    attn = kind in ("gat", "gatv2")
    heads = [2] * (len(dims) - 1) if attn else None
    fc_in = dims[-1] * (2 if attn else 1)
    a = BlockStack(kind, list(dims), [fc_in, 1], norm=norm, residual=residual, heads=heads, **kw).eval()
    return block_ref.randomise_norms(a, seed + 5)


# ------------------------------------------------------------------ the module
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_blockstack_forward_matches_the_restatement(kind, norm, residual):
    """dims [6, 8, 8, 8] (attention: 2 heads, so 6 -> 16 -> 16 -> 16): block 0 changes the width
    and takes no skip, blocks 1 and 2 do with `residual`."""
    a = _stack(kind, norm, residual)
    x, ei, m = _small_graph()
    ref = block_ref.union_outputs(a, x.numpy(), ei, m)
    got = block_ref.module_outputs(a, x.numpy(), ei, m)
    assert np.abs(got - ref).max() < 1e-12
    if residual:
        assert np.abs(ref - block_ref.union_outputs(a, x.numpy(), ei, m, drop_residual=True)).max() > 1e-3
    if norm:
        assert np.abs(ref - block_ref.union_outputs(a, x.numpy(), ei, m, drop_norm=True)).max() > 1e-3


def test_state_dict_keys_and_hops():
    a = BlockStack("sage", [6, 8, 8], [8, 4, 1], norm="batch")
    keys = set(a.state_dict())
    assert {"conv.0.lin_l.weight", "conv.0.lin_l.bias", "conv.0.lin_r.weight", "conv.1.weight",
            "conv.1.bias", "conv.1.running_mean", "conv.1.running_var", "conv.3.lin_l.weight",
            "conv.4.running_var", "fc.0.weight", "fc.2.bias"} <= keys
    assert [type(m).__name__ for m in a.conv] == ["SAGEConv", "BatchNorm1d", "ReLU"] * 2
    assert [type(m).__name__ for m in a.fc] == ["Linear", "ReLU", "Linear", "Sigmoid"]
    assert isinstance(a.conv[1], torch.nn.BatchNorm1d) and a.conv[1].num_features == 8
    ln = BlockStack("gat", [6, 4, 4], [8, 1], norm="layer", heads=[3, 2])
    assert isinstance(ln.conv[1], torch.nn.LayerNorm) and ln.conv[1].normalized_shape == (12,)
    assert ln.conv[4].normalized_shape == (8,) and ln.conv[3].lin_src.weight.shape == (8, 12)
    g = BlockStack("gin", [6, 8, 8], [8], norm="batch")
    assert [type(m).__name__ for m in g.conv] == ["GINConv", "ReLU"] * 2 and len(g.fc) == 0
    assert [type(m).__name__ for m in g.conv[0].nn] == ["Linear", "BatchNorm1d", "ReLU", "Linear"]
    assert "conv.0.nn.1.running_mean" in g.state_dict()
    gl = BlockStack("gin", [6, 8, 8], [8, 1], norm="layer")
    assert [type(m).__name__ for m in gl.conv] == ["GINConv", "LayerNorm", "ReLU"] * 2
    assert [type(m).__name__ for m in gl.conv[0].nn] == ["Linear", "ReLU", "Linear"]
    for m, hops in ((a, 2), (ln, 2), (g, 2), (gl, 2), (_stack("sage", "layer", True), 3)):
        assert count_message_passing(m) == hops
        assert compile_arch(m.eval(), attention=True).hops == hops
    with pytest.raises(ValueError):
        BlockStack("sage", [6, 8], [8, 1], norm="group")
    with pytest.raises(ValueError):
        BlockStack("sage", [6, 8], [8, 1], heads=[2])


# ------------------------------------------------------------------ lowering
def _program_forward(prog, x, ei):
    """The program's layers in fp64 on one graph (no masks): terms as the conv families define them
    (tests of the fold: gcn / mean / sum / max / root terms only), post-ops by block_ref.post_rows."""
    from bikg_graph_explainability_public_amd.nn import aggregate
    import oracle
    h = x.double()
    eit = torch.as_tensor(ei)
    n = h.shape[0]
    for c in prog.convs:
        z = c.bias.double().expand(n, -1).clone()
        for t in c.terms:
            W = t.weight.double()
            if t.kind == "root":
                z = z + h @ W.T
            elif t.kind == "gcn":
                z = z + torch.as_tensor(oracle.gcn_conv(h.numpy(), ei[0], ei[1], n, W.numpy(), None))
            else:
                z = z + aggregate(h, eit, n, {"mean": "mean", "sum": "add", "max": "max"}[t.kind]) @ W.T
        z = z.numpy()
        if c.post is not None:
            q = c.post
            z = block_ref.post_rows(z, c.f_out, q.scale, q.shift, q.norm, q.gamma, q.beta, q.eps, q.act,
                                    h.numpy()[None] if q.residual else None,
                                    np.arange(n) if q.residual else None)
        else:
            z = oracle.apply_act(z, c.act)
        h = torch.as_tensor(z)
    h = h.numpy()
    for hl in prog.head:
        h = oracle.apply_act(h @ hl.weight.double().numpy().T + (0 if hl.bias is None else hl.bias.double().numpy()),
                             hl.act)
    return h


@pytest.mark.parametrize("kind", ["gcn", "sage", "sage-add", "sage-max", "graphconv", "graphconv-max", "gin"])
def test_batchnorm_folds_reproduce_the_module(kind):
    """The fold is exact algebra: compiled without the program's float32 rounding (_compile_fp64)
    and evaluated in fp64, the folded program reproduces the double module to 1e-12; the float32
    program (weights rounded once after an fp64 fold) to 1e-5.  The folded program has the term
    kinds and shapes of the same model without norms."""
    a = _stack(kind, "batch", False).double()
    prog = compile_arch(a)
    assert not prog.has_post and all(c.act == "relu" for c in prog.convs)
    plain = compile_arch(_stack(kind, None, False))
    assert [[(t.kind, tuple(t.weight.shape)) for t in c.terms] for c in prog.convs] == \
        [[(t.kind, tuple(t.weight.shape)) for t in c.terms] for c in plain.convs]
    assert [tuple(c.bias.shape) for c in prog.convs] == [tuple(c.bias.shape) for c in plain.convs]
    x, ei, _ = _small_graph()
    with torch.no_grad():
        want = a(x.double(), torch.as_tensor(ei)).numpy()
    got32 = _program_forward(prog, x, ei)
    assert np.abs(got32 - want).max() < 1e-5
    prog64 = _compile_fp64(a)
    got = _program_forward(prog64, x, ei)
    print("fold error fp64:", np.abs(got - want).max())
    assert np.abs(got - want).max() < 1e-12
    if kind == "sage-max":
        bn = a.conv[1]
        assert (bn.weight < 0).any()  # a negative gamma after a max aggregation


def _compile_fp64(arch):
    """compile_arch with the float32 rounding of the program's tensors switched off."""
    from bikg_graph_explainability_public_amd import program
    saved = (program._f32, program._fold_rows, program._fold_bias)
    program._f32 = lambda t: t.detach().double()
    program._fold_rows = lambda w, s: s.reshape(-1, 1) * w.detach().double()
    program._fold_bias = lambda b, s, t, width: s * (torch.zeros(width, dtype=torch.float64) if b is None
                                                   else b.detach().double()) + t
    try:
        return compile_arch(arch, attention=True)
    finally:
        program._f32, program._fold_rows, program._fold_bias = saved


@torch.no_grad()
def test_gin_mlp_with_batchnorm_lowers():
    a = _stack("gin", "batch", False)
    prog = compile_arch(a)
    assert [[t.kind for t in c.terms] for c in prog.convs] == [["sum", "root"], ["root"]] * 3
    assert prog.extra_layers == 3 and prog.hops == 3 and not prog.has_post
    lin, bn = a.conv[0].nn[0], a.conv[0].nn[1]
    s = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).double()
    np.testing.assert_allclose(prog.convs[0].terms[0].weight.double(), s[:, None] * lin.weight.double(),
                               rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(prog.convs[0].bias.double(),
                               s * (lin.bias.double() - bn.running_mean.double()) + bn.bias.double(),
                               rtol=1e-6, atol=1e-7)
    # plain user module, the textbook block, BN also after the head Linear
    class Gin(torch.nn.Module):
        def __init__(self):
            super().__init__()
            seq = torch.nn.Sequential
            self.c1 = xnn.GINConv(seq(xnn.Linear(6, 8), torch.nn.BatchNorm1d(8), torch.nn.ReLU(), xnn.Linear(8, 8)))
            self.a1 = torch.nn.ReLU()
            self.l = xnn.Linear(8, 4)
            self.bn = torch.nn.BatchNorm1d(4, affine=False)
            self.a2 = torch.nn.ReLU()
            self.o = xnn.Linear(4, 1)

        def forward(self, x, ei):
            return self.o(self.a2(self.bn(self.l(self.a1(self.c1(x, ei))))))
    torch.manual_seed(1)
    m = block_ref.randomise_norms(Gin().eval(), 2).double()
    x, ei, _ = _small_graph()
    with torch.no_grad():
        want = m(x.double(), torch.as_tensor(ei)).numpy()
    assert np.abs(_program_forward(_compile_fp64(m), x, ei) - want).max() < 1e-12
    p = compile_arch(m)
    assert len(p.head) == 2 and p.head[0].act == "relu" and not p.has_post


@pytest.mark.parametrize("kind,term", [("gat", "att"), ("gatv2", "att2")])
@torch.no_grad()
def test_attention_norms_become_post_ops(kind, term):
    bn = compile_arch(_stack(kind, "batch", True), attention=True)
    for li, c in enumerate(bn.convs):
        assert [t.kind for t in c.terms] == [term] and c.act is None
        q = c.post
        assert q.norm is None and q.scale.shape == (16,) and q.shift.shape == (16,) and q.act == "relu"
        assert q.gamma is None and q.beta is None and q.residual == (li > 0)
    a = _stack(kind, "batch", False)
    m = a.conv[1]
    q = compile_arch(a, attention=True).convs[0].post
    s = m.weight.double() / torch.sqrt(m.running_var.double() + m.eps)
    np.testing.assert_allclose(q.scale.double(), s, rtol=1e-6)
    np.testing.assert_allclose(q.shift.double(), m.bias.double() - m.running_mean.double() * s, rtol=1e-6, atol=1e-7)
    assert (q.scale < 0).any()
    plain = compile_arch(_stack(kind, None, False), attention=True)
    for c, d in zip(bn.convs, plain.convs):  # the terms are untouched
        assert all(torch.equal(getattr(c.terms[0], f), getattr(d.terms[0], f)) for f in ("weight",))
    ln = compile_arch(_stack(kind, "layer", False), attention=True)
    for c in ln.convs:
        q = c.post
        assert c.act is None and q.norm == "layer" and q.eps == 1e-5 and q.scale is None and q.shift is None
        assert q.gamma.shape == (16,) and q.beta.shape == (16,) and q.act == "relu" and not q.residual


@torch.no_grad()
def test_layernorm_and_residual_records():
    a = _stack("sage", "layer", True)
    prog = compile_arch(a)
    assert [c.post.residual for c in prog.convs] == [False, True, True]
    assert all(c.act is None and c.post.act == "relu" and c.post.norm == "layer" for c in prog.convs)
    assert torch.equal(prog.convs[1].post.gamma, a.conv[4].weight.detach())
    a.conv[1] = torch.nn.LayerNorm(8, elementwise_affine=False)
    q = compile_arch(a).convs[0].post
    assert q.gamma is None and q.beta is None and q.norm == "layer"
    # BN folded + skip: the record holds the activation and the skip only
    p = compile_arch(_stack("gcn", "batch", True))
    assert p.convs[0].post is None and p.convs[0].act == "relu"
    q = p.convs[1].post
    assert (q.norm, q.scale, q.shift, q.act, q.residual) == (None, None, None, "relu", True)
    # fp64 program against the module, LN + skip, on one graph
    x, ei, _ = _small_graph()
    m = _stack("sage-max", "layer", True).double()
    with torch.no_grad():
        want = m(x.double(), torch.as_tensor(ei)).numpy()
    assert np.abs(_program_forward(_compile_fp64(m), x, ei) - want).max() < 1e-12
    # a plain user module in registration order, no skip
    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.n1, self.a1 = xnn.SAGEConv(6, 8), torch.nn.LayerNorm(8), torch.nn.ReLU()
            self.c2, self.n2, self.a2 = xnn.GCNConv(8, 8), torch.nn.BatchNorm1d(8), torch.nn.ReLU()
            self.o = xnn.Linear(8, 1)

        def forward(self, x, ei):
            x = self.a1(self.n1(self.c1(x, ei)))
            return self.o(self.a2(self.n2(self.c2(x, ei))))
    torch.manual_seed(3)
    m = block_ref.randomise_norms(Plain().eval(), 4).double()
    pp = compile_arch(m)
    assert pp.convs[0].post.norm == "layer" and pp.convs[1].post is None and pp.convs[1].act == "relu"
    with torch.no_grad():
        want = m(x.double(), torch.as_tensor(ei)).numpy()
    assert np.abs(_program_forward(_compile_fp64(m), x, ei) - want).max() < 1e-12


def test_convstack_compiles_to_an_unchanged_program():
    for kind in ("gcn", "sage", "sage-max", "gin", "gat"):
        torch.manual_seed(0)
        a = ConvStack(kind, [6, 8, 8], [8, 1]).eval()
        p = compile_arch(a, attention=True)
        assert not p.has_post and all(c.post is None and c.act == "relu" for c in p.convs)
        torch.manual_seed(0)
        b = BlockStack(kind, [6, 8, 8], [8, 1]).eval()  # no norm, no skip: the same model
        q = compile_arch(b, attention=True)
        assert not q.has_post
        for c, d in zip(p.convs, q.convs):
            assert [t.kind for t in c.terms] == [t.kind for t in d.terms]
            assert all(torch.equal(s.weight, t.weight) for s, t in zip(c.terms, d.terms))
            assert torch.equal(c.bias, d.bias) and c.act == d.act


# ------------------------------------------------------------------ refusals
class Odd(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bn = torch.nn.BatchNorm1d(4)

    def forward(self, x, ei):
        return self.bn(x)


class LayerNorm(torch.nn.Module):
    """A graph-mode norm that shares torch's class name (as PyG's does)."""

    def __init__(self, n):
        super().__init__()
        self.weight, self.bias = torch.nn.Parameter(torch.ones(n)), torch.nn.Parameter(torch.zeros(n))
        self.normalized_shape, self.eps = (n,), 1e-5

    def forward(self, x):
        return x


def _refuse(arch, match, **kw):
    with pytest.raises(UnsupportedArch, match=match):
        compile_arch(arch, **kw)


def test_refusals():
    with pytest.raises(UnsupportedArch):
        compile_arch(Odd())
    for norm in NORMS:
        _refuse(_stack("gin", norm, True), "span two program layers")
    a = _stack("sage", "batch", False)
    a.conv[1].train()
    _refuse(a, "training mode")
    a = _stack("sage", "batch", False)
    a.conv[1] = torch.nn.BatchNorm1d(8, track_running_stats=False).eval()
    _refuse(a, "running statistics")
    a = _stack("gin", "batch", False)
    a.conv[0].nn[1].train()
    _refuse(a, "training mode")
    a = _stack("sage", "layer", False)
    a.conv[1] = LayerNorm(8)
    _refuse(a, "not torch.nn.LayerNorm")
    a = _stack("sage", "layer", False)
    a.conv[1] = torch.nn.LayerNorm([1, 8])
    _refuse(a, "last dimension only")
    a = _stack("sage", "layer", False)
    a.conv[1] = torch.nn.LayerNorm(4)
    _refuse(a, "width 8")
    a = _stack("sage", None, False)
    a.fc = torch.nn.ModuleList([xnn.Linear(8, 4), torch.nn.LayerNorm(4), torch.nn.ReLU(), xnn.Linear(4, 1)])
    _refuse(a, "LayerNorm after a head Linear")
    # residual on the first block (equal widths from the start)
    _refuse(_stack("sage", None, True, dims=(8, 8, 8)), "first block")
    # typed relations, HeteroConv, multi-node-type graphs
    r = xnn.RGCNStack([6, 8, 8], [8, 1], 3)
    for norm, what in ((torch.nn.LayerNorm(8), "LayerNorm after RGCNConv"),
                       (torch.nn.BatchNorm1d(8).eval(), "BatchNorm1d after RGCNConv")):
        rr = copy.deepcopy(r)
        rr.conv = torch.nn.ModuleList([rr.conv[0], norm, rr.conv[1], rr.conv[2], rr.conv[3]])
        _refuse(rr.eval(), what)
    rels = [("n", "a", "n"), ("n", "b", "n")]
    h = ConvStack("sage", [6, 8, 8], [8, 1], hetero_rels=rels)
    h.conv = torch.nn.ModuleList([h.conv[0], torch.nn.LayerNorm(8)] + list(h.conv[1:]))
    _refuse(h.eval(), "after HeteroConv", edge_type_names=rels)
    mt = xnn.HeteroSageStack([("a", "r", "b"), ("b", "s", "a")], {"a": 4, "b": 5}, 8, 2, [8, 1])
    mt.conv = torch.nn.ModuleList([mt.conv[0], torch.nn.BatchNorm1d(8)] + list(mt.conv[1:]))
    _refuse(mt.eval(), "after HeteroConv", edge_type_names=[("a", "r", "b"), ("b", "s", "a")],
            node_type_names=["a", "b"])
    # link models over an encoder with post-ops
    enc = BlockStack("sage", [6, 8, 8], [8], norm="layer", final_act="identity").eval()
    _refuse(LinkModel(enc), "LinkModel over an encoder with post-ops")
    # a PooledModel encoder with post-ops compiles; its head takes BN, not LN
    pm = PooledModel(BlockStack("sage", [6, 8, 8], [8], norm="layer", residual=True), "mean", [8, 1]).eval()
    p = compile_arch(pm)
    assert p.pool == "mean" and p.has_post and p.convs[1].post.residual
    pm.fc = torch.nn.ModuleList([xnn.Linear(8, 4), torch.nn.LayerNorm(4), xnn.Linear(4, 1)])
    _refuse(pm, "LayerNorm after a head Linear")


# ------------------------------------------------------------------ C-ABI
def test_abi_is_additive():
    lib = _lib.load()
    for name in ("xpg_forward_workspace_post", "xpg_masked_forward_post", "xpg_forward_describe_post",
                 "xpg_post_rows", "xpg_post_describe"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert _lib.ABI_VERSION == 28 and lib.xpg_abi_version() == 28
    assert [f[0] for f in _lib.LayerDesc._fields_[-2:]] == ["seg_rel", "pool"]
    assert _lib.ForwardPlanDesc._fields_[-1][0] == "dot_scale"
    assert [f[0] for f in _lib.PostDesc._fields_] == ["norm", "eps", "scale", "shift", "gamma", "beta",
                                                      "act", "residual"]
    assert ctypes.sizeof(_lib.PostDesc) == 48


def _post(n, **layers):
    """n records; layers: l<i>=dict(fields)."""
    P = (_lib.PostDesc * n)()
    for k, f in layers.items():
        for name, v in f.items():
            setattr(P[int(k[1:])], name, v)
    return P


def describe_post(desc, post, rows=70):
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load().xpg_forward_describe_post(ctypes.byref(desc), post, rows, buf, len(buf)))
    return buf.value.decode()


def _noact(desc, *layers):
    for l in layers:
        desc.layers[l].act = 0
    return desc


def test_describe_post_null_and_empty_records_are_the_old_entry_point(monkeypatch):
    for layers, kw in (([(SAGE, 128), (SAGE, 128)], dict(n_nodes=10000, n_tgt=10000)),
                       ([(SAGE, 128), (SAGE, 128)], {}), ([(GCN, 32), (GCN, 32)], dict(n_nodes=40, n_tgt=8))):
        desc = make_plan(layers, **kw)
        old = describe(desc)
        assert describe_post(desc, None) == old
        assert describe_post(desc, _post(len(layers))) == old
        n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(_lib.load().xpg_forward_workspace(ctypes.byref(desc), 70, ctypes.byref(n0)))
        _lib.check(_lib.load().xpg_forward_workspace_post(ctypes.byref(desc), None, 70, ctypes.byref(n1)))
        assert n0.value == n1.value > 0
    monkeypatch.setenv("XPG_FORWARD", "rows")
    small = make_plan([(GCN, 32), (GCN, 32)], n_nodes=40, n_tgt=8)
    assert describe_post(small, None) == describe(small) == "rows"


def test_post_plans_run_unfused_and_name_their_kernels(monkeypatch):
    # a small plan the rows kernel would take, a big one the wide path would take
    for kw in (dict(n_nodes=40, n_tgt=8), dict(n_nodes=10000, n_tgt=10000)):
        desc = _noact(make_plan([(SAGE, 32), (SAGE, 32), (SAGE, 32)][:3], **kw), 1, 2)
        post = _post(3, l1=dict(norm=1, eps=1e-5, gamma=PTR, beta=PTR, act=1),
                     l2=dict(scale=PTR, shift=PTR, act=1, residual=1))
        assert describe_post(desc, post) == "unfused post2=k_post<layer,0> post3=k_post<none,1>"
    two = _noact(make_plan([(SAGE, 128), (SAGE, 128)], n_nodes=10000, n_tgt=10000), 1)
    post = _post(2, l1=dict(norm=1, eps=1e-5, act=1, residual=1))
    assert describe(two).startswith("wide")
    assert describe_post(two, post) == "unfused post2=k_post<layer,1>"
    n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    lib = _lib.load()
    _lib.check(lib.xpg_forward_workspace_post(ctypes.byref(two), post, 70, ctypes.byref(n1)))
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    _lib.check(lib.xpg_forward_workspace(ctypes.byref(two), 70, ctypes.byref(n0)))
    assert n0.value == n1.value  # the multi-kernel layout of the same plan
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    assert describe_post(two, post) == "unfused post2=k_post<layer,1>"
    for path in ("rows", "fused", "wide"):
        monkeypatch.setenv("XPG_FORWARD", path)
        with pytest.raises(RuntimeError, match="forced XPG_FORWARD path does not take this plan"):
            describe_post(two, post)
        rc = lib.xpg_masked_forward_post(ctypes.byref(two), post, None, 70, None, None, n1.value, None)
        assert rc == 1  # XPG_EINVAL, before anything is launched
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    for path in ("rows", "fused", "wide"):  # not strict: the fall-back
        monkeypatch.setenv("XPG_FORWARD", path)
        assert describe_post(two, post).startswith("unfused ")


@pytest.mark.parametrize("fields,edit,match", [
    (dict(norm=1, eps=1e-5), "act", "must have act NONE"),
    (dict(norm=2, eps=1e-5), None, "norm outside enum xpg_norm"),
    (dict(norm=-1), None, "norm outside enum xpg_norm"),
    (dict(norm=1, eps=0.0), None, "finite eps > 0"),
    (dict(norm=1, eps=-1.0), None, "finite eps > 0"),
    (dict(norm=1, eps=float("inf")), None, "finite eps > 0"),
    (dict(norm=1, eps=float("nan")), None, "finite eps > 0"),
    (dict(gamma=PTR), None, "gamma / beta need norm LAYER"),
    (dict(act=9), None, "act outside enum xpg_act"),
    (dict(act=1, residual=1), "width", "equal to the previous layer's"),
    (dict(act=1, residual=1), "tgt_prev", "residual needs tgt_prev"),
    (dict(act=1), "edge_masks", "edge-mask plans"),
    (dict(act=1), "edge_dot", "link decoder"),
    (dict(act=1), "n_types", "multi-node-type plans"),
    (dict(act=1), "tgt_type", "multi-node-type plans"),
])
def test_host_checks_of_post_records(fields, edit, match):
    desc = make_plan([(SAGE, 32), (SAGE, 32)])
    if edit != "act":
        _noact(desc, 1)
    if edit == "width":
        desc.layers[1].f_out, desc.layers[1].f_out_pad = 64, 64
        desc.head[0].k_pad = 64
    elif edit == "tgt_prev":
        desc.layers[1].tgt_prev = None
    elif edit in ("edge_masks", "edge_dot"):
        setattr(desc, edit, 1)
    elif edit == "n_types":
        desc.layers[0].n_types = 2
    elif edit == "tgt_type":
        desc.layers[0].tgt_type = PTR
    post = _post(2, l1=fields)
    lib = _lib.load()
    with pytest.raises(RuntimeError, match=match):
        describe_post(desc, post)
    n = ctypes.c_size_t(0)
    assert lib.xpg_forward_workspace_post(ctypes.byref(desc), post, 70, ctypes.byref(n)) == 1
    assert lib.xpg_masked_forward_post(ctypes.byref(desc), post, None, 70, None, None, 1 << 30, None) == 1
    assert match in lib.xpg_last_error().decode()


def test_residual_on_layer_one_is_refused():
    desc = _noact(make_plan([(SAGE, 32), (SAGE, 32)]), 0)
    with pytest.raises(RuntimeError, match="residual on layer 1"):
        describe_post(desc, _post(2, l0=dict(act=1, residual=1)))


def test_post_describe_names_the_lane_group():
    lib = _lib.load()

    def d(M, ld, f_out, **f):
        buf = ctypes.create_string_buffer(128)
        pd = _lib.PostDesc(**f)
        _lib.check(lib.xpg_post_describe(M, ld, f_out, ctypes.byref(pd), buf, len(buf)))
        return buf.value.decode()
    assert d(10, 8, 5, norm=1, eps=1e-5) == "k_post<layer,0> group=2 rows_per_wave=32"
    assert d(10, 32, 32, act=1, residual=1) == "k_post<none,1> group=8 rows_per_wave=8"
    assert d(10, 64, 40, norm=1, eps=1e-5, residual=1) == "k_post<layer,1> group=16 rows_per_wave=4"
    assert d(10, 96, 96, act=1) == "k_post<none,0> group=32 rows_per_wave=2"  # 24 chunks, 8 idle lanes
    assert d(10, 256, 256, act=1) == "k_post<none,0> group=64 rows_per_wave=1"
    for bad in ((10, 6, 5), (10, 260, 5), (10, 8, 9), (10, 8, 0), (-1, 8, 5)):
        buf = ctypes.create_string_buffer(128)
        pd = _lib.PostDesc(act=1)
        assert lib.xpg_post_describe(*bad, ctypes.byref(pd), buf, len(buf)) == 1
    pd = _lib.PostDesc(norm=1, eps=0.0)
    assert lib.xpg_post_rows(None, 0, 8, 5, ctypes.byref(pd), None, 0, 0, 0, None, None) == 1
    pd = _lib.PostDesc(act=1)
    assert lib.xpg_post_rows(None, 0, 8, 5, ctypes.byref(pd), None, 0, 0, 0, None, None) == 0  # M = 0


# ------------------------------------------------------------------ the GPU cases, on the reference alone
@pytest.mark.parametrize("name", block_ref.PLAN_CASES + block_ref.PATH_CASES + block_ref.POOLED_CASES)
def test_gpu_cases_move_with_masks_norms_and_skips(name):
    """On each input of tests/test_gpu_blocks.py: at least half the outputs differ from the all-on
    row's by more than 1e-3; removing the norms, and separately the skips, moves at least half the
    outputs by more than 1e-3; the float32 CPU module is within 1e-6 of fp64."""
    c = block_ref.case(name)
    arch, x, ei, m = c["arch"], c["x"].numpy(), c["ei"], c["masks"]
    ref = c["ref"]
    spread = float(np.mean(np.abs(ref - ref[1]) > 1e-3))
    outs = block_ref.pooled_outputs if c["pooled"] else block_ref.union_outputs
    pick = (lambda y: y) if c["pooled"] else (lambda y: y[:, block_ref.QUERIES])
    no_norm = float(np.mean(np.abs(pick(outs(arch, x, ei, m, drop_norm=True)) - ref) > 1e-3))
    enc = arch.encoder if c["pooled"] else arch
    e64 = float(np.abs(pick(block_ref.module_outputs(arch, x, ei, m)) - ref).max())
    e32 = float(np.abs(pick(block_ref.module_outputs(arch, x, ei, m, torch.float32)) - ref).max())
    print(name, "spread", spread, "norm moves", no_norm, "module fp64", e64, "e32", e32)
    assert e64 < 1e-12
    assert spread >= 0.5 and no_norm >= 0.5
    if enc.residual:
        no_res = float(np.mean(np.abs(pick(outs(arch, x, ei, m, drop_residual=True)) - ref) > 1e-3))
        print(name, "skip moves", no_res)
        assert no_res >= 0.5
    assert e32 < 1e-6
