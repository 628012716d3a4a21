"""Graphs with edge features (edge_attr for GINEConv) without a GPU: nn.py's modules against the
fp64 restatement of tests/edge_attr_ref.py, the lowering, the plan's edge-feature arrays against a
brute-force loop, the C-ABI's host checks on synthetic descriptors (nothing is launched), the
Explainer / pipeline refusals, and the non-vacuity of the GPU cases (asserted about the reference
alone)."""
import ctypes

import numpy as np
import pytest
import torch

import edge_attr_ref as ear
from test_aggr_cpu import make_plan as make_plan_raw
from test_dispatch_cpu import ENV, GCN, PTR, SAGE, describe, make_plan

from bikg_graph_explainability_public_amd import _lib, engine, pipeline
from bikg_graph_explainability_public_amd import nn as xnn
from bikg_graph_explainability_public_amd.model import Model
from bikg_graph_explainability_public_amd.nn import BlockStack, ConvStack, PooledModel
from bikg_graph_explainability_public_amd.program import UnsupportedArch, compile_arch, count_message_passing

TAG = "efeat=k_agg_e"


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    for k in tuple(ENV) + ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_EFEAT_MSG"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------ nn.py against the restatement
def _graph(dim=5):
    """12 nodes: duplicate edges with different rows (2 -> 3 twice, 5 -> 1 three times), node 4 with
    two self-loops with different rows, node 9 with one, node 11 isolated."""
    ei = np.array([[0, 1, 2, 2, 4, 5, 5, 5, 6, 4, 7, 8, 9, 3, 10, 0, 6, 4],
                   [1, 2, 3, 3, 4, 1, 1, 1, 0, 5, 6, 7, 9, 8, 0, 10, 4, 4]], dtype=np.int64)
    g = np.random.default_rng(7)
    ea = g.standard_normal((ei.shape[1], dim))
    x = g.standard_normal((12, 6))
    l4 = np.nonzero((ei[0] == 4) & (ei[1] == 4))[0]
    assert l4.size == 2 and not np.array_equal(ea[l4[0]], ea[l4[1]]) and not np.array_equal(ea[2], ea[3])
    assert 11 not in ei
    return ei, ea, x


def _mlp(i, o):
    return torch.nn.Sequential(xnn.Linear(i, o), torch.nn.ReLU(), xnn.Linear(o, o))


@pytest.mark.parametrize("edge_dim", [1, 5, None])
def test_gineconv_equals_the_restatement_in_double(edge_dim):
    ei, ea, x = _graph(6 if edge_dim is None else edge_dim)
    torch.manual_seed(3)
    conv = xnn.GINEConv(_mlp(6, 5), eps=0.25, edge_dim=edge_dim).double().eval()
    assert (conv.lin is None) == (edge_dim is None)
    assert edge_dim is None or tuple(conv.lin.weight.shape) == (6, edge_dim)
    with torch.no_grad():
        got = conv(torch.as_tensor(x), torch.as_tensor(ei), edge_attr=torch.as_tensor(ea)).numpy()
    ref = ear.gine_conv(conv, x, ei[0], ei[1], ea)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    # the isolated node has its (1 + eps) x root term and an empty sum
    np.testing.assert_allclose(got[11], ear.mlp_rows(conv.nn, 1.25 * x[11:12])[0], rtol=0, atol=1e-12)
    # the rows matter: zero attributes, and the two loops' / the duplicates' rows swapped with a
    # third edge's row, give other outputs
    assert np.abs(ref - ear.gine_conv(conv, x, ei[0], ei[1], np.zeros_like(ea))).max() > 1e-3
    if edge_dim == 1:  # a 1-D tensor of length E is D = 1
        with torch.no_grad():
            flat = conv(torch.as_tensor(x), torch.as_tensor(ei), edge_attr=torch.as_tensor(ea[:, 0])).numpy()
        assert np.array_equal(flat, got)


def test_gineconv_train_eps_and_width_mismatch():
    ei, ea, x = _graph(5)
    conv = xnn.GINEConv(_mlp(6, 5), eps=0.5, train_eps=True).double()
    assert isinstance(conv.eps, torch.nn.Parameter) and conv.lin is None and conv.aggr == "add"
    with pytest.raises(ValueError, match="do not match"):
        conv(torch.as_tensor(x), torch.as_tensor(ei), edge_attr=torch.as_tensor(ea))  # 5 != 6
    with pytest.raises(ValueError, match="edge_attr"):
        conv(torch.as_tensor(x), torch.as_tensor(ei))


@pytest.mark.parametrize("edge_dim", [1, 5, None])
def test_stacks_equal_the_restatement_in_double(edge_dim):
    ei, ea, x = _graph(6 if edge_dim is None else edge_dim)
    masks = np.ones((2, 12), dtype=bool)
    masks[1, [3, 4]] = False
    dims = [6, 6, 6] if edge_dim is None else [6, 8, 8]
    torch.manual_seed(5)
    import block_ref
    for arch in (ConvStack("gine", dims, [dims[-1], 1], edge_dim=edge_dim),
                 block_ref.randomise_norms(BlockStack("gine", dims, [dims[-1], 1], norm="batch", edge_dim=edge_dim), 2),
                 block_ref.randomise_norms(BlockStack("gine", dims, [dims[-1], 1], norm="layer", edge_dim=edge_dim), 3),
                 PooledModel(ConvStack("gine", dims, [dims[-1]], edge_dim=edge_dim), "add", [dims[-1], 1])):
        arch = arch.double().eval()
        got = ear.module_outputs(arch, x, ei, ea, masks, torch.float64)
        ref = ear.union_outputs(arch, x, ei, ea, masks)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
        assert np.abs(ref - ear.union_outputs(arch, x, ei, np.zeros_like(ea), masks)).max() > 1e-4


def test_stacks_refuse_both_keywords_and_a_stray_edge_dim():
    ei, ea, x = _graph(5)
    xt, eit, eat = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(ei), torch.as_tensor(ea, dtype=torch.float32)
    for arch in (ConvStack("gine", [6, 8], [8, 1], edge_dim=5), BlockStack("gine", [6, 8], [8, 1], edge_dim=5)):
        with pytest.raises(ValueError, match="together"):
            arch(xt, eit, edge_weight=torch.ones(18), edge_attr=eat)
    with pytest.raises(ValueError, match="together"):
        PooledModel(ConvStack("gine", [6, 8], [8], edge_dim=5), "add", [8, 1])(
            xt, eit, None, edge_weight=torch.ones(18), edge_attr=eat)
    with pytest.raises(ValueError, match="edge_dim"):
        ConvStack("gin", [6, 8], [8, 1], edge_dim=5)
    with pytest.raises(ValueError, match="edge_dim"):
        BlockStack("gcn", [6, 8], [8, 1], edge_dim=5)


def test_forward_signatures_keep_their_call_forms():
    """The trailing edge_attr keyword is no part of the call convention: a ConvStack is still a
    two-parameter model, a PooledModel still the (x, edge_index, batch) form; Model.infer passes
    the keyword on in both."""
    ei, ea, x = _graph(5)
    xt, eit, eat = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(ei), torch.as_tensor(ea, dtype=torch.float32)
    cs = ConvStack("gine", [6, 8], [8, 1], edge_dim=5).eval()
    pm = PooledModel(ConvStack("gine", [6, 8], [8], edge_dim=5), "mean", [8, 1]).eval()
    assert not pipeline.pooled_call(cs) and not pipeline.pooled_call(BlockStack("gine", [6, 8], [8, 1], edge_dim=5))
    assert pipeline.pooled_call(pm)
    with torch.no_grad():
        assert torch.equal(Model(cs).infer(xt, eit, edge_attr=eat), cs(xt, eit, edge_attr=eat))
        b = torch.zeros(12, dtype=torch.long)
        assert torch.equal(Model(pm).infer(xt, eit, batch=b, edge_attr=eat), pm(xt, eit, b, edge_attr=eat))
    with pytest.raises(ValueError, match="together"):
        Model(cs).infer(xt, eit, edge_weight=torch.ones(18), edge_attr=eat)
    assert count_message_passing(cs) == 1 and Model(cs).get_hops(0) == 1


# ------------------------------------------------------------------ lowering
def test_lowering_is_gins_own_with_the_edge_map_on_the_term():
    torch.manual_seed(1)
    gine = ConvStack("gine", [6, 8, 8], [8, 1], edge_dim=5).eval()
    gin = ConvStack("gin", [6, 8, 8], [8, 1]).eval()
    with torch.no_grad():
        for i in (0, 2):
            gine.conv[i].eps.fill_(0.3)
            gin.conv[i].eps.fill_(0.3)
            gin.conv[i].nn.load_state_dict(gine.conv[i].nn.state_dict())
    p, q = compile_arch(gine, edge_attr=True), compile_arch(gin)
    assert p.edge_featured is True and q.edge_featured is False and p.weighted is False
    assert p.extra_layers == q.extra_layers == 2 and p.hops == 2 and len(p.convs) == 4
    for li, (a, b) in enumerate(zip(p.convs, q.convs)):
        assert [t.kind for t in a.terms] == [t.kind for t in b.terms] == (["sum", "root"] if li % 2 == 0 else ["root"])
        assert a.act == b.act and a.f_in == b.f_in and a.f_out == b.f_out and torch.equal(a.bias, b.bias)
        for s, t in zip(a.terms, b.terms):
            assert torch.equal(s.weight, t.weight)
            assert t.edge_lin_w is None and t.edge_lin_b is None
        conv = gine.conv[li - li % 2]
        if li % 2 == 0:
            assert torch.equal(a.terms[0].edge_lin_w, conv.lin.weight) and tuple(a.terms[0].edge_lin_w.shape) == (a.f_in, 5)
            assert torch.equal(a.terms[0].edge_lin_b, conv.lin.bias)
            root = ((1.0 + float(conv.eps)) * conv.nn[0].weight.detach().double()).float()
            assert torch.equal(a.terms[1].weight, root) and a.terms[1].edge_lin_w is None
        else:
            assert a.terms[0].edge_lin_w is None
    none = compile_arch(ConvStack("gine", [6, 6, 6], [6, 1]).eval(), edge_attr=True)
    assert all(t.edge_lin_w is None and t.edge_lin_b is None for c in none.convs for t in c.terms)


def test_batchnorm_folds_as_gins_does_and_containers_compile():
    import block_ref
    torch.manual_seed(2)
    a = block_ref.randomise_norms(BlockStack("gine", [6, 8, 8], [8, 1], norm="batch", edge_dim=5), 4).eval()
    b = BlockStack("gin", [6, 8, 8], [8, 1], norm="batch").eval()
    for i in range(0, len(a.conv), a.block_len):
        b.conv[i].nn.load_state_dict(a.conv[i].nn.state_dict())
    p, q = compile_arch(a, edge_attr=True), compile_arch(b)
    for x, y in zip(p.convs, q.convs):
        assert torch.equal(x.bias, y.bias) and all(torch.equal(s.weight, t.weight) for s, t in zip(x.terms, y.terms))
    assert not p.has_post and p.edge_featured
    ln = compile_arch(BlockStack("gine", [6, 8, 8], [8, 1], norm="layer", edge_dim=5).eval(), edge_attr=True)
    assert ln.has_post and ln.edge_featured
    pm = compile_arch(PooledModel(ConvStack("gine", [6, 8, 8], [8], edge_dim=5), "add", [8, 1]).eval(), edge_attr=True)
    assert pm.pool == "sum" and pm.edge_featured
    with pytest.raises(UnsupportedArch, match="skip would span"):
        compile_arch(BlockStack("gine", [6, 8, 8], [8, 1], residual=True, edge_dim=5).eval(), edge_attr=True)


def test_compile_arch_refusals():
    gine = ConvStack("gine", [6, 8, 8], [8, 1], edge_dim=5).eval()
    with pytest.raises(UnsupportedArch, match="GINEConv needs edge_attr"):
        compile_arch(gine)
    with pytest.raises(UnsupportedArch, match="GINEConv needs edge_attr"):
        compile_arch(PooledModel(ConvStack("gine", [6, 8], [8], edge_dim=5), "add", [8, 1]).eval())
    for arch, kw in ((ConvStack("sage", [6, 8, 8], [8, 1]), {}), (ConvStack("gin", [6, 8, 8], [8, 1]), {}),
                     (ConvStack("gcn", [6, 8, 8], [8, 1]), {}), (ConvStack("graphconv", [6, 8, 8], [8, 1]), {}),
                     (ConvStack("gat", [6, 8, 8], [8, 1]), {"attention": True}),
                     (xnn.RGCNStack([6, 8, 8], [8, 1], 3), {}),
                     (BlockStack("gcn", [6, 8, 8], [8, 1], norm="layer"), {}),
                     (PooledModel(ConvStack("sage", [6, 8, 8], [8]), "mean", [8, 1]), {})):
        compile_arch(arch.eval(), **kw)
        with pytest.raises(UnsupportedArch, match="takes no edge_attr"):
            compile_arch(arch.eval(), edge_attr=True, **kw)
    mixed = ConvStack("gine", [6, 8, 8], [8, 1], edge_dim=5)
    mixed.conv[2] = xnn.GCNConv(8, 8)
    with pytest.raises(UnsupportedArch, match="GCNConv takes no edge_attr"):
        compile_arch(mixed.eval(), edge_attr=True)
    with pytest.raises(UnsupportedArch, match="link"):
        compile_arch(xnn.LinkModel(ConvStack("gine", [6, 8, 8], [8], edge_dim=5)).eval(), edge_attr=True)
    with pytest.raises(UnsupportedArch, match="typed"):
        compile_arch(gine, edge_type_names=[("n", "a", "n")], edge_attr=True)
    with pytest.raises(UnsupportedArch, match="edge_weight"):
        compile_arch(gine, edge_weight=True, edge_attr=True)
    het = torch.nn.Module()
    het.conv = torch.nn.ModuleList([xnn.HeteroConv({("n", "a", "n"): xnn.GINEConv(xnn.Linear(6, 8), edge_dim=5)})])
    with pytest.raises(UnsupportedArch, match="GINEConv inside HeteroConv"):
        compile_arch(het.eval(), edge_type_names=[("n", "a", "n")])


def test_program_cache_is_keyed_on_the_flag():
    pipeline.clear_programs()
    arch = ConvStack("gine", [6, 8, 8], [8, 1], edge_dim=5).eval()
    b = pipeline.compiled_program(arch, edge_attr=True)
    assert b.edge_featured and pipeline.compiled_program(arch, edge_attr=True) is b
    with pytest.raises(UnsupportedArch):
        pipeline.compiled_program(arch)
    pipeline.clear_programs()


# ------------------------------------------------------------------ plan arrays
@pytest.mark.parametrize("edge_dim", [5, None])
def test_edge_feature_arrays_against_a_brute_force_loop(edge_dim):
    ei, ea, x = _graph(6 if edge_dim is None else edge_dim)
    ea, x = ea.astype(np.float32), x.astype(np.float32)
    E = ei.shape[1]
    queries = [1, 4, 9]
    torch.manual_seed(4)
    dims = [6, 6, 6] if edge_dim is None else [6, 40, 8]
    prog = compile_arch(ConvStack("gine", dims, [dims[-1], 1], edge_dim=edge_dim).eval(), edge_attr=True)
    L = len(prog.convs)
    arr = engine.plan_arrays(12, [ei], queries, L, [np.arange(E, dtype=np.int64)])
    fr = arr["frontiers"]
    x0 = x[np.asarray(fr[0])]
    fa = engine.edge_feature_arrays(arr, prog.convs, ea, x0)
    assert len(fa) == L and [a is None for a in fa] == [False, True, False, True]
    for li in (0, 2):
        conv, lay, got = prog.convs[li], arr["layers"][li], fa[li]
        term = conv.terms[0]
        if edge_dim is None:
            EE = ea
        else:
            EE = (ea.astype(np.float64) @ term.edge_lin_w.double().numpy().T
                  + term.edge_lin_b.double().numpy()).astype(np.float32)
        pad = (conv.f_in + 31) // 32 * 32
        agg_rows, self_rows, msg_agg, msg_self = [], [], [], []
        for ti, t in enumerate(fr[li + 1]):
            for e in range(E):  # in-edges in edge order, the loops apart
                if ei[1, e] == t and ei[0, e] != t:
                    agg_rows.append(EE[e])
                    msg_agg.append(np.maximum(x[ei[0, e]] + EE[e], np.float32(0)) if li == 0 else None)
            for e in range(E):
                if ei[1, e] == t and ei[0, e] == t:
                    self_rows.append(EE[e])
                    msg_self.append(np.maximum(x[t] + EE[e], np.float32(0)) if li == 0 else None)
        assert got["agg_e"].shape == (len(agg_rows), pad) == (lay["agg_src"].size, pad)
        assert got["self_e"].shape == (len(self_rows), pad) and got["agg_e"].dtype == np.float32
        assert np.array_equal(got["agg_e"][:, :conv.f_in], np.array(agg_rows, np.float32).reshape(-1, conv.f_in))
        assert np.array_equal(got["self_e"][:, :conv.f_in], np.array(self_rows, np.float32).reshape(-1, conv.f_in))
        assert not got["agg_e"][:, conv.f_in:].any() and not got["self_e"][:, conv.f_in:].any()  # exactly 0
        if li == 0:
            msg = np.array(msg_agg + msg_self, np.float32).reshape(-1, conv.f_in)
            assert got["msg_rows"].dtype == np.float32 and got["msg_rows"].shape == (msg.shape[0], pad)
            assert np.array_equal(got["msg_rows"][:, :conv.f_in], msg)  # bit for bit in fp32
            assert not got["msg_rows"][:, conv.f_in:].any()
            assert len(self_rows) >= 2  # node 4's two loops are among the targets'
        else:
            assert "msg_rows" not in got
    if edge_dim is None:
        with pytest.raises(ValueError, match="width"):
            engine.edge_feature_arrays(arr, prog.convs, ea[:, :5], x0)
    else:
        with pytest.raises(ValueError, match="edge_dim"):
            engine.edge_feature_arrays(arr, prog.convs, ea[:, :3], x0)


def test_check_edge_attr():
    ok = engine.check_edge_attr(torch.tensor([[0.5, 2.0], [0.0, -1.0]], dtype=torch.float64), 2)
    assert ok.dtype == np.float32 and ok.tolist() == [[0.5, 2.0], [0.0, -1.0]]
    assert engine.check_edge_attr(torch.tensor([1.0, 2.0, 3.0]), 3).shape == (3, 1)
    with pytest.raises(ValueError, match="one row per edge"):
        engine.check_edge_attr(torch.ones(4, 2), 3)
    with pytest.raises(ValueError, match="one row per edge"):
        engine.check_edge_attr(torch.ones(3, 2, 2), 3)
    with pytest.raises(ValueError, match="finite"):
        engine.check_edge_attr(torch.tensor([[1.0], [float("nan")]]), 2)
    with pytest.raises(ValueError, match="finite"):
        engine.check_edge_attr(torch.tensor([[1.0], [float("inf")]]), 2)
    with pytest.raises(ValueError, match="floating"):
        engine.check_edge_attr(torch.tensor([[1], [2]]), 2)


# ------------------------------------------------------------------ C-ABI
def test_abi_is_additive():
    lib = _lib.load()
    for name in ("xpg_forward_workspace_e", "xpg_masked_forward_e", "xpg_forward_describe_e",
                 "xpg_forward_workspace_w", "xpg_masked_forward_w", "xpg_forward_describe_w"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert _lib.ABI_VERSION == 28 and lib.xpg_abi_version() == 28
    assert ctypes.sizeof(_lib.LayerEfeat) == 24 and ctypes.sizeof(_lib.EdgeFeats) == 8
    assert ctypes.sizeof(_lib.LayerWeights) == 32 and ctypes.sizeof(_lib.EdgeWeights) == 24
    assert ctypes.sizeof(_lib.PostDesc) == 48
    assert [f[0] for f in _lib.LayerDesc._fields_[-2:]] == ["seg_rel", "pool"]
    assert _lib.ForwardPlanDesc._fields_[-1][0] == "dot_scale"


SUM = ("sum", "root")
ROOT = ("root",)
SMALL = dict(n_nodes=40, n_tgt=8)


def gine_plan(layers=((SUM, 32), (ROOT, 32), (SUM, 32), (ROOT, 32)), **kw):
    """A raw-form descriptor (every layer aggregate-then-transform) with self_ptr set."""
    d = make_plan_raw(list(layers), raw=True, **dict(SMALL, **kw))
    for l in range(len(layers)):
        d.layers[l].self_ptr = PTR
    return d


def _feats(n, msg=True):
    LE = (_lib.LayerEfeat * n)()
    for l, le in enumerate(LE):
        le.agg_e = le.self_e = PTR
        le.msg_rows = PTR if (msg and l == 0) else None
    F = _lib.EdgeFeats(layers=LE)
    F._keep = LE
    return F


def _weights(n):
    LW = (_lib.LayerWeights * n)()
    for lw in LW:
        lw.agg_w = lw.self_sum = lw.self_wmax = lw.self_wmin = PTR
    W = _lib.EdgeWeights(deg_w=PTR, loop_w=PTR, layers=LW)
    W._keep = LW
    return W


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def describe_e(desc, post, wts, fe, rows=70):
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.load().xpg_forward_describe_e(ctypes.byref(desc), post, _ref(wts), _ref(fe), rows, buf, len(buf)))
    return buf.value.decode()


def workspace_e(desc, post, wts, fe, rows=70):
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_forward_workspace_e(ctypes.byref(desc), post, _ref(wts), _ref(fe), rows, ctypes.byref(n)))
    return n.value


def _refused(desc, fe, match, wts=None):
    with pytest.raises(RuntimeError, match=match):
        describe_e(desc, None, wts, fe)
    with pytest.raises(RuntimeError, match=match):
        workspace_e(desc, None, wts, fe)
    y = ctypes.c_void_p(0)
    rc = _lib.load().xpg_masked_forward_e(ctypes.byref(desc), None, _ref(wts), ctypes.byref(fe), y, 70, y, y, 0, y)
    assert rc == 1  # XPG_EINVAL, before any launch (no workspace, no device pointer read)


def test_null_feats_are_the_w_entry_points():
    lib = _lib.load()
    for layers, kw in (([(SAGE, 128), (SAGE, 128)], dict(n_nodes=10000, n_tgt=10000)),
                       ([(SAGE, 128), (SAGE, 128)], {}), ([(GCN, 32), (GCN, 32)], SMALL)):
        desc = make_plan(layers, **kw)
        assert describe_e(desc, None, None, None) == describe(desc)
        n0 = ctypes.c_size_t(0)
        _lib.check(lib.xpg_forward_workspace(ctypes.byref(desc), 70, ctypes.byref(n0)))
        assert workspace_e(desc, None, None, None) == n0.value > 0
    desc = make_plan([(GCN, 32), (GCN, 32)], **SMALL)
    W = _weights(2)
    buf = ctypes.create_string_buffer(512)
    _lib.check(lib.xpg_forward_describe_w(ctypes.byref(desc), None, ctypes.byref(W), 70, buf, len(buf)))
    assert describe_e(desc, None, W, None) == buf.value.decode() == "unfused weights=k_degree_w+k_agg_w"
    n1 = ctypes.c_size_t(0)
    _lib.check(lib.xpg_forward_workspace_w(ctypes.byref(desc), None, ctypes.byref(W), 70, ctypes.byref(n1)))
    assert workspace_e(desc, None, W, None) == n1.value


def test_edge_featured_plans_take_the_multi_kernel_path():
    d = gine_plan()
    assert describe_e(d, None, None, _feats(4)) == "unfused " + TAG
    assert describe_e(d, None, None, _feats(4, msg=False)) == "unfused " + TAG
    big = gine_plan(n_nodes=10000, n_tgt=10000)
    assert describe_e(big, None, None, _feats(4)) == "unfused " + TAG
    # post tokens follow
    d = gine_plan()
    d.layers[3].act = 0
    P = (_lib.PostDesc * 4)()
    P[3].norm, P[3].eps, P[3].act = 1, 1e-5, 1
    assert describe_e(d, P, None, _feats(4)) == "unfused " + TAG + " post4=k_post<layer,0>"


def test_workspace_is_the_multi_kernel_layout_of_the_same_plan():
    for rows in (1, 70):
        d = gine_plan()
        P = (_lib.PostDesc * 4)()  # no post-op: the multi-kernel layout of the same plan
        assert workspace_e(d, None, None, _feats(4), rows) == workspace_e(d, P, None, None, rows) > 0
    assert workspace_e(gine_plan(), None, None, _feats(4), 16) < workspace_e(gine_plan(), None, None, _feats(4), 64)


def test_host_checks():
    F = _feats(4)
    d = gine_plan()
    d.edge_masks = 1
    _refused(d, F, "edge_masks")
    d = gine_plan()
    d.edge_dot = 1
    _refused(d, F, "edge_dot")
    d = gine_plan()
    d.n_rel = 2
    _refused(d, F, "n_rel")
    d = gine_plan()
    d.layers[2].tgt_type = PTR
    _refused(d, F, "tgt_type")
    for kind in ("att", "att2", "rel", "gcn", "mean", "max"):
        d = gine_plan(layers=((SUM, 32), ((kind,), 32)))
        _refused(d, _feats(2), "SUM / ROOT terms only")
    d = gine_plan()
    for field in ("agg_e", "self_e"):
        for l in (0, 2):
            F2 = _feats(4)
            setattr(F2.layers[l], field, None)
            _refused(d, F2, "layer record misses")
    F3 = _feats(4)
    F3.layers[1].agg_e = F3.layers[1].self_e = None  # a ROOT-only layer's record is not read
    assert TAG in describe_e(d, None, None, F3)
    F4 = _feats(4)
    F4.layers = None
    _refused(d, F4, "layer records")
    F5 = _feats(4)
    F5.layers[2].msg_rows = PTR
    _refused(d, F5, "layer 1 only")
    d = gine_plan()
    d.layers[2].self_ptr = None
    _refused(d, F, "self_ptr")
    _refused(gine_plan(), F, "edge weights together", wts=_weights(4))
    # the table form of layer 1 is not taken
    d = make_plan([(SUM, 32), (SUM, 32)], **SMALL)
    for l in range(2):
        d.layers[l].self_ptr = PTR
    _refused(d, _feats(2), "aggregate-then-transform")


@pytest.mark.parametrize("path", ["rows", "fused", "wide"])
def test_forced_paths_are_refused_under_strict(path, monkeypatch):
    d = gine_plan()
    monkeypatch.setenv("XPG_FORWARD", path)
    assert TAG in describe_e(d, None, None, _feats(4))  # not strict: falls back
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="forced XPG_FORWARD path"):
        describe_e(d, None, None, _feats(4))
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    assert describe_e(d, None, None, _feats(4)) == "unfused " + TAG


# ------------------------------------------------------------------ data helpers
def test_comp_graph_carries_the_rows():
    from bikg_graph_explainability_public_amd.data import Data
    ei, ea, x = _graph(5)
    feat, eit, eat = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(ei), torch.as_tensor(ea, dtype=torch.float32)
    names = [str(i) for i in range(12)]
    data = Data(feat, eit)
    plain = data.comp_graph(3, 1, "node_prediction", names, return_pos=True)
    out = data.comp_graph(3, 1, "node_prediction", names, return_pos=True, edge_attr=eat)
    assert len(out) == len(plain) + 1
    sub_ei, pos, sub_a = out[1], out[6], out[-1]
    assert torch.equal(sub_ei, plain[1]) and sub_a.shape == (sub_ei.shape[1], 5)
    # every kept edge carries its own row: look each one up in the full graph (duplicates share ends)
    orig = torch.as_tensor(pos)[sub_ei]
    for k in range(sub_ei.shape[1]):
        cands = [e for e in range(18) if ei[0, e] == int(orig[0, k]) and ei[1, e] == int(orig[1, k])]
        assert any(torch.equal(sub_a[k], eat[e]) for e in cands)
    # the isolated node: the fabricated self-loop gets a zero row
    iso = data.comp_graph(11, 1, "node_prediction", names, edge_attr=eat)
    assert iso[1].shape == (2, 1) and torch.equal(iso[-1], torch.zeros(1, 5))


# ------------------------------------------------------------------ Explainer refusals
def _explainer(arch=None, ea="ok", **kw):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    ei, eav, x = _graph(5)
    feat, eit = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(ei)
    eat = torch.as_tensor(eav, dtype=torch.float32) if isinstance(ea, str) else ea
    params = dict({"seed": 1, "interpret_samples": 10, "epochs": 8, "optimizer": "adam", "lr": 0.01,
                   "lr_patience": 10, "l1_lambda": 1e-4}, **kw.pop("params", {}))
    arch = ConvStack("gine", [6, 8, 8], [8, 1], edge_dim=5).eval() if arch is None else arch
    args = dict(problem="node_prediction", edge_attr=eat)
    args.update(kw)
    return Explainer(args.pop("feat", feat), args.pop("edge_index", eit), arch, params,
                     args.pop("names", [str(i) for i in range(12)]), None, None, None, **args)


def test_explainer_refusals():
    assert _explainer().edge_attr is not None
    with pytest.raises(ValueError, match="one row per edge"):
        _explainer(ea=torch.ones(5, 5))
    bad = torch.ones(18, 5)
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        _explainer(ea=bad)
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        _explainer(ea=bad)
    with pytest.raises(ValueError, match="floating"):
        _explainer(ea=torch.ones(18, 5, dtype=torch.long))
    with pytest.raises(TypeError, match="torch tensor"):
        _explainer(ea=np.ones((18, 5), np.float32))
    with pytest.raises(NotImplementedError, match="edge_weight"):
        _explainer(edge_weight=torch.ones(18))
    with pytest.raises(NotImplementedError, match="hetero"):
        ei, _, x = _graph()
        _explainer(feat={"n": torch.as_tensor(x, dtype=torch.float32)},
                   edge_index={("n", "a", "n"): torch.as_tensor(ei)}, names={"n": [str(i) for i in range(12)]})
    with pytest.raises(NotImplementedError, match="node_types / edge_types"):
        _explainer(edge_types=torch.zeros(18))
    with pytest.raises(NotImplementedError, match="node_types / edge_types"):
        _explainer(node_types=torch.zeros(12))
    with pytest.raises(NotImplementedError, match="edge masks"):
        _explainer(params={"edge_masks": True}, problem="edge_prediction")
    with pytest.raises(NotImplementedError, match="link_prediction"):
        _explainer(problem="link_prediction")

    class NoKeyword(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = ConvStack("gcn", [6, 8, 8], [8, 1])

        def forward(self, x, edge_index):
            return self.inner(x, edge_index)
    with pytest.raises(TypeError, match="no edge_attr parameter"):
        _explainer(NoKeyword().eval())
    with pytest.raises(TypeError, match="no edge_attr parameter"):
        pipeline.generic_outputs(NoKeyword().eval(), None, None, None, 0, "node_prediction",
                                 edge_attr=torch.ones(18, 5))
    with pytest.raises(TypeError, match="no edge_attr parameter"):
        pipeline.build_plan(NoKeyword().eval(), None, torch.zeros((2, 18)), [0], edge_attr=torch.ones(18, 5))
    with pytest.raises(NotImplementedError, match="typed"):
        pipeline.build_plan(ConvStack("gine", [6, 8], [8, 1], edge_dim=5).eval(), None, torch.zeros((2, 18)), [0],
                            edge_type=torch.zeros(18), edge_attr=torch.ones(18, 5))


def test_an_arch_with_other_convs_and_the_keyword_falls_to_the_generic_path():
    """A model that takes edge_attr but is no GINE stack: build_plan warns and returns None (the
    generic path then runs it)."""
    class Mixed(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = ConvStack("gcn", [6, 8, 8], [8, 1])

        def forward(self, x, edge_index, edge_attr=None):
            return self.inner(x, edge_index)
    ei, ea, x = _graph(5)
    with pytest.warns(UserWarning, match="generic torch path"):
        plan = pipeline.build_plan(Mixed().eval(), torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(ei), [0],
                                   edge_attr=torch.as_tensor(ea, dtype=torch.float32))
    assert plan is None


# ------------------------------------------------------------------ the GPU cases are not vacuous
@pytest.mark.parametrize("name", sorted(ear.CASES))
def test_gpu_cases_depend_on_the_attributes_and_the_masks(name):
    """About the reference alone: on tests/test_gpu_edge_attr.py's graph and models the fp64 outputs
    with the attributes differ from those with all-zero attributes by more than 1e-3 (100 x the
    parity bar), in every case and for both heads; they vary over the mask rows, and at least half
    of the sigmoid outputs lie off the tails."""
    for act in ("sigmoid", "identity"):
        c = ear.case(name, act)
        assert c["ref"].shape == (ear.ROWS, 3)
        assert np.abs(c["ref"] - c["ref0"]).max() > 1e-3
        assert np.ptp(c["ref"]) > 1e-3 and np.ptp(c["ref"][:, 0]) > 1e-3
    ref = ear.case(name)["ref"]
    assert np.mean((ref > 0.02) & (ref < 0.98)) >= 0.5
    ei = ear.case(name)["ei"]
    assert ear.ISOLATED not in ei and ((ei[0] == 7) & (ei[1] == 7)).sum() == 2


@pytest.mark.parametrize("kind,S", [("gine", 60), ("pooled-gine", 30)])
def test_explainer_cases_depend_on_the_attributes(kind, S):
    """The Explainer.run cases of the GPU tests, about the reference alone: over random mask rows
    the fp64 outputs at the query vary by more than 1e-2 and move by more than 1e-2 when the
    attributes are zeroed (the runs are compared at 1e-4)."""
    import pool_ref
    arch, feat, ei, ea, q = ear.explainer_inputs(kind, S)
    masks = pool_ref.row_masks(64, S, 3)
    a = ear.union_outputs(arch, feat.numpy(), ei, ea, masks)
    b = ear.union_outputs(arch, feat.numpy(), ei, np.zeros_like(ea), masks)
    if a.ndim == 2:
        a, b = a[:, q], b[:, q]
    assert np.ptp(a) > 1e-2 and np.abs(a - b).max() > 1e-2
    assert ((ei[0] == q) & (ei[1] == q)).sum() >= 2
