"""Typed link models under edge masks, without a GPU: nn.RelLinkModel against the fp64
restatement of tests/rel_edge_ref.py, its lowering (link_act / link_rel), the generic path with
edge types, the typed edge columns of a plan, ABI v27 (dot_scale, REL + edge_masks host checks,
workspace sizes pinned to the v26 library's) and the refusals that stay."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import rel_edge_ref as ref
from bikg_graph_explainability_public_amd import _lib, engine, pipeline
from bikg_graph_explainability_public_amd import nn as xnn
from bikg_graph_explainability_public_amd.program import UnsupportedArch, compile_arch

PTR = 256  # a non-NULL "device pointer": never dereferenced by the host queries
ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _model(dims, fc, R, decoder="distmult", act="sigmoid", seed=5, **kw):
    torch.manual_seed(seed)
    enc = xnn.RGCNStack(list(dims), list(fc), R, final_act="identity", **kw)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.3, 0.3)
    return xnn.RelLinkModel(enc, R, decoder=decoder, act=act).eval()


def _graph(n=30, e=140, f=8, R=5, seed=0):
    """Random typed edges, duplicates of one and of two types, node 2 with two type-0 self-loops
    and one type-1 self-loop; relation R - 1 absent."""
    g = np.random.default_rng(seed)
    ei = np.stack([g.integers(0, n, e), g.integers(0, n - 3, e)])
    et = g.integers(0, R - 1, e)
    ei = np.concatenate([ei, ei[:, :8], np.array([[2, 2, 2], [2, 2, 2]])], 1).astype(np.int64)
    et = np.concatenate([et, np.where(np.arange(8) % 2, et[:8], (et[:8] + 1) % (R - 1)),
                         np.array([0, 0, 1])]).astype(np.int64)
    return ei, et, g.standard_normal((n, f)) - 0.5


FORMS = {"plain": {}, "bases": {"num_bases": 3}, "blocks": {"num_blocks": 2}}


def _masks(rows, E, seed, query=None):
    g = np.random.default_rng(seed)
    m = g.random((rows, E)) < g.uniform(0.2, 0.9, (rows, 1))
    m[0], m[1] = True, False
    if query is not None:
        m[2:, query] = False  # the query edge's own column dropped
        m[2, :] = True
        m[2, query] = False
    return m


def _module_on_union(model, x, ei, et, m, u, v, lt):
    """The module's own forward (fp64) on the union graph built here with torch."""
    n = x.shape[0]
    rows, cols = torch.nonzero(torch.as_tensor(m), as_tuple=True)
    uei = torch.as_tensor(ei)[:, cols] + rows * n
    off = torch.arange(m.shape[0]) * n
    with torch.no_grad():
        return model(torch.as_tensor(x).repeat(m.shape[0], 1), uei, None, torch.as_tensor(et)[cols],
                     edge_label_index=torch.stack([off + u, off + v]),
                     edge_label_type=torch.full((m.shape[0],), lt)).reshape(-1).numpy()


# ------------------------------------------------------------------ module vs restatement
@pytest.mark.parametrize("act", ["sigmoid", "identity"])
@pytest.mark.parametrize("decoder", ["distmult", "dot"])
@pytest.mark.parametrize("aggr", ["mean", "add"])
@pytest.mark.parametrize("form", list(FORMS))
def test_module_matches_restatement_fp64(form, aggr, decoder, act):
    ei, et, x = _graph()
    model = _model([8, 6, 4], [4], 5, decoder, act, aggr=aggr, **FORMS[form]).double()
    assert (model.rel_emb is None) == (decoder == "dot")
    if decoder == "distmult":
        assert tuple(model.rel_emb.shape) == (5, 4) and "rel_emb" in model.state_dict()
    with torch.no_grad():  # defaults: every edge with its own type
        got = model(torch.as_tensor(x), torch.as_tensor(ei), None, torch.as_tensor(et))
    assert tuple(got.shape) == (ei.shape[1], 1)
    np.testing.assert_allclose(got.reshape(-1).numpy(), ref.all_edge_outputs(model, x, ei, et),
                               rtol=0, atol=1e-12)
    li = np.array([[3, 2, 7, 0], [4, 2, 1, 29]])  # explicit label index / type (a non-edge too)
    lt = np.array([0, 1, 3, 2])
    with torch.no_grad():
        got = model(torch.as_tensor(x), torch.as_tensor(ei), None, torch.as_tensor(et).int(),
                    edge_label_index=torch.as_tensor(li), edge_label_type=torch.as_tensor(lt))
    np.testing.assert_allclose(got.reshape(-1).numpy(), ref.all_edge_outputs(model, x, ei, et, li, lt),
                               rtol=0, atol=1e-12)
    # masked copies; from row 2 on the query edge's own column is dropped
    q = 20
    u, v, t = int(ei[0, q]), int(ei[1, q]), int(et[q])
    m = _masks(9, ei.shape[1], 7, q)
    want = ref.edge_outputs(model, x, ei, et, m, u, v, t)
    np.testing.assert_allclose(_module_on_union(model, x, ei, et, m, u, v, t), want, rtol=0, atol=1e-12)
    assert np.ptp(want) > 1e-6  # the masks matter


def test_head_and_constructor_checks():
    ei, et, x = _graph()
    model = _model([8, 6], [6, 5, 3], 5).double()  # a two-layer head: rel_emb has its width
    assert tuple(model.rel_emb.shape) == (5, 3)
    with torch.no_grad():
        got = model(torch.as_tensor(x), torch.as_tensor(ei), None, torch.as_tensor(et))
    np.testing.assert_allclose(got.reshape(-1).numpy(), ref.all_edge_outputs(model, x, ei, et),
                               rtol=0, atol=1e-12)
    enc = xnn.RGCNStack([8, 4], [4], 5, final_act="identity")
    with pytest.raises(ValueError):
        xnn.RelLinkModel(enc, 5, decoder="transe")
    with pytest.raises(ValueError):
        xnn.RelLinkModel(enc, 5, act="tanh")
    # LinkModel is untouched: two-argument encoder call, no rel_emb
    lm = xnn.LinkModel(xnn.ConvStack("sage", [8, 4], [4], final_act="identity"))
    assert not hasattr(lm, "rel_emb")


# ------------------------------------------------------------------ lowering
def test_compiled_program_carries_the_decoder():
    model = _model([8, 6, 4], [4], 5, "distmult", "sigmoid", num_bases=3)
    prog = compile_arch(model)
    assert prog.link_act == "sigmoid" and prog.link_rel.dtype == torch.float32
    assert torch.equal(prog.link_rel, model.rel_emb.detach())
    assert all(t.kind in ("rel", "root") for c in prog.convs for t in c.terms) and not prog.head
    assert pipeline.typed_relations(prog) == 5
    prog = compile_arch(_model([8, 6, 4], [4, 3], 5, "dot", "identity"))
    assert prog.link_act == "identity" and prog.link_rel is None and len(prog.head) == 1
    # a double-precision module lowers to fp32
    assert compile_arch(model.double()).link_rel.dtype == torch.float32


def test_lowering_refusals():
    model = _model([8, 6, 4], [4], 5)
    bad = copy.deepcopy(model)
    bad.rel_emb = torch.nn.Parameter(torch.zeros(5, 6))
    with pytest.raises(UnsupportedArch, match="rel_emb"):
        compile_arch(bad)

    class RelLinkModel(torch.nn.Module):  # the class-name rule, with an untyped encoder
        def __init__(self):
            super().__init__()
            self.encoder = xnn.ConvStack("sage", [8, 4], [4], final_act="identity")
            self.act = "sigmoid"
            self.rel_emb = None
    with pytest.raises(UnsupportedArch, match="RGCNConv"):
        compile_arch(RelLinkModel())
    # a node problem on a link model: the ValueError a LinkModel gets
    with pytest.raises(ValueError, match="edge_prediction"):
        pipeline.build_plan(model, torch.zeros(4, 8), torch.zeros((2, 3), dtype=torch.long), [0],
                            None, torch.zeros(3, dtype=torch.long))


# ------------------------------------------------------------------ generic path
@pytest.mark.parametrize("decoder", ["distmult", "dot"])
@pytest.mark.parametrize("form,aggr", [("plain", "mean"), ("bases", "add"), ("blocks", "mean")])
def test_generic_edge_outputs_with_types(form, aggr, decoder):
    ei, et, x = _graph(seed=2)
    x = x.astype(np.float32)
    model = _model([8, 6, 4], [4], 5, decoder, aggr=aggr, **FORMS[form])
    m = _masks(24, ei.shape[1], 5)
    for q in (20, ei.shape[1] - 1):  # a regular edge and a self-loop of node 2
        u, v, t = int(ei[0, q]), int(ei[1, q]), int(et[q])
        want = ref.edge_outputs(copy.deepcopy(model).double(), x, ei, et, m, u, v, t)
        for step in (None, 7):
            got = pipeline.generic_edge_outputs(model, torch.from_numpy(x), torch.from_numpy(ei),
                                                torch.from_numpy(m), u, v, max_rows=step,
                                                edge_type=torch.from_numpy(et), label_type=t)
            np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=2e-6)
    # without the types the call is LinkModel's, as before
    lm = xnn.LinkModel(xnn.ConvStack("sage", [8, 4], [4], final_act="identity")).eval()
    got = pipeline.generic_edge_outputs(lm, torch.from_numpy(x), torch.from_numpy(ei),
                                        torch.from_numpy(m), 3, 4)
    assert tuple(got.shape) == (24,)


# ------------------------------------------------------------------ shared inputs of the GPU suite
@pytest.mark.parametrize("query", ["regular", "loop", "into_hub"])
def test_hub_graph_and_masks_have_their_edge_cases(query):
    """The graph and masks tests/test_gpu_rel_edge.py uses, and (on the same inputs) that at least
    half of the rows' reference outputs differ from the all-on row's."""
    ei, et, info = ref.typed_hub_graph(4)
    E = ei.shape[1]
    assert info["S"] == 120 and 480 <= E <= 540 and not (et == 3).any()
    into0 = ei[1] == 0
    assert into0.sum() >= 300 and set(et[into0].tolist()) == {0, 1, 2}
    for node, deg in zip((10, 11, 12, 13), (1, 3, 4, 5)):
        sel = ei[1] == node
        assert sel.sum() == deg and set(et[sel].tolist()) == {0}
    assert (ei[1] == 14).sum() == 9
    loops7 = et[(ei[0] == 7) & (ei[1] == 7)]
    assert sorted(loops7.tolist()) == [0, 0, 1] and len(info["loops7_t0"]) == 2
    assert set(et[ei[1] == 20].tolist()) == {1}
    pairs = {}
    for (a, b), t in zip(ei.T.tolist(), et.tolist()):
        pairs.setdefault((a, b), []).append(t)
    assert any(len(v) > len(set(v)) for v in pairs.values())   # duplicates of one type
    assert any(len(set(v)) > 1 for v in pairs.values())        # duplicates of two types
    q = info[query]
    m = ref.hub_masks(ei, et, info, q)
    assert m.shape == (70, E) and m[0].all() and not m[1].any()
    assert not m[2, ei[1] == ei[0][q]].any() and m[2, ei[1] != ei[0][q]].all()
    assert m[3, info["loops7_t0"]].sum() == 1 and m[3].sum() == E - 1
    # the GPU suite's own cases on this query: the masks move the fp64 reference
    import test_gpu_rel_edge as gpu_suite
    for form, aggr in gpu_suite.CASES:
        for feat in ("randn", "neg"):
            y = gpu_suite._case(form, aggr, "distmult", "sigmoid", feat, query, fc=gpu_suite.HEAD)["ref"]
            assert np.mean((y > 0.02) & (y < 0.98)) >= 0.5
            assert np.mean(np.abs(y - y[0]) > 1e-9) >= 0.5, (form, aggr, feat)


# ------------------------------------------------------------------ typed edge columns of a plan
@pytest.mark.parametrize("seed", [0, 1])
def test_typed_edge_columns_brute_force(seed):
    """typed_relation_edges' order as edge_cols through the native plan arrays: equal to the numpy
    restatement, and every CSR entry's agg_eid names an edge of that relation, source and target;
    self_eid names the self-loop columns."""
    R, L = 5, 2
    ei, et, _ = _graph(seed=seed)
    S, E = 30, ei.shape[1]
    rels, order = pipeline.typed_relation_edges(torch.as_tensor(ei), torch.as_tensor(et), R,
                                                return_order=True)
    ecols = list(torch.split(order, [e.shape[1] for e in rels]))
    assert sorted(order.tolist()) == list(range(E))
    for r in range(R):
        assert torch.equal(rels[r], torch.as_tensor(ei)[:, ecols[r]])
        assert (et[ecols[r].numpy()] == r).all() and (np.diff(ecols[r].numpy()) > 0).all()
    rel_np = [e.numpy() for e in rels]
    rel_eid = [c.numpy() for c in ecols]
    queries = [2, 5]
    arr = engine.plan_arrays(S, rel_np, queries, L, rel_eid)
    arr_np = engine.plan_arrays_numpy(S, rel_np, queries, L, rel_eid)
    seen_loop = 0
    for li in range(L):
        lay, lay_np = arr["layers"][li], arr_np["layers"][li]
        for k in ("agg_ptr", "agg_src", "agg_f0", "self_mult", "agg_eid", "self_ptr", "self_eid"):
            assert np.array_equal(np.asarray(lay[k]), lay_np[k]), k
        targets, f0 = arr["frontiers"][li + 1], arr["frontiers"][0]
        n_t = targets.size
        ptr_ = np.asarray(lay["agg_ptr"]).reshape(R, n_t + 1)
        sptr = np.asarray(lay["self_ptr"]).reshape(R, n_t + 1)
        for r in range(R):
            for t in range(n_t):
                node = int(targets[t])
                cols = [int(c) for c in lay["agg_eid"][ptr_[r, t]:ptr_[r, t + 1]]]
                want = [e for e in range(E) if et[e] == r and ei[1, e] == node and ei[0, e] != node]
                assert cols == want  # edge order, duplicates as separate entries
                srcs = [int(f0[p]) for p in lay["agg_f0"][ptr_[r, t]:ptr_[r, t + 1]]]
                assert srcs == [int(ei[0, e]) for e in want]
                loops = [int(c) for c in lay["self_eid"][sptr[r, t]:sptr[r, t + 1]]]
                assert loops == [e for e in range(E) if et[e] == r and ei[0, e] == ei[1, e] == node]
                assert len(loops) == int(np.asarray(lay["self_mult"]).reshape(R, n_t)[r, t])
                seen_loop += len(loops)
    assert seen_loop >= 3


# ------------------------------------------------------------------ ABI v27
def make_rel_plan(n_layers=2, n_rel=5, slices=None, coef=False, root=True, f_out=32, n_nodes=300,
                  n_tgt=40, edge_masks=False, n_edges=1500):
    """tests/test_rgcn_cpu.py's synthetic REL descriptor; edge_masks: mask columns = the edges and
    every conv layer carries agg_eid / self_ptr / self_eid."""
    L = (_lib.LayerDesc * n_layers)()
    prev = 0
    for li, ld in enumerate(L):
        ld.n_terms, ld.act, ld.f_in_pad = 1 + int(root), 1, prev
        ld.f_out, ld.f_out_pad = f_out, (f_out + 31) // 32 * 32
        ld.n_tgt, ld.n_edges = n_tgt, n_edges
        for f in ("tgt_prev", "tgt_f0", "agg_ptr", "agg_src", "agg_f0", "self_mult", "bias", "seg_ptr",
                  "seg_rel") + (("agg_eid", "self_ptr", "self_eid") if edge_masks else ()):
            setattr(ld, f, PTR)
        ld.weight = PTR if li else None
        t = ld.terms[0]
        t.kind, t.rel, t.dst_type, t.norm = _lib.TERM["rel"], -1, -1, 0
        t.table = PTR if li == 0 else None
        t.n_slices = n_rel if li == 0 or slices is None else slices
        t.coef = PTR if (coef and li > 0) else None
        if root:
            ld.terms[1].kind, ld.terms[1].rel, ld.terms[1].dst_type = _lib.TERM["root"], -1, -1
            ld.terms[1].table = PTR if li == 0 else None
        prev = ld.f_out_pad
    H = (_lib.HeadDesc * 1)()
    H[0].k_pad, H[0].n_real, H[0].n_pad, H[0].act, H[0].weight, H[0].bias = prev, 1, 32, 2, PTR, PTR
    desc = _lib.ForwardPlanDesc(cols=n_edges if edge_masks else n_nodes, n_rel=n_rel, n0=n_nodes,
                                f0_node=PTR, deg_ptr=PTR, deg_src=PTR, n_deg_edges=n_edges,
                                n_layers=n_layers, layers=L, n_head=1, head=H, out_col=0)
    if edge_masks:
        desc.edge_masks, desc.deg_eid = 1, PTR
        desc.edge_dot, desc.dot_a, desc.dot_b, desc.dot_act, desc.dot_scale = 1, 0, 1, 2, PTR
    desc._keep = (L, H)
    return desc


def make_edge_plan(kinds, n_layers=2, f_out=32, n_nodes=300, n_tgt=2, n_edges=1500):
    """An untyped edge-mask descriptor (GCN / SAGE-mean terms, dot-product decoder, no head)."""
    L = (_lib.LayerDesc * n_layers)()
    prev = 0
    for li, ld in enumerate(L):
        ld.n_terms, ld.act, ld.f_in_pad = len(kinds), 1, prev
        ld.f_out, ld.f_out_pad = f_out, (f_out + 31) // 32 * 32
        ld.n_tgt, ld.n_edges = (n_tgt if li == n_layers - 1 else 40), n_edges
        for f in ("tgt_prev", "tgt_f0", "agg_ptr", "agg_src", "agg_f0", "self_mult", "bias", "agg_eid",
                  "self_ptr", "self_eid"):
            setattr(ld, f, PTR)
        ld.weight = PTR if li else None
        for k, kind in enumerate(kinds):
            ld.terms[k].kind, ld.terms[k].rel, ld.terms[k].dst_type = _lib.TERM[kind], 0, -1
            ld.terms[k].table = PTR if li == 0 else None
        prev = ld.f_out_pad
    H = (_lib.HeadDesc * 1)()
    desc = _lib.ForwardPlanDesc(cols=n_edges, n_rel=1, n0=n_nodes, f0_node=PTR, deg_ptr=PTR,
                                deg_src=PTR, n_deg_edges=n_edges, n_layers=n_layers, layers=L,
                                n_head=0, head=H, out_col=0, edge_masks=1, deg_eid=PTR, edge_dot=1,
                                dot_a=0, dot_b=1, dot_act=2)
    desc._keep = (L, H)
    return desc


def describe(desc, rows=70):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().xpg_forward_describe(ctypes.byref(desc), rows, buf, 256))
    return buf.value.decode()


def workspace(desc, rows):
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_forward_workspace(ctypes.byref(desc), rows, ctypes.byref(n)))
    return n.value


def forward_rc(desc, rows=70):
    rc = _lib.load().xpg_masked_forward(ctypes.byref(desc), None, rows, None, None, 0, None)
    return rc, _lib.load().xpg_last_error().decode()


def test_abi_v27():
    assert _lib.ABI_VERSION == 28 and _lib.load().xpg_abi_version() == 28
    assert _lib.ForwardPlanDesc._fields_[-1][0] == "dot_scale"
    assert _lib.ForwardPlanDesc.dot_scale.offset == _lib.ForwardPlanDesc.dot_act.offset + 8 \
        or _lib.ForwardPlanDesc.dot_scale.offset == _lib.ForwardPlanDesc.dot_act.offset + 4
    assert len(engine.wide_variants()) == 27


@pytest.mark.parametrize("kw", [{}, {"n_rel": 100, "slices": 32, "coef": True}, {"root": False},
                                {"n_layers": 1}, {"n_layers": 3, "n_rel": 32}])
def test_rel_edge_mask_descriptors_pass_the_host_checks(kw):
    desc = make_rel_plan(edge_masks=True, **kw)
    assert describe(desc) == "unfused"
    rc, msg = forward_rc(desc)
    assert rc == 1 and "workspace too small" in msg
    # no degree region: the node-mask plan's workspace, whatever the relation count
    assert workspace(desc, 70) == workspace(make_rel_plan(**kw), 70)
    if "coef" in kw:
        many = make_rel_plan(edge_masks=True, **dict(kw, n_rel=400))
        assert workspace(many, 70) == workspace(desc, 70)


@pytest.mark.parametrize("field", ["agg_eid", "self_ptr", "self_eid"])
@pytest.mark.parametrize("layer", [0, 1])
def test_rel_edge_mask_descriptor_without_a_column_array_is_refused(field, layer):
    desc = make_rel_plan(edge_masks=True)
    setattr(desc._keep[0][layer], field, None)
    rc, msg = forward_rc(desc)  # before the workspace check, i.e. before any launch
    assert rc == 1 and "REL terms do not take edge-mask plans" in msg and field in msg
    rc = _lib.load().xpg_masked_forward(ctypes.byref(desc), None, 70, None, None, 1 << 40, None)
    assert rc == 1 and b"REL terms do not take edge-mask plans" in _lib.load().xpg_last_error()


@pytest.mark.parametrize("path", ["wide", "rows", "fused"])
def test_forced_paths_decline_rel_edge_plans(path, monkeypatch):
    desc = make_rel_plan(edge_masks=True, n_nodes=40, n_tgt=2)
    monkeypatch.setenv("XPG_FORWARD", path)
    assert describe(desc) == "unfused"
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="forced XPG_FORWARD path does not take this plan"):
        describe(desc)


# bytes for 70 rows, recorded with these descriptors from the library of the commit before v27
# (ABI 26: the same fields without dot_scale), which this library must still return
V26_WORKSPACES = {
    "rel": 3584256, "rel-bases": 13261056, "rel-noroot-1": 1075456, "rel-32x3": 39424256,
    "edge-gcn": 478720, "edge-sage": 120320,
}


def test_workspace_sizes_equal_the_v26_library():
    got = {
        "rel": workspace(make_rel_plan(), 70),
        "rel-bases": workspace(make_rel_plan(n_rel=100, slices=32, coef=True), 70),
        "rel-noroot-1": workspace(make_rel_plan(n_layers=1, root=False), 70),
        "rel-32x3": workspace(make_rel_plan(n_layers=3, n_rel=32, f_out=70), 70),
        "edge-gcn": workspace(make_edge_plan(("gcn",)), 70),
        "edge-sage": workspace(make_edge_plan(("mean", "root"), n_layers=1, f_out=50), 70),
    }
    assert got == V26_WORKSPACES


# ------------------------------------------------------------------ refusals that stay
@pytest.mark.parametrize("kinds", [("sum", "root"), ("max", "root")])
def test_edge_mask_plans_still_refuse_sum_and_max(kinds):
    desc = make_edge_plan(kinds)
    rc = _lib.load().xpg_masked_forward(ctypes.byref(desc), None, 70, None, None, workspace(desc, 70),
                                        None)
    assert rc == 1 and b"SUM / MAX terms do not take edge-mask plans" in _lib.load().xpg_last_error()


def test_build_edge_plan_falls_back_without_usable_types():
    """A missing edge_type, a type outside [0, R) and convs that disagree on num_relations: the
    usual warning and None (the generic path), before any device work."""
    model = _model([8, 6, 4], [4], 5)
    ei, et, x = _graph()
    x, ei_t, et_t = torch.from_numpy(x).float(), torch.from_numpy(ei), torch.from_numpy(et)
    with pytest.warns(UserWarning, match="needs edge_types"):
        assert pipeline.build_edge_plan(model, x, ei_t, 3, 4) is None
    bad = et_t.clone()
    bad[3] = 5
    with pytest.warns(UserWarning, match="outside"):
        assert pipeline.build_edge_plan(model, x, ei_t, 3, 4, edge_type=bad, label_type=0) is None
    two = copy.deepcopy(model)
    two.encoder.conv[2] = xnn.RGCNConv(6, 4, 7)
    with pytest.warns(UserWarning, match="different num_relations"):
        assert pipeline.build_edge_plan(two, x, ei_t, 3, 4, edge_type=et_t, label_type=0) is None
    with pytest.warns(UserWarning, match="relation embedding"):
        assert pipeline.build_edge_plan(model, x, ei_t, 3, 4, edge_type=et_t, label_type=9) is None
