"""GPU parity of weighted graphs (edge_weight for GCNConv / GraphConv; k_degree_w + k_agg_w,
xpgnn.h xpg_edge_weights) against the fp64 restatement of tests/edge_weight_ref.py on the hub
graph of tests/test_gpu_aggr.py (S = 400, node 0 with 300 extra in-edges, node 7 with two
self-loops of unequal weight).  Bars, the project's existing ones: sigmoid outputs atol 1e-5
against fp64; identity heads max(1e-5, 4 x e32), e32 = the nn.py module's own float32 CPU error on
the same inputs; DataFrames atol 1e-4.  Every test first asserts the path it measures
(ForwardPlan.describe contains `weights=k_degree_w+k_agg_w`)."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import edge_weight_ref as ewr
import gatv2_ref
import pool_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
QUERIES = ewr.QUERIES
ROWS = 64
TAG = "weights=k_degree_w+k_agg_w"
ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS", "XPG_AGG_GENERIC")
KINDS = ["gcn", "graphconv", "graphconv-mean", "graphconv-max"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _pack(m):
    from bikg_graph_explainability_public_amd import engine
    return engine.pack_masks(torch.as_tensor(m, device=DEV))


def _plan(arch, x, ei, queries, w=None):
    from bikg_graph_explainability_public_amd import pipeline
    kw = {} if w is None else {"edge_weight": torch.as_tensor(w, dtype=torch.float32, device=DEV)}
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a generic-path warning fails the test
        plan = pipeline.build_plan(copy.deepcopy(arch).to(DEV), x.to(DEV), torch.as_tensor(ei, device=DEV),
                                   queries, **kw)
    assert plan is not None
    if w is not None:
        assert TAG in plan.describe(ROWS)
    return plan


def _check(got, ref, atol=1e-5):
    got = got.cpu().numpy().reshape(ref.shape)
    err = float(np.abs(got - ref).max())
    print("max |engine - fp64| =", err)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    return err


@functools.lru_cache(maxsize=None)
def _case(kind, dims=(16, 8, 8), final_act="sigmoid"):
    """ConvStack(kind, dims, [dims[-1], 1]) on the hub graph with weights uniform(0.25, 2) (node
    7's loops 0.5 and 1.75; GraphConv: a quarter of the edges negated), 64 rows: all-off, all-on,
    one row per query with the query masked.  The conv weight scale is fitted on the sigmoid
    model's fp64 reference; `final_act="identity"` then swaps the last activation."""
    S = 400
    x = torch.randn((S, dims[0]), generator=torch.Generator().manual_seed(21))
    ei = pool_ref.hub_graph(S)
    w = ewr.hub_weights(ei, signed=kind != "gcn")
    masks = gatv2_ref.row_masks(ROWS, S, 3, QUERIES)
    arch = ewr.model(kind, dims, (dims[-1], 1))
    ewr.fit_scale(arch, x.numpy(), ei, w, masks, QUERIES)
    if final_act != "sigmoid":
        arch.fc[-1] = torch.nn.Identity()
    ref = ewr.union_outputs(arch, x.numpy(), ei, w, masks)[:, QUERIES]
    ref1 = ewr.union_outputs(arch, x.numpy(), ei, None, masks)[:, QUERIES]
    return {"S": S, "x": x, "ei": ei, "w": w, "arch": arch, "masks": masks, "ref": ref, "ref_unweighted": ref1}


# ------------------------------------------------------------------ plans against fp64
@pytest.mark.parametrize("dims", [(16, 8, 8), (40, 70, 8), (16, 256, 8)])
@pytest.mark.parametrize("kind", KINDS)
def test_weighted_plans_vs_fp64(kind, dims):
    """Two conv layers at widths 32 / 32 (LPS 8), 96 / 32 with a 40-wide input (LPS 24, and 16 for
    the raw first layer of max) and 256 / 32 (LPS 64).  Measured max |engine - fp64| on an
    MI355X: 5.1e-8 ... 5.2e-7 over the 12 cases."""
    c = _case(kind, dims)
    ref = c["ref"]
    assert np.mean((ref > 0.02) & (ref < 0.98)) >= 0.5
    assert np.ptp(ref) > 1e-3 and np.ptp(ref[:, 0]) > 1e-3  # a kernel ignoring the masks fails
    assert np.abs(ref - c["ref_unweighted"]).max() > 1e-3  # and one ignoring the weights
    plan = _plan(c["arch"], c["x"], c["ei"], QUERIES, c["w"])
    assert plan.describe(ROWS).startswith("unfused " + TAG)
    kinds = {k for low in plan.lowering for k, _, _ in low}
    assert kinds == {"gcn"} if kind == "gcn" else "root" in kinds
    _check(plan.forward(_pack(c["masks"])), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_identity_head_vs_fp64(kind):
    """No sigmoid to hide errors: bar max(1e-5, 4 x e32), e32 = the largest difference of the same
    nn.py module in float32 on CPU torch from fp64 on the same weighted union graph."""
    c = _case(kind, (16, 8, 8), "identity")
    out32 = ewr.module_outputs(c["arch"], c["x"].numpy(), c["ei"], c["w"], c["masks"])[:, QUERIES]
    e32 = float(np.abs(out32 - c["ref"]).max())
    bar = max(1e-5, 4 * e32)
    print(f"{kind}: e32 = {e32:.3g}, bar = {bar:.3g}, |ref| max = {np.abs(c['ref']).max():.3g}")
    plan = _plan(c["arch"], c["x"], c["ei"], QUERIES, c["w"])
    _check(plan.forward(_pack(c["masks"])), c["ref"], bar)


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_weights_equal_the_unweighted_plan(kind):
    """GraphConv add / mean / max: bitwise (w = 1 multiplies exactly and the adds keep k_agg's
    order).  GCN: within 1e-6 (the weighted degree is the same float, the coefficient has one
    more factor)."""
    c = _case(kind)
    bits = _pack(c["masks"])
    y0 = _plan(c["arch"], c["x"], c["ei"], QUERIES).forward(bits)
    y1 = _plan(c["arch"], c["x"], c["ei"], QUERIES, np.ones(c["ei"].shape[1])).forward(bits)
    d = float((y0 - y1).abs().max())
    print(f"{kind}: max |weighted(1) - unweighted| = {d:.3g}")
    if kind == "gcn":
        assert d <= 1e-6  # observed on an MI355X: 0 (bitwise equal, like the GraphConv kinds)
    else:
        assert torch.equal(y0, y1)


# ------------------------------------------------------------------ zero weights
@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights(kind):
    """Node 5: every in-edge and its self-loop have weight 0 (GCN: lw = 0, deg = 0, dis = 0, no
    NaN; GraphConv: an all-zero in-neighbourhood).  Node 9: in-weights 0, no loop."""
    S = 40
    g = np.random.default_rng(11)
    ei = g.integers(0, S, (2, 260))
    ei = ei[:, ei[0] != ei[1]]
    ei = np.concatenate([ei, np.array([[5, 3], [5, 3]])], 1).astype(np.int64)
    w = g.uniform(0.25, 2.0, ei.shape[1]).astype(np.float32).astype(np.float64)
    w[(ei[1] == 5) | (ei[1] == 9)] = 0.0
    x = torch.randn((S, 16), generator=torch.Generator().manual_seed(2))
    qs = [5, 9, 3]
    masks = gatv2_ref.row_masks(ROWS, S, 8, qs)
    arch = ewr.model(kind, (16, 8, 8), (8, 1), final_act="identity")
    ref = ewr.union_outputs(arch, x.numpy(), ei, w, masks)[:, qs]
    assert np.isfinite(ref).all() and np.ptp(ref) > 1e-3
    plan = _plan(arch, x, ei, qs, w)
    _check(plan.forward(_pack(masks)), ref)


# ------------------------------------------------------------------ workspace, chunks, row counts
@pytest.mark.parametrize("kind", ["gcn", "graphconv-max"])
def test_outputs_do_not_depend_on_workspace_chunks_or_row_count(kind):
    c = _case(kind)
    plan = _plan(c["arch"], c["x"], c["ei"], QUERIES, c["w"])
    bits = _pack(c["masks"])
    nb = plan.workspace_bytes(ROWS)
    outs = []
    for fill in (0x00, 0xFF):  # 0xFF: every float of the workspace a NaN
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        out = torch.empty((ROWS, len(QUERIES)), dtype=torch.float32, device=DEV)
        plan.forward(bits, out=out, workspace=ws)
        outs.append(out)
    _check(outs[0], c["ref"])
    assert torch.equal(outs[0], outs[1])
    y = plan.forward(bits)
    assert torch.equal(y, outs[0])
    assert torch.equal(torch.cat([plan.forward(bits[:32]), plan.forward(bits[32:])]), y)
    for rows in (1, 33):
        assert torch.equal(plan.forward(bits[:rows]), y[:rows])
    small = plan.workspace_bytes(16)
    assert small < nb
    plan._ws = None
    assert torch.equal(plan.forward(bits, max_ws_bytes=small), y)


# ------------------------------------------------------------------ composition
def test_block_stack_with_layer_norm_and_residual():
    """BlockStack("gcn", norm="layer", residual=True): k_post follows the weighted layers."""
    from bikg_graph_explainability_public_amd.nn import BlockStack
    import block_ref
    c = _case("gcn")
    torch.manual_seed(5)
    arch = block_ref.randomise_norms(BlockStack("gcn", [16, 8, 8], [8, 1], norm="layer", residual=True), 6).eval()
    ref = ewr.union_outputs(arch, c["x"].numpy(), c["ei"], c["w"], c["masks"])[:, QUERIES]
    assert np.ptp(ref) > 1e-3
    assert np.abs(ref - ewr.union_outputs(arch, c["x"].numpy(), c["ei"], None, c["masks"])[:, QUERIES]).max() > 1e-3
    plan = _plan(arch, c["x"], c["ei"], QUERIES, c["w"])
    assert plan.describe(ROWS) == "unfused " + TAG + " post1=k_post<layer,0> post2=k_post<layer,1>"
    _check(plan.forward(_pack(c["masks"])), ref)


def test_pooled_graphconv():
    """PooledModel(ConvStack("graphconv"), "add"): the readout follows the weighted layers."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel
    c = _case("graphconv")
    torch.manual_seed(5)
    arch = PooledModel(ConvStack("graphconv", [16, 8, 8], [8]), "add", [8, 1]).eval()
    with torch.no_grad():
        arch.fc[0].weight.mul_(pool_ref.HEAD_SCALE["sum"])
    ref = ewr.fit_scale(arch, c["x"].numpy(), c["ei"], c["w"], c["masks"])
    assert ref.shape == (ROWS,) and np.ptp(ref) > 1e-3
    assert np.abs(ref - ewr.union_outputs(arch, c["x"].numpy(), c["ei"], None, c["masks"])).max() > 1e-3
    plan = _plan(arch, c["x"], c["ei"], [0], c["w"])
    assert plan.pool == "sum"
    _check(plan.forward(_pack(c["masks"]))[:, 0], ref)


# ------------------------------------------------------------------ forced paths
def test_forced_rows_path_is_refused_under_strict(monkeypatch):
    c = _case("gcn")
    plan = _plan(c["arch"], c["x"], c["ei"], QUERIES, c["w"])
    y = plan.forward(_pack(c["masks"]))
    monkeypatch.setenv("XPG_FORWARD", "rows")
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="forced XPG_FORWARD path"):
        plan.describe(ROWS)
    with pytest.raises(RuntimeError, match="forced XPG_FORWARD path"):
        plan.forward(_pack(c["masks"]))
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    assert TAG in plan.describe(ROWS)  # not strict: the multi-kernel path, same result
    assert torch.equal(plan.forward(_pack(c["masks"])), y)


# ------------------------------------------------------------------ Explainer.run
def _explainer(kind, problem, S, weighted=True, params=None):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel
    g = np.random.default_rng(1)
    ei = g.integers(0, S, (2, 4 * S))
    q = int(ei[1, 0])  # the query: a node with an in-edge, given two self-loops of unequal weight
    ei = np.concatenate([ei, np.array([[q, q], [q, q]])], 1)
    w = g.uniform(0.25, 2.0, ei.shape[1])
    w[-2:] = [0.5, 1.75]
    feat = torch.randn((S, 12), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    if kind == "pooled-graphconv":
        arch = PooledModel(ConvStack("graphconv", [12, 8, 8], [8]), "add", [8, 1]).eval()
        w = w * np.where(g.random(w.size) < 0.25, -1.0, 1.0)
        ewr.scale_convs(arch, 0.25)
    else:
        arch = ConvStack("gcn", [12, 8, 8], [8, 1]).eval()
    base = {"seed": 1, "interpret_samples": 10, "epochs": 8, "optimizer": "adam", "lr": 0.01,
            "lr_patience": 10, "l1_lambda": 1e-4, "verify_arch": True}
    wt = torch.as_tensor(w, dtype=torch.float32) if weighted else None
    exp = Explainer(feat, torch.as_tensor(ei, dtype=torch.long), arch, dict(base, **(params or {})),
                    [str(i) for i in range(S)], None, None, None, problem=problem, edge_weight=wt)
    return exp, str(q)


@pytest.mark.parametrize("kind,problem,S,sampler", [
    ("gcn", "node_prediction", 60, "compat"),
    ("gcn", "node_prediction", 60, "device"),
    ("pooled-graphconv", "graph_prediction", 30, "compat"),
])
def test_explainer_run_matches_the_generic_path(kind, problem, S, sampler, monkeypatch):
    """Explainer.run(edge_weight=...), times=2, verify_arch on: it runs on the engine with the
    arch check `verified`, agrees with a run whose forward is pipeline.generic_outputs (the user's
    module on the weighted union graph; y within 1e-5, DataFrames within 1e-4) and differs from the
    unweighted run."""
    from bikg_graph_explainability_public_amd import pipeline
    params = {"mask_sampler": sampler}
    exp, q = _explainer(kind, problem, S, params=params)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df, _ = exp.run(q, 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified"
    assert TAG in lr["plan"].describe(16)
    y = torch.stack([lr["repeats"][i]["y"].reshape(-1) for i in range(2)])
    assert float(y.std()) > 1e-4
    df0, _ = _explainer(kind, problem, S, weighted=False, params=params)[0].run(q, 2)
    assert np.abs(df.loc[df0.index].values - df0.values).max() > 1e-4
    exp2, _ = _explainer(kind, problem, S, params=params)
    monkeypatch.setattr(pipeline, "build_plan", lambda *a, **k: None)
    df2, _ = exp2.run(q, 2)
    assert exp2.last_run["engine"] is False
    y2 = torch.stack([exp2.last_run["repeats"][i]["y"].reshape(-1) for i in range(2)])
    torch.testing.assert_close(y, y2, rtol=0, atol=1e-5)
    np.testing.assert_allclose(df.loc[df2.index].values, df2.values, rtol=0, atol=1e-4)


def test_an_in_place_weight_edit_invalidates_the_cached_query():
    exp, q = _explainer("gcn", "node_prediction", 60)
    df_a, _ = exp.run(q, 1)
    df_b, _ = exp.run(q, 1)
    assert exp.last_run["query_cache"] == "hit"
    np.testing.assert_array_equal(df_a.loc[df_b.index].values, df_b.values)
    with torch.no_grad():
        exp.edge_weight.mul_(0.25)
        exp.edge_weight[::3] = 2.0
    df_c, _ = exp.run(q, 1)
    assert exp.last_run["query_cache"] == "miss" and exp.last_run["engine"] is True
    fresh, _ = _explainer("gcn", "node_prediction", 60)
    with torch.no_grad():
        fresh.edge_weight.copy_(exp.edge_weight)
    df_d, _ = fresh.run(q, 1)
    np.testing.assert_array_equal(df_c.loc[df_d.index].values, df_d.values)
    assert np.abs(df_c.loc[df_a.index].values - df_a.values).max() > 1e-4
