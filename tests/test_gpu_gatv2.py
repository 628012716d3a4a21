"""GPU parity of the opt-in GATv2Conv (dynamic attention) engine path: ForwardPlan terms of kind
"att2" (k_agg_att2 in csrc/xpgnn.hip, k_dense for the deeper layers' transforms) against the fp64
per-target restatement of tests/gatv2_ref.py.  Bars: forward outputs atol 1e-5 against fp64 (the
bar of test_gpu_attention.py / test_gpu_parity.py); with an identity final activation max(1e-5,
4 x e32), e32 = the error of the nn.py module in float32 on CPU torch against fp64; DataFrames
atol 1e-4.  XPG_FORWARD is unset unless a test says otherwise."""
import copy
import warnings

import numpy as np
import pytest
import torch

import gatv2_ref
import oracle
import pool_ref
from gatv2_ref import QUERIES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S = 400


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("XPG_FORWARD", raising=False)
    monkeypatch.delenv("XPG_FORWARD_STRICT", raising=False)


def _pack(m):
    from bikg_graph_explainability_public_amd import engine
    return engine.pack_masks(torch.as_tensor(m, device=DEV))


def _plan(arch, x, ei, queries=QUERIES, kinds=None, **geo):
    from bikg_graph_explainability_public_amd import pipeline
    eit = torch.as_tensor(ei, device=DEV)
    if geo:
        plan = pipeline.build_plan(copy.deepcopy(arch).to(DEV), x.to(DEV), eit, queries, None,
                                   torch.as_tensor(geo["et"], device=DEV), None, geo["rels"], None,
                                   attention=True)
    else:
        plan = pipeline.build_plan(copy.deepcopy(arch).to(DEV), x.to(DEV), eit, queries, attention=True)
    assert plan is not None
    got = [sorted({k for k, _, _ in low}) for low in plan.lowering]
    assert got == (kinds or [["att2"]] * len(plan.lowering)), got
    assert plan.describe(64) == "unfused"
    return plan


def _check(got, ref, atol=1e-5):
    got = got.cpu().numpy()
    print("max |engine - fp64| =", float(np.abs(got - ref).max()), "bar", atol)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)


def _biases(arch, seed):
    """GATv2Conv initialises lin_l.bias / lin_r.bias / bias to zero: give them values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in arch.modules():
            if type(m).__name__ == "GATv2Conv":
                for b in (m.lin_l.bias, m.lin_r.bias, m.bias):
                    if b is not None:
                        b.copy_(torch.rand(b.shape, generator=g) - 0.5)
    return arch


_MASKS = gatv2_ref.row_masks(64, S, 3, QUERIES)


def _case(arch, rel_edges=None):
    x, ei = gatv2_ref.features(S), gatv2_ref.hub_graph(S)
    ref = gatv2_ref.union_outputs(arch, x.numpy(), rel_edges(ei) if rel_edges else [ei], _MASKS)[:, QUERIES]
    return x, ei, ref


# ------------------------------------------------------------------ the hub case
@pytest.mark.parametrize("att_scale", [1.0, 16.0])
@pytest.mark.parametrize("self_loops", [False, True])
def test_hub_vs_fp64_union_graph(self_loops, att_scale):
    """Two GATv2 layers (heads [2, 1], C = 8) on the hub graph: duplicate edges, explicit
    self-loops (ordinary edges without add_self_loops, replaced by one unconditional loop with it),
    a 300-in-edge hub, all-off / all-on rows and rows with the query itself masked; att x 16 spreads
    the logits (softmax stability).  tests/test_gatv2_cpu.py shows from the reference alone that
    these outputs move with the masks and with the logits."""
    c = gatv2_ref.hub_case(self_loops, att_scale)
    conv = c["arch"].conv[0]
    p = gatv2_ref.conv_params(conv)
    h = c["x"].double().numpy()
    xl = (h @ p["Wl"].T + p["bl"]).reshape(S, 2, 8)
    xr = (h @ p["Wr"].T + p["br"]).reshape(S, 2, 8)
    s = xl[c["ei"][0]] + xr[c["ei"][1]]
    z = (p["att"] * np.where(s > 0, s, 0.2 * s)).sum(-1)
    print("layer-1 logit span =", float(z.max() - z.min()))
    assert att_scale == 1.0 or z.max() - z.min() > 89.0  # past ln(FLT_MAX) without the max subtraction
    plan = _plan(c["arch"], c["x"], c["ei"])
    _check(plan.forward(_pack(c["masks"])), c["ref"])


# ------------------------------------------------------------------ heads x channels
@pytest.mark.parametrize("H,C", [(1, 1), (4, 1), (2, 3), (3, 5), (1, 8), (2, 16), (4, 16), (8, 32),
                                 (1, 256), (3, 40)])
def test_head_and_channel_matrix(H, C):
    """Every shape as layer 1 and as a deeper layer: the aligned kernel (head_ch / 4 a power of
    two: 8, 16, 32, 256) and the general one (heads inside a chunk: 1; chunks straddling heads: 3,
    5; head_ch / 4 = 10), lane groups of 8 (width 32), 16 (64), 32 (128) and 64 (256, the limit).
    Width 96 (24 chunks on a 32-lane group) is the `w96` case of test_module_options."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(100 * H + C)
    arch = _biases(ConvStack("gatv2", [16, C, C], [H * C, 1], heads=[H, H], add_self_loops=(H + C) % 2 == 0)
                   .eval(), H + C)
    x, ei, ref = _case(arch)
    print("reference output range", float(ref.min()), float(ref.max()))
    _check(_plan(arch, x, ei).forward(_pack(_MASKS)), ref)


def _swap(arch, i, conv):
    arch.conv[i] = conv
    return arch


@pytest.mark.parametrize("name", ["shared", "separate", "no_bias", "slope0", "slope1", "mean1", "three", "w96"])
def test_module_options(name):
    """share_weights both ways, bias=False, negative slopes 0 and 1, concat=False with one head, a
    three-conv-layer stack, and a 96-wide layer (24 chunks in a 32-lane group) at both depths."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, GATv2Conv
    torch.manual_seed(31)
    if name in ("shared", "separate"):
        arch = ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1], share_weights=name == "shared",
                         add_self_loops=name == "shared")
    elif name == "no_bias":
        arch = ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1])
        _swap(arch, 0, GATv2Conv(16, 8, heads=2, bias=False))
        _swap(arch, 2, GATv2Conv(16, 8, heads=1, bias=False, add_self_loops=False))
    elif name in ("slope0", "slope1"):
        arch = ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1], add_self_loops=False)
        arch.conv[0].negative_slope = arch.conv[2].negative_slope = float(name[-1])
    elif name == "mean1":
        arch = ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[1, 1])
        _swap(arch, 0, GATv2Conv(16, 8, heads=1, concat=False))
        _swap(arch, 2, GATv2Conv(8, 8, heads=1, concat=False, add_self_loops=False))
    elif name == "three":
        arch = ConvStack("gatv2", [16, 8, 6, 8], [8, 1], heads=[2, 3, 1])
    else:
        arch = ConvStack("gatv2", [16, 32, 48], [96, 1], heads=[3, 2], add_self_loops=False)
    arch = _biases(arch.eval(), 7)
    x, ei, ref = _case(arch)
    plan = _plan(arch, x, ei)
    if name == "shared":
        assert all(t.weight_r is None for c in plan.program.convs for t in c.terms)
    _check(plan.forward(_pack(_MASKS)), ref)


def test_identity_final_activation():
    """No sigmoid to compress the error: bar max(1e-5, 4 x e32), e32 = the float32 CPU module on
    the union graph against fp64."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(17)
    arch = _biases(ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1], final_act="identity").eval(), 3)
    x, ei, ref = _case(arch)
    keep, tiled = oracle.build_edge_mask(_MASKS, ei)
    with torch.no_grad():
        y32 = arch(x.repeat(_MASKS.shape[0], 1), torch.as_tensor(tiled[:, keep]))
    e32 = float(np.abs(y32[:, 0].reshape(_MASKS.shape).double().numpy()[:, QUERIES] - ref).max())
    got = _plan(arch, x, ei).forward(_pack(_MASKS))
    print("e32 =", e32, "output range", float(ref.min()), float(ref.max()))
    assert float(ref.max() - ref.min()) > 0.05
    _check(got, ref, max(1e-5, 4 * e32))


# ------------------------------------------------------------------ edge-set corners
@pytest.mark.parametrize("self_loops", [False, True])
def test_edge_set_corners(self_loops):
    """Rows built for one corner each, queries 0 (the hub; it has a self-loop edge) and 5 (none):
    0 all-off; 1 only the queries kept (every source masked: without a loop the conv gives
    act(bias), with add_self_loops the one loop); 2 the queries and exactly one in-neighbour of
    each; 3 everything but the queries (a masked target: only an added loop survives); 4 all-on
    (the hub with all 300 extra in-edges)."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(9)
    arch = _biases(ConvStack("gatv2", [16, 8, 8], [8, 1], heads=[2, 1], add_self_loops=self_loops).eval(), 5)
    x, ei = gatv2_ref.features(S), gatv2_ref.hub_graph(S)
    qs = [0, 5]
    assert (ei[0] == ei[1])[ei[1] == 0].any() and not (ei[0] == ei[1])[ei[1] == 5].any()
    m = np.zeros((5, S), dtype=bool)
    m[1, qs] = True
    m[2, qs] = True
    for q in qs:
        m[2, ei[0][(ei[1] == q) & (ei[0] != q) & ~np.isin(ei[0], qs)][0]] = True
    m[3] = True
    m[3, qs] = False
    m[4] = True
    assert ((ei[1] == 0) & (ei[0] != 0)).sum() >= 300
    ref = gatv2_ref.union_outputs(arch, x.numpy(), [ei], m)[:, qs]
    if not self_loops:  # query 5, alone: both layers give act(bias), as with every node masked
        assert ref[1, 1] == ref[0, 1] and ref[1, 0] != ref[0, 0]
    # the hub's corners differ in the reference, but for those that leave it the same edge set (a
    # masked target, row 3, has row 0's: nothing, or the one added loop)
    assert len({float(v) for v in ref[:, 0]}) == 4 and ref[3, 0] == ref[0, 0]
    _check(_plan(arch, x, ei, qs).forward(_pack(m)), ref)


# ------------------------------------------------------------------ relations, other kinds, readout
def test_single_type_hetero_two_relations():
    from bikg_graph_explainability_public_amd.nn import ConvStack
    rels = [("n", "a", "n"), ("n", "b", "n")]
    torch.manual_seed(4)
    arch = _biases(ConvStack("gatv2", [16, 8, 8], [8, 1], hetero_rels=rels, heads=[2, 1]).eval(), 2)
    et = (np.arange(gatv2_ref.hub_graph(S).shape[1]) % 3 == 0).astype(np.int64)
    x, ei, ref = _case(arch, lambda ei: [ei[:, et == 0], ei[:, et == 1]])
    plan = _plan(arch, x, ei, et=et, rels=rels)
    assert [(k, r) for k, r, _ in plan.lowering[1]] == [("att2", 0), ("att2", 1)]
    _check(plan.forward(_pack(_MASKS)), ref)


def test_gcn_then_gatv2():
    """Degrees are needed by layer 1 only; the GATv2 layer reads the GCN layer's rows."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, GATv2Conv
    torch.manual_seed(6)
    arch = ConvStack("gcn", [16, 8, 8], [8, 1])
    arch = _biases(_swap(arch, 2, GATv2Conv(8, 4, heads=2, add_self_loops=False)).eval(), 1)
    x, ei, ref = _case(arch)
    _check(_plan(arch, x, ei, kinds=[["gcn"], ["att2"]]).forward(_pack(_MASKS)), ref)


@pytest.mark.parametrize("pool", ["mean", "add", "max"])
def test_pooled_model(pool):
    """The readout after two GATv2 layers, identity head (a sum over 400 nodes would sit on a
    sigmoid's tail): bar max(1e-5, 4 x e32), e32 = the float32 CPU module against fp64."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel
    torch.manual_seed(8)
    enc = ConvStack("gatv2", [16, 8, 8], [8], heads=[2, 1])
    arch = _biases(PooledModel(enc, pool, [8, 1], final_act="identity").eval(), 4)
    x, ei = gatv2_ref.features(S), gatv2_ref.hub_graph(S)
    ref = gatv2_ref.pooled_outputs(arch, x.numpy(), [ei], _MASKS)
    B = _MASKS.shape[0]
    keep, tiled = oracle.build_edge_mask(_MASKS, ei)
    with torch.no_grad():
        y32 = arch(x.repeat(B, 1), torch.as_tensor(tiled[:, keep]), torch.arange(B).repeat_interleave(S))
    e32 = float(np.abs(y32[:, 0].double().numpy() - ref).max())
    print("e32 =", e32, "reference output range", float(ref.min()), float(ref.max()))
    assert np.mean(np.abs(ref - ref[1]) > 1e-3) >= 0.5
    plan = _plan(arch, x, ei, [0])
    assert plan.pool == pool_ref.POOLS[pool] and plan.n_out == 1
    _check(plan.forward(_pack(_MASKS))[:, 0], ref, max(1e-5, 4 * e32))


# ------------------------------------------------------------------ bitwise properties
def _ws_fill(ws, fill):
    if fill == "zero":
        ws.zero_()
    elif fill == "ff":
        ws.fill_(0xFF)
    else:
        ws.random_(0, 256, generator=torch.Generator(device=DEV).manual_seed(5))


@pytest.mark.parametrize("kind", ["aligned", "general"])
def test_outputs_independent_of_workspace_rows_and_chunks(kind):
    """Bitwise identical outputs over caller workspaces pre-filled with zero bytes, 0xFF bytes
    (NaNs) and random bytes; forward(bits[:35]) || forward(bits[35:]) == forward(bits); a
    max_ws_bytes that forces 16-row chunks gives the same bits; two calls are equal."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    if kind == "aligned":
        arch = gatv2_ref.hub_case(True)["arch"]
    else:
        torch.manual_seed(2)
        arch = ConvStack("gatv2", [16, 5, 6], [12, 1], heads=[3, 2], add_self_loops=False).eval()
    x, ei = gatv2_ref.features(S), gatv2_ref.hub_graph(S)
    plan = _plan(arch, x, ei)
    bits = _pack(gatv2_ref.row_masks(70, S, 6, QUERIES))
    nb = plan.workspace_bytes(70)
    outs = []
    for fill in ("zero", "ff", "rand"):
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _ws_fill(ws, fill)
        out = torch.empty((70, plan.n_out), dtype=torch.float32, device=DEV)
        plan.forward(bits, out=out, workspace=ws)
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].std()) > 1e-4
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    y = plan.forward(bits)
    assert torch.equal(y, outs[0]) and torch.equal(plan.forward(bits), y)
    assert torch.equal(torch.cat([plan.forward(bits[:35]), plan.forward(bits[35:])]), y)
    small = plan.workspace_bytes(16)
    assert small < plan.workspace_bytes(70)
    plan._ws = None
    assert torch.equal(plan.forward(bits, max_ws_bytes=small), y)
    assert plan._ws.numel() <= small  # several chunks of at most 16 rows


def test_forced_paths_are_refused(monkeypatch):
    c = gatv2_ref.hub_case(False)
    plan = _plan(c["arch"], c["x"], c["ei"])
    bits = _pack(c["masks"])
    y = plan.forward(bits)
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    assert torch.equal(plan.forward(bits), y)
    for path in ("rows", "fused", "wide"):
        monkeypatch.setenv("XPG_FORWARD", path)
        out = torch.full_like(y, -7.0)
        with pytest.raises(RuntimeError, match="does not take this plan"):
            plan.forward(bits, out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())  # no output produced


# ------------------------------------------------------------------ Explainer.run
def _explainer(params=None, pathways=False):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack
    n = 60
    g = np.random.default_rng(1)
    ei = torch.as_tensor(g.integers(0, n, (2, 240)), dtype=torch.long)
    feat = torch.randn((n, 12), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    arch = _biases(ConvStack("gatv2", [12, 8, 8], [8, 1], heads=[2, 1]).eval(), 6)
    base = {"seed": 1, "interpret_samples": 10, "epochs": 8, "optimizer": "adam", "lr": 0.01,
            "lr_patience": 10, "l1_lambda": 1e-4, "verify_arch": True}
    pw = [list(range(0, 8)), list(range(6, 20)), list(range(30, 45))] if pathways else None
    exp = Explainer(feat, ei, arch, dict(base, **(params or {})), [str(i) for i in range(n)], pw,
                    ["a", "b", "c"] if pathways else None, None, problem="node_prediction")
    return exp, str(int(np.bincount(ei[1].numpy(), minlength=n).argmax()))  # the busiest target


@pytest.mark.parametrize("sampler,pathways", [("compat", False), ("device", False), ("compat", True)])
def test_explainer_run_matches_the_generic_path(sampler, pathways, monkeypatch):
    """Explainer.run(node_prediction), times=2, verify_arch on: with attention_engine it runs on
    the engine with the arch check `verified` and agrees with a run forced onto the generic path
    (y within 1e-5 per row, both DataFrames within 1e-4); with default params the same arch runs
    on the generic path."""
    from bikg_graph_explainability_public_amd import pipeline
    params = {"mask_sampler": sampler, "attention_engine": True}
    exp, el = _explainer(params, pathways)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df, pdf = exp.run(el, 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified"
    assert all(k == "att2" for low in lr["plan"].lowering for k, _, _ in low)
    y = torch.stack([lr["repeats"][i]["y"].reshape(-1) for i in range(2)])
    assert float(y.std()) > 1e-4  # the masks move the output
    exp2, _ = _explainer(params, pathways)
    real_build_plan = pipeline.build_plan
    monkeypatch.setattr(pipeline, "build_plan", lambda *a, **k: None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df2, pdf2 = exp2.run(el, 2)
    assert exp2.last_run["engine"] is False
    y2 = torch.stack([exp2.last_run["repeats"][i]["y"].reshape(-1) for i in range(2)])
    torch.testing.assert_close(y, y2, rtol=0, atol=1e-5)
    np.testing.assert_allclose(df.loc[df2.index].values, df2.values, rtol=0, atol=1e-4)
    assert (pdf is None) == (not pathways)
    if pathways:
        np.testing.assert_allclose(pdf.loc[pdf2.index].select_dtypes("number").values,
                                   pdf2.select_dtypes("number").values, rtol=0, atol=1e-4)
    monkeypatch.setattr(pipeline, "build_plan", real_build_plan)
    exp3, _ = _explainer({"mask_sampler": sampler}, pathways)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp3.run(el, 2)
    assert exp3.last_run["engine"] is False  # no opt-in: the generic path
