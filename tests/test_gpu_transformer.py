"""GPU parity of the opt-in TransformerConv (dot-product attention) engine path: ForwardPlan terms
of kind "qkv" (k_agg_qkv in csrc/xpgnn.hip, k_dense for the deeper layers' transforms) against the
fp64 per-target restatement of tests/transformer_ref.py.  Bars (those of test_gpu_gatv2.py): forward
outputs behind a sigmoid atol 1e-5 against fp64; with an identity final activation, for the pooled
models and for the x 32 spread case max(1e-5, 4 x e32), e32 = the error of the nn.py module in
float32 on CPU torch against fp64; DataFrames atol 1e-4.  XPG_FORWARD is unset unless a test says
otherwise.

Measured on the MI355X (max |engine - fp64|): see DESIGN.md section 4k."""
import copy
import warnings

import numpy as np
import pytest
import torch

import block_ref
import oracle
import pool_ref
import transformer_ref as tref
from transformer_ref import QUERIES

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
    assert got == (kinds or [["qkv"]] * len(plan.lowering)), got
    assert plan.describe(64).startswith("unfused")
    return plan


def _check(got, ref, atol=1e-5):
    got = got.cpu().numpy()
    print("max |engine - fp64| =", float(np.abs(got - ref).max()), "bar", atol)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)


_MASKS = tref.row_masks(64, S, 3, QUERIES)


def _case(arch, rel_edges=None):
    x, ei = tref.features(S), tref.hub_graph(S)
    ref = tref.union_outputs(arch, x.numpy(), rel_edges(ei) if rel_edges else [ei], _MASKS)[:, QUERIES]
    return x, ei, ref


def _e32(arch, x, ei, ref, masks=_MASKS, queries=QUERIES):
    """The float32 CPU module on the union graph against the fp64 reference."""
    keep, tiled = oracle.build_edge_mask(masks, ei)
    with torch.no_grad():
        y32 = arch(x.repeat(masks.shape[0], 1), torch.as_tensor(tiled[:, keep]))
    return float(np.abs(y32[:, 0].reshape(masks.shape).double().numpy()[:, queries] - ref).max())


# ------------------------------------------------------------------ the hub case
@pytest.mark.parametrize("q_scale", [1.0, 32.0])
@pytest.mark.parametrize("root,beta", [(True, False), (True, True), (False, False)])
def test_hub_vs_fp64_union_graph(root, beta, q_scale):
    """Two TransformerConv layers (heads [2, 1], C = 8) on the hub graph: duplicate edges, stored
    self-loops (ordinary edges), a 300-in-edge hub, all-off / all-on rows and rows with the query
    itself masked; lin_query x 32 spreads the logits (softmax stability; bar max(1e-5, 4 x e32)
    there).  tests/test_transformer_cpu.py shows from the reference alone that these outputs move
    with the masks, with the logits and with the gate."""
    c = tref.hub_case(root, beta, q_scale)
    span = tref.layer1_logit_span(c["arch"], c["x"].numpy(), c["ei"])
    print("layer-1 logit span =", span)
    assert q_scale == 1.0 or span > 89.0  # past ln(FLT_MAX) without the max subtraction
    bar = 1e-5
    if q_scale != 1.0:
        e32 = _e32(c["arch"], c["x"], c["ei"], c["ref"], c["masks"])
        print("e32 =", e32)
        bar = max(1e-5, 4 * e32)
    plan = _plan(c["arch"], c["x"], c["ei"])
    _check(plan.forward(_pack(c["masks"])), c["ref"], bar)


# ------------------------------------------------------------------ heads x channels
@pytest.mark.parametrize("H,C", [(1, 1), (4, 1), (2, 3), (3, 5), (1, 8), (2, 16), (4, 16), (8, 32),
                                 (1, 256), (3, 40)])
def test_head_and_channel_matrix(H, C):
    """Every shape as layer 1 and as a deeper layer: the aligned kernel (head_ch / 4 a power of
    two: 8, 16, 32, 256) and the general one (heads inside a chunk: 1; chunks straddling heads: 3,
    5; head_ch / 4 = 10), lane groups of 8 (width 32), 16 (64), 32 (128) and 64 (256, the limit:
    the deeper layer's four transforms take four k_dense launches there).  Root and the gate
    alternate over the cases."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(100 * H + C)
    root, beta = (H + C) % 2 == 0, (H + C) % 4 == 0
    arch = ConvStack("transformer", [16, C, C], [H * C, 1], heads=[H, H], beta=beta, root_weight=root).eval()
    x, ei, ref = _case(arch)
    print("root", root, "beta", beta, "reference output range", float(ref.min()), float(ref.max()))
    _check(_plan(arch, x, ei).forward(_pack(_MASKS)), ref)


def _swap(arch, i, conv):
    arch.conv[i] = conv
    return arch


@pytest.mark.parametrize("name", ["no_bias", "mean1", "three", "w96", "gate256"])
def test_module_options(name):
    """bias=False (lin_skip without a bias), concat=False with one head, a three-conv-layer stack, a
    96-wide layer (24 chunks in a 32-lane group) and a gated layer of width 256 (the gate's
    reduction spans 64 lanes), each at both depths."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, TransformerConv
    torch.manual_seed(31)
    if name == "no_bias":
        arch = ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1])
        _swap(arch, 0, TransformerConv(16, 8, heads=2, bias=False, beta=True))
        _swap(arch, 2, TransformerConv(16, 8, heads=1, bias=False))
    elif name == "mean1":
        arch = ConvStack("transformer", [16, 8, 8], [8, 1], heads=[1, 1])
        _swap(arch, 0, TransformerConv(16, 8, heads=1, concat=False, beta=True))
        _swap(arch, 2, TransformerConv(8, 8, heads=1, concat=False, root_weight=False))
    elif name == "three":
        arch = ConvStack("transformer", [16, 8, 6, 8], [8, 1], heads=[2, 3, 1], beta=True)
    elif name == "w96":
        arch = ConvStack("transformer", [16, 32, 48], [96, 1], heads=[3, 2], beta=True)
    else:
        arch = ConvStack("transformer", [16, 64, 32], [256, 1], heads=[4, 8], beta=True)
    arch = arch.eval()
    x, ei, ref = _case(arch)
    _check(_plan(arch, x, ei).forward(_pack(_MASKS)), ref)


def test_identity_final_activation():
    """No sigmoid to compress the error: bar max(1e-5, 4 x e32)."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(17)
    arch = ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1], beta=True, final_act="identity").eval()
    x, ei, ref = _case(arch)
    e32 = _e32(arch, x, ei, ref)
    got = _plan(arch, x, ei).forward(_pack(_MASKS))
    print("e32 =", e32, "output range", float(ref.min()), float(ref.max()))
    assert float(ref.max() - ref.min()) > 0.05
    _check(got, ref, max(1e-5, 4 * e32))


# ------------------------------------------------------------------ edge-set corners
@pytest.mark.parametrize("root", [True, False])
def test_edge_set_corners(root):
    """Rows built for one corner each, queries 0 (the hub; it has a stored self-loop) and 5 (none):
    0 all-off; 1 only the queries kept (query 0 keeps its loop, query 5 nothing); 2 the queries and
    exactly one in-neighbour of each; 3 everything but the queries (a masked target has no edges:
    its row is the skip alone, and equals the all-off row); 4 all-on (the hub with all 300 extra
    in-edges).  root=True carries the gate."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    torch.manual_seed(9)
    arch = ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1], beta=root, root_weight=root).eval()
    x, ei = tref.features(S), tref.hub_graph(S)
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
    ref = tref.union_outputs(arch, x.numpy(), [ei], m)[:, qs]
    assert np.abs(ref[3] - ref[0]).max() < 1e-12  # a masked target: the all-off row
    assert abs(ref[1, 1] - ref[0, 1]) < 1e-12 and abs(ref[1, 0] - ref[0, 0]) > 1e-6  # the loop of node 0
    assert len({round(float(v), 9) for v in ref[:, 0]}) == 4
    _check(_plan(arch, x, ei, qs).forward(_pack(m)), ref)


# ------------------------------------------------------------------ relations, other kinds, readout
def test_single_type_hetero_two_relations():
    from bikg_graph_explainability_public_amd.nn import ConvStack
    rels = [("n", "a", "n"), ("n", "b", "n")]
    torch.manual_seed(4)
    arch = ConvStack("transformer", [16, 8, 8], [8, 1], hetero_rels=rels, heads=[2, 1], beta=True).eval()
    et = (np.arange(tref.hub_graph(S).shape[1]) % 3 == 0).astype(np.int64)
    x, ei, ref = _case(arch, lambda ei: [ei[:, et == 0], ei[:, et == 1]])
    plan = _plan(arch, x, ei, et=et, rels=rels)
    assert [(k, r) for k, r, _ in plan.lowering[1]] == [("qkv", 0), ("qkv", 1)]
    _check(plan.forward(_pack(_MASKS)), ref)


def test_gcn_then_transformer():
    """Degrees are needed by layer 1 only; the TransformerConv layer reads the GCN layer's rows."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, TransformerConv
    torch.manual_seed(6)
    arch = ConvStack("gcn", [16, 8, 8], [8, 1])
    arch = _swap(arch, 2, TransformerConv(8, 4, heads=2, beta=True)).eval()
    x, ei, ref = _case(arch)
    _check(_plan(arch, x, ei, kinds=[["gcn"], ["qkv"]]).forward(_pack(_MASKS)), ref)


def test_transformer_then_sage():
    """The SAGE layer's dense input follows a layer that ends without a dense launch."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, TransformerConv
    torch.manual_seed(7)
    arch = ConvStack("sage", [16, 8, 8], [8, 1])
    arch = _swap(arch, 0, TransformerConv(16, 4, heads=2)).eval()
    x, ei, ref = _case(arch)
    _check(_plan(arch, x, ei, kinds=[["qkv"], ["mean", "root"]]).forward(_pack(_MASKS)), ref)


@pytest.mark.parametrize("pool", ["mean", "add", "max"])
def test_pooled_model(pool):
    """The readout after two TransformerConv layers, identity head (a sum over 400 nodes would sit
    on a sigmoid's tail): bar max(1e-5, 4 x e32), e32 = the float32 CPU module against fp64."""
    from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel
    torch.manual_seed(8)
    enc = ConvStack("transformer", [16, 8, 8], [8], heads=[2, 1], beta=True)
    arch = PooledModel(enc, pool, [8, 1], final_act="identity").eval()
    x, ei = tref.features(S), tref.hub_graph(S)
    ref = tref.pooled_outputs(arch, x.numpy(), [ei], _MASKS)
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


def test_block_stack_layer_norm_and_residual():
    """BlockStack("transformer", norm="layer", residual=True): LayerNorm, ReLU and the skip are the
    attention layer's post-op; the reference runs the conv modules in fp64 (block_ref)."""
    from bikg_graph_explainability_public_amd.nn import BlockStack
    torch.manual_seed(12)
    arch = BlockStack("transformer", [16, 16, 16], [32, 1], norm="layer", residual=True, heads=[2, 2],
                      beta=True).eval()
    block_ref.randomise_norms(arch, 3)
    x, ei = tref.features(S), tref.hub_graph(S)
    ref = block_ref.union_outputs(arch, x.numpy(), ei, _MASKS)[:, QUERIES]
    plan = _plan(arch, x, ei)
    assert plan.program.convs[1].post.residual and plan.program.convs[0].post.norm == "layer"
    assert " post" in plan.describe(64)
    _check(plan.forward(_pack(_MASKS)), ref)


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
    max_ws_bytes that forces 16-row chunks gives the same bits; two calls are equal.  Both models
    carry the gate."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    if kind == "aligned":
        arch = tref.hub_case(True, True)["arch"]
    else:
        torch.manual_seed(2)
        arch = ConvStack("transformer", [16, 5, 6], [12, 1], heads=[3, 2], beta=True).eval()
    x, ei = tref.features(S), tref.hub_graph(S)
    plan = _plan(arch, x, ei)
    bits = _pack(tref.row_masks(70, S, 6, QUERIES))
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
    c = tref.hub_case(True, True)
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
def _explainer(params=None, pathways=False, classes=1):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack
    n = 60
    g = np.random.default_rng(1)
    ei = torch.as_tensor(g.integers(0, n, (2, 240)), dtype=torch.long)
    feat = torch.randn((n, 12), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    arch = ConvStack("transformer", [12, 8, 8], [8, classes], heads=[2, 1], beta=True,
                     final_act="sigmoid" if classes == 1 else "softmax").eval()
    if classes > 1:
        with torch.no_grad():  # logits that tell the classes apart
            arch.fc[0].weight.mul_(4.0)
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
    assert all(k == "qkv" for low in lr["plan"].lowering for k, _, _ in low)
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


def test_run_classes_on_a_softmax_head(monkeypatch):
    """run_classes over the 3 classes of a softmax head: on the engine (k_class_out after the qkv
    layers), arch check `verified`, rows that are distributions, agreeing with the run forced onto
    the generic path (y within 1e-5, DataFrames within 1e-4)."""
    from bikg_graph_explainability_public_amd import pipeline
    params = {"attention_engine": True}
    exp, el = _explainer(params, classes=3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = exp.run_classes(el, None, 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified" and lr["classes"] == [0, 1, 2]
    assert all(k == "qkv" for low in lr["plan"].lowering for k, _, _ in low)
    assert lr["plan"].describe(16).endswith("class=k_class_out<softmax,all>")
    y = lr["y"].double()
    torch.testing.assert_close(y.sum(-1), torch.ones_like(y[..., 0]), rtol=0, atol=1e-5)
    assert float(y[..., 0].std()) > 1e-4 and float((y[..., 0] - y[..., 2]).abs().max()) > 1e-3
    exp2, _ = _explainer(params, classes=3)
    monkeypatch.setattr(pipeline, "build_plan", lambda *a, **k: None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out2 = exp2.run_classes(el, None, 2)
    assert exp2.last_run["engine"] is False
    torch.testing.assert_close(lr["y"], exp2.last_run["y"].to(lr["y"].device), rtol=0, atol=1e-5)
    for (df, _), (df2, _) in zip(out, out2):
        np.testing.assert_allclose(df.loc[df2.index].values, df2.values, rtol=0, atol=1e-4)
