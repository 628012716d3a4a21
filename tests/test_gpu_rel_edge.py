"""GPU parity of typed link models under edge masks (XPG_TERM_REL on edge-mask plans, the EM
instantiations of k_agg_rel, and the DistMult decoder k_edge_dot_scaled, ABI v27) against the fp64
restatement of tests/rel_edge_ref.py, everything through the C-ABI.  Bars (DESIGN §4c's): sigmoid
scores atol 1e-5 against fp64; identity scores max(1e-5, 4 x e32), e32 = the nn.py module's own
float32 CPU error on the same inputs; DataFrames atol 1e-4.  The graph and masks are
rel_edge_ref.typed_hub_graph / hub_masks (their edge cases are asserted in
tests/test_rel_edge_cpu.py, with the check that the masks move the reference outputs)."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import rel_edge_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS", "XPG_AGG_GENERIC")
PEAK_MAX = 64.0


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


def _eng():
    from bikg_graph_explainability_public_amd import engine
    return engine


def _pack(m):
    return _eng().pack_masks(torch.as_tensor(m, device=DEV))


def _model(dims, fc, R, decoder="distmult", act="sigmoid", **kw):
    from bikg_graph_explainability_public_amd import nn as xnn
    enc = xnn.RGCNStack(list(dims), list(fc), R, final_act="identity", **kw)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias") and n.startswith("conv"):
                p.uniform_(-0.2, 0.2)
    return xnn.RelLinkModel(enc, R, decoder=decoder, act=act).eval()


def _halve(model):
    with torch.no_grad():
        for n, p in model.encoder.conv.named_parameters():
            if n.endswith("weight") or n.endswith("root"):
                p.mul_(0.5)
        if model.rel_emb is not None:
            model.rel_emb.mul_(0.5)


def _fit_scale(model, x, ei, et, masks, u, v, t):
    """Halve the conv weights and rel_emb, at most 20 times, until in the fp64 REFERENCE alone (with
    the sigmoid) at least half of the outputs lie in (0.02, 0.98) and no conv pre-activation
    exceeds PEAK_MAX (float32's own limit on the hub's sums, tests/test_gpu_rgcn.py)."""
    act, model.act = model.act, "sigmoid"
    try:
        for _ in range(20):
            y, peak = ref.edge_outputs(copy.deepcopy(model).double(), x, ei, et, masks, u, v, t, True)
            if np.mean((y > 0.02) & (y < 0.98)) >= 0.5 and peak <= PEAK_MAX:
                return
            _halve(model)
    finally:
        model.act = act
    raise AssertionError("no weight scale keeps the reference outputs off the sigmoid's tails")


# name -> (num_relations, RGCNStack keywords)
FORMS = {
    "plain-3": (3, {}), "plain-32": (32, {}), "bases-40x12": (40, {"num_bases": 12}),
    "blocks-4x4": (4, {"num_blocks": 4}), "plain-3-noroot": (3, {"root_weight": False}),
    "plain-3-nobias": (3, {"bias": False}), "bases-5x3": (5, {"num_bases": 3}),
    "bases-5x10": (5, {"num_bases": 10}),
}


@functools.lru_cache(maxsize=None)
def _case(form, aggr="mean", decoder="distmult", act="sigmoid", feat="randn", query="regular",
          dims=(16, 8, 8), fc=None, rows=70):
    R, kw = FORMS[form]
    ei, et, info = ref.typed_hub_graph(R)
    S = info["S"]
    x = torch.randn((S, dims[0]), generator=torch.Generator().manual_seed(21))
    if feat == "neg":
        x = x - 3.0
    q = info[query]
    u, v, t = int(ei[0, q]), int(ei[1, q]), int(et[q])
    torch.manual_seed(17)
    model = _model(dims, fc or (dims[-1],), R, decoder, act, aggr=aggr, **kw)
    masks = ref.hub_masks(ei, et, info, q, rows=max(rows, 4))[:rows]
    _fit_scale(model, x.numpy(), ei, et, masks, u, v, t)
    want = ref.edge_outputs(copy.deepcopy(model).double(), x.numpy(), ei, et, masks, u, v, t)
    return {"x": x, "ei": ei, "et": et, "model": model, "masks": masks, "ref": want, "R": R,
            "uvt": (u, v, t), "E": ei.shape[1]}


def _plan(c, model=None):
    from bikg_graph_explainability_public_amd import pipeline
    u, v, t = c["uvt"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        plan = pipeline.build_edge_plan(copy.deepcopy(model or c["model"]).to(DEV), c["x"].to(DEV),
                                        torch.as_tensor(c["ei"], device=DEV), u, v,
                                        edge_type=torch.as_tensor(c["et"], device=DEV), label_type=t)
    assert plan is not None, [str(w.message) for w in caught]
    return plan


def _assert_rel_edge_plan(plan, c, rows):
    """The plan the test measures: REL / ROOT terms only, edge masks (columns = the edges), one
    relation per edge type, the link decoder, the multi-kernel path."""
    kinds = {k for low in plan.lowering for k, _, _ in low}
    assert kinds <= {"rel", "root"} and "rel" in kinds
    assert plan.edge_masks and plan.cols == c["E"] and plan.n_rel == c["R"] and plan.n_out == 1
    assert plan.desc.edge_masks == 1 and plan.desc.edge_dot == 1
    assert bool(plan.desc.dot_scale) == (c["model"].rel_emb is not None)
    assert plan.desc.dot_a == 0 and plan.desc.dot_b == (0 if c["uvt"][0] == c["uvt"][1] else 1)
    assert plan.describe(rows) == "unfused"


def _check(got, want, atol=1e-5):
    got = got.cpu().numpy()[:, 0]
    err = float(np.abs(got - want).max())
    print("max |engine - fp64| =", err)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=atol)
    return err


# ------------------------------------------------------------------ engine vs fp64
# a Linear(8, 8) head with no activation after the convs: the decoder then multiplies dense rows
# (headless, both rows come out of a ReLU and their product is exactly 0 on many mask rows); the
# headless form is the layer and width sweeps' below
HEAD = (8, 8)
CASES = [("plain-3", "mean"), ("plain-3", "add"), ("plain-32", "mean"), ("bases-40x12", "mean"),
         ("blocks-4x4", "add"), ("plain-3-noroot", "mean"), ("plain-3-nobias", "mean")]


@pytest.mark.parametrize("query", ["regular", "loop", "into_hub"])
@pytest.mark.parametrize("feat", ["randn", "neg"])
@pytest.mark.parametrize("form,aggr", CASES)
def test_forms_vs_fp64_union_graph(form, aggr, feat, query):
    """RelLinkModel(RGCNStack([16, 8, 8], [8, 8], R), distmult, sigmoid) on the typed hub graph, 70
    mask rows over its ~510 edge columns, three query edges (a regular edge whose source loses all
    in-edges in row 2, a self-loop edge of node 7: one target, link (0, 0); an edge into the hub).
    Measured max |engine - fp64| on an MI355X: see DESIGN §4d."""
    c = _case(form, aggr, "distmult", "sigmoid", feat, query, fc=HEAD)
    want = c["ref"]
    assert np.mean((want > 0.02) & (want < 0.98)) >= 0.5
    assert np.mean(np.abs(want - want[0]) > 1e-9) >= 0.5  # a kernel that ignores the masks cannot pass
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, 70)
    _check(plan.forward(_pack(c["masks"])), want)


@pytest.mark.parametrize("query", ["regular", "loop", "into_hub"])
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_dot_decoder_vs_fp64(aggr, query):
    c = _case("plain-3", aggr, "dot", "sigmoid", "randn", query, fc=HEAD)
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, 70)
    assert not plan.desc.dot_scale
    _check(plan.forward(_pack(c["masks"])), c["ref"])


IDENTITY = [("plain-3", "mean", "distmult"), ("plain-3", "add", "distmult"), ("plain-3", "add", "dot"),
            ("plain-32", "mean", "distmult"), ("bases-40x12", "mean", "distmult"),
            ("blocks-4x4", "add", "distmult")]


@pytest.mark.parametrize("form,aggr,decoder", IDENTITY)
def test_identity_act_vs_fp64(form, aggr, decoder):
    """No sigmoid to hide errors: bar max(1e-5, 4 x e32), e32 = the largest difference of the same
    nn.py module in float32 on CPU torch from fp64 on the same union graph.  Measured e32 / engine
    error on an MI355X host and card: see DESIGN §4d."""
    from bikg_graph_explainability_public_amd import pipeline
    c = _case(form, aggr, decoder, "identity", "randn", "into_hub", fc=HEAD)
    u, v, t = c["uvt"]
    out32 = pipeline.generic_edge_outputs(c["model"], c["x"], torch.as_tensor(c["ei"]),
                                          torch.as_tensor(c["masks"]), u, v,
                                          edge_type=torch.as_tensor(c["et"]), label_type=t)
    e32 = float(np.abs(out32.double().numpy() - c["ref"]).max())
    bar = max(1e-5, 4 * e32)
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, 70)
    got = plan.forward(_pack(c["masks"])).cpu().numpy()[:, 0]
    err = float(np.abs(got - c["ref"]).max())
    print(f"IDENTITY {form} {aggr} {decoder}: e32 = {e32:.3g}, engine = {err:.3g}, bar = {bar:.3g}, "
          f"|ref| max = {np.abs(c['ref']).max():.3g}")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, c["ref"], rtol=0, atol=bar)


# ------------------------------------------------------------------ shape sweeps
@pytest.mark.parametrize("dims", [(16, 8), (16, 8, 8), (16, 32, 16, 8)])
@pytest.mark.parametrize("form", ["plain-3", "bases-5x3"])
def test_one_two_and_three_conv_layers(form, dims):
    c = _case(form, "mean", "distmult", "sigmoid", "neg", "regular", dims=dims)
    assert np.ptp(c["ref"]) > 1e-3
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, 70)
    assert len(plan.lowering) == len(dims) - 1
    _check(plan.forward(_pack(c["masks"])), c["ref"])


@pytest.mark.parametrize("dims", [(16, 32, 8), (50, 96, 8), (64, 256, 8), (16, 32, 70)])
@pytest.mark.parametrize("form", ["plain-3", "bases-5x10"])
def test_encoder_widths(form, dims):
    """Layer 1 writing and layer 2 reading 32-, 96- and 256-wide rows (8, 24 and 64 lanes per
    item) from 16-, 50- and 64-wide features; an output of 70 columns (padded to 96) under the
    decoder; 10 bases = two slice groups, the second partial."""
    c = _case(form, "mean", "distmult", "sigmoid", "randn", "loop", dims=dims)
    assert np.ptp(c["ref"]) > 1e-3
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, 70)
    assert plan._layers[1].f_in_pad == dims[1] and plan._layers[1].f_out == dims[2]
    _check(plan.forward(_pack(c["masks"])), c["ref"])


@pytest.mark.parametrize("rows", [1, 63, 65, 70])
@pytest.mark.parametrize("form", ["plain-3", "bases-40x12"])
def test_row_counts(form, rows):
    c = _case(form, "mean", "distmult", "sigmoid", "neg", "loop")
    plan = _plan(c)
    _assert_rel_edge_plan(plan, c, rows)
    _check(plan.forward(_pack(c["masks"][:rows])), c["ref"][:rows])


# ------------------------------------------------------------------ workspace, dispatch
@pytest.mark.parametrize("form", ["plain-3", "bases-40x12"])
def test_outputs_independent_of_workspace_contents(form):
    c = _case(form, "mean", "distmult", "sigmoid", "neg", "into_hub")
    plan = _plan(c)
    bits = _pack(c["masks"])
    nb = plan.workspace_bytes(70)
    outs = []
    for fill in ("zero", "ff", "rand"):
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        if fill == "zero":
            ws.zero_()
        elif fill == "ff":
            ws.fill_(0xFF)
        else:
            ws.random_(0, 256, generator=torch.Generator(device=DEV).manual_seed(5))
        out = torch.empty((70, 1), dtype=torch.float32, device=DEV)
        plan.forward(bits, out=out, workspace=ws)
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


@pytest.mark.parametrize("path", ["rows", "fused", "wide"])
def test_forced_paths_are_declined(path, monkeypatch):
    c = _case("plain-3", "mean", "distmult", "sigmoid", "randn", "regular")
    plan = _plan(c)
    assert plan.describe(70) == "unfused"
    monkeypatch.setenv("XPG_FORWARD", path)
    assert plan.describe(70) == "unfused"
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.describe(70)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.forward(_pack(c["masks"]))


@pytest.mark.parametrize("kind,dims,fc", [("sage", [12, 16, 16], [16, 8]), ("gcn", [12, 16, 16], [16, 8])])
def test_untyped_link_plans_keep_their_kernel(kind, dims, fc):
    """nn.LinkModel plans (tests/test_edge_masks.py's archs) on this graph leave dot_scale NULL
    and launch k_edge_dot as before: against the oracle, and bitwise equal to the same plan with
    a scale vector of ones (k_edge_dot_scaled: (a * 1) * b is the same float)."""
    import oracle
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.program import compile_arch
    from test_edge_masks import _link, _spec
    ei, et, info = ref.typed_hub_graph(4)
    q = info["regular"]
    u, v = int(ei[0, q]), int(ei[1, q])
    x = np.random.default_rng(12).standard_normal((info["S"], dims[0])).astype(np.float32)
    model = _link(kind, dims, fc).to(DEV)
    xt, eit = torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV)
    plan = pipeline.build_edge_plan(model, xt, eit, u, v)
    assert plan is not None and plan.edge_masks and not plan.desc.dot_scale and plan.n_rel == 1
    m = ref.hub_masks(ei, et, info, q)
    bits = _pack(m)
    y = plan.forward(bits)
    want = oracle.masked_edge_outputs(_spec(kind, dims, fc, model), x, ei, m, u, v)
    np.testing.assert_allclose(y[:, 0].cpu().numpy(), want, atol=1e-5)
    cols = torch.arange(ei.shape[1], device=DEV)
    ones = _eng().ForwardPlan(compile_arch(model), xt, [eit], [u, v], edge_cols=[cols],
                              link=(0, 1, "sigmoid", torch.ones(fc[-1])))
    assert ones.desc.dot_scale
    assert torch.equal(ones.forward(bits), y)


def test_refusals_that_stay():
    """att / sum / max terms on edge-mask plans, and a rel_emb the output cannot take."""
    from bikg_graph_explainability_public_amd import nn as xnn
    from bikg_graph_explainability_public_amd.program import compile_arch
    ei, et, info = ref.typed_hub_graph(4)
    x = torch.randn(info["S"], 12).to(DEV)
    eit = torch.as_tensor(ei, device=DEV)
    cols = torch.arange(ei.shape[1], device=DEV)
    for kind, att in (("sage-add", False), ("sage-max", False), ("gat", True)):
        prog = compile_arch(xnn.ConvStack(kind, [12, 8], [8], final_act="identity"), attention=att)
        with pytest.raises(ValueError, match="edge-mask"):
            _eng().ForwardPlan(prog, x, [eit], [0, 1], edge_cols=[cols], link=(0, 1, "sigmoid"))
    prog = compile_arch(xnn.ConvStack("sage", [12, 8], [8], final_act="identity"))
    with pytest.raises(ValueError, match="scale vector"):
        _eng().ForwardPlan(prog, x, [eit], [0, 1], edge_cols=[cols], link=(0, 1, "sigmoid", torch.ones(5)))


# ------------------------------------------------------------------ Explainer.run end to end
PARAMS = {"seed": 3, "interpret_samples": 16, "epochs": 10, "optimizer": "adam", "lr": 0.01,
          "lr_patience": 10, "l1_lambda": 1e-4, "edge_masks": True, "verify_arch": True}


def _explainer(sampler, comms=False, seed=12, **kw):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    g = np.random.default_rng(41)
    S, E, R = 300, 1200, 6
    ei = g.integers(0, S, (2, E)).astype(np.int64)
    ei[:, :5] = ei[0, :5]       # self-loops
    ei[:, 5:10] = ei[:, 10:15]  # duplicates
    et = g.integers(0, R - 1, E).astype(np.int64)
    x = g.standard_normal((S, 12)).astype(np.float32)
    torch.manual_seed(seed)
    model = _model([12, 16, 16], [16, 16], R, num_bases=3)
    names = [f"edge_{i}" for i in range(E)]
    pw = pw_names = None
    if comms:
        import oracle
        _, _, pos, _, _ = oracle.edge_comp_graph(40, 2, ei, S)
        sub = [names[p] for p in pos]
        pw, pw_names = [sub[i::4] for i in range(4)], [f"c{i}" for i in range(4)]
    exp = Explainer(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), model,
                    dict(PARAMS, mask_sampler=sampler, **kw), names, pathways=pw, pathway_names=pw_names,
                    problem="edge_prediction", node_types=torch.ones(S, dtype=torch.long),
                    edge_types=torch.from_numpy(et))
    return exp, et


@pytest.mark.parametrize("sampler,comms", [("compat", False), ("device", False), ("device", True)])
def test_explainer_run_matches_the_generic_path(sampler, comms, monkeypatch):
    from bikg_graph_explainability_public_amd import pipeline
    exp, et = _explainer(sampler, comms)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df, pdf = exp.run("edge_40", 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    assert exp.last_run["engine"] is True and exp.last_run["arch_check"] == "verified"
    plan = exp.last_run["plan"]
    assert plan.edge_masks and plan.n_rel == 6 and plan.desc.dot_scale
    assert "rel" in {k for low in plan.lowering for k, _, _ in low}
    assert (pdf is not None) == comms and exp.last_run["S"] == plan.cols
    y = torch.stack([exp.last_run["repeats"][i]["y"].reshape(-1) for i in range(2)])
    # the same inputs again: the cached plan; a permuted edge_types tensor: a new one
    exp.run("edge_40", 2)
    assert exp.last_run["query_cache"] == "hit" and exp.last_run["plan"] is plan
    keep_type = int(et[40])
    perm = torch.from_numpy(np.random.default_rng(1).permutation(et))
    perm[40] = keep_type
    exp.edge_types = perm
    exp.run("edge_40", 2)
    assert exp.last_run["query_cache"] == "miss" and exp.last_run["plan"] is not plan
    assert exp.last_run["engine"] is True
    y_perm = torch.stack([exp.last_run["repeats"][i]["y"].reshape(-1) for i in range(2)])
    assert float((y_perm - y).abs().max()) > 1e-6  # the types reached the plan
    # the generic path on the same masks (fixed seed)
    exp2, _ = _explainer(sampler, comms)
    monkeypatch.setattr(pipeline, "build_edge_plan", lambda *a, **k: None)
    df2, pdf2 = exp2.run("edge_40", 2)
    assert exp2.last_run["engine"] is False
    y2 = torch.stack([exp2.last_run["repeats"][i]["y"].reshape(-1) for i in range(2)])
    torch.testing.assert_close(y, y2, rtol=0, atol=1e-5)
    np.testing.assert_allclose(df.loc[df2.index].values, df2.values, rtol=0, atol=1e-4)
    if comms:
        np.testing.assert_allclose(pdf.loc[pdf2.index, "score"].values, pdf2["score"].values,
                                   rtol=0, atol=1e-4)


def test_explainer_refusals():
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from case_builders import build_explainer
    exp, _ = _explainer("compat")
    # a node problem on a link model: LinkModel's ValueError
    node = Explainer(exp.feat, exp.edge_index, exp.arch, dict(PARAMS, edge_masks=False),
                     [f"n{i}" for i in range(300)], problem="node_prediction",
                     node_types=exp.node_types, edge_types=exp.edge_types)
    with pytest.raises(ValueError, match="edge_prediction"):
        node.run("n3", 1)
    # without the flag the edge problem fails where the reference's does (masks.py:294)
    off = Explainer(exp.feat, exp.edge_index, exp.arch, dict(PARAMS, edge_masks=False), exp.names,
                    problem="edge_prediction", node_types=exp.node_types, edge_types=exp.edge_types)
    with pytest.raises(Exception) as info:
        off.run("edge_40", 1)
    assert not isinstance(info.value, NotImplementedError)
    # more than one node type, and named types (dict inputs), stay refused
    nt = exp.node_types.clone()
    nt[:10] = 0
    two = Explainer(exp.feat, exp.edge_index, exp.arch, dict(PARAMS), exp.names,
                    problem="edge_prediction", node_types=nt, edge_types=exp.edge_types)
    with pytest.raises(NotImplementedError):
        two.run("edge_40", 1)
    het, _, meta = build_explainer("hetero_single")
    key = list(het.edge_index.keys())[0]
    named = Explainer(het.feat, het.edge_index, exp.arch, dict(PARAMS), het.names,
                      element_type=key, problem="edge_prediction")
    with pytest.raises(NotImplementedError):
        named.run(meta["element"], 1)
