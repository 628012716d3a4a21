"""Every kernel variant of the wide forward (run_wide_forward in csrc/xpgnn.hip) against the fp64
oracle, with the variant pinned: each case runs under XPG_FORWARD=wide + XPG_FORWARD_STRICT=1 and
asserts ForwardPlan.describe() -- the library's own dispatch decision -- before it compares
numbers, so a case cannot quietly test another kernel.

One graph for the whole module: 300 nodes, ~1,800 random edges, 10 explicit self-loops, 10
duplicated edges, hub targets of in-degree 300 (past layer 2's 256-entry in-edge list: its
in-place rounds) and 140 (past the 128-entry layer-1 staging round; thresholds as in
test_gpu_coverage.test_hub_targets_all_nodes); every node is a target.  70 mask rows = two
32-sample passes + a partial pass of 6: row 0 all-on, row 1 all-off, row 2 at 3 % density, the
rest with per-row keep probabilities in (0.2, 0.9).

Bar: atol 1e-5 against fp64, rtol 0 (the bar of test_gpu_parity.py) on all S columns.  The last
test checks that the variants asserted here are all the variants the dispatcher can name."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle
from golden_utils import oracle_spec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S, ROWS, F_IN = 300, 70, 16
ATOL = 1e-5
SWITCHES = ("XPG_WIDE_B3", "XPG_WIDE_OVERLAP", "XPG_DIAGNOSTICS", "XPG_WIDE_L1_GATHER",
            "XPG_WIDE_DBG")
GATHER = {"XPG_DIAGNOSTICS": "1", "XPG_WIDE_L1_GATHER": "1"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _wide_strict(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("XPG_FORWARD", "wide")
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")


def _eng():
    from bikg_graph_explainability_public_amd import engine
    return engine


# ------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def _graph():
    rng = np.random.default_rng(41)
    ei = rng.integers(0, S, (2, 1800))
    ei = ei[:, ei[0] != ei[1]]
    loops = rng.choice(S, 10, replace=False)
    dup = ei[:, rng.choice(ei.shape[1], 10, replace=False)]
    hubs = [np.stack([rng.integers(2, S, deg), np.full(deg, node)]) for node, deg in ((0, 300), (1, 140))]
    ei = np.concatenate([ei, np.stack([loops, loops]), dup] + hubs, 1)
    ei = ei[:, rng.permutation(ei.shape[1])].astype(np.int64)
    indeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=S)
    assert indeg[0] >= 300 and 256 >= indeg[1] >= 140 and int((ei[0] == ei[1]).sum()) == 10
    x = torch.randn((S, F_IN), generator=torch.Generator().manual_seed(5))
    return ei, x


@functools.lru_cache(maxsize=None)
def _masks():
    rng = np.random.default_rng(3)
    m = rng.random((ROWS, S)) < rng.uniform(0.2, 0.9, (ROWS, 1))
    m[0] = True
    m[1] = False
    m[2] = rng.random(S) < 0.03
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _bits():
    return _eng().pack_masks(torch.as_tensor(_masks().copy()).to(DEV))


def _rel_edges(n_rel):
    """The graph's edges split over n_rel relations (edge i belongs to relation i % n_rel)."""
    ei, _ = _graph()
    et = np.arange(ei.shape[1]) % n_rel
    return et, [ei[:, et == r] for r in range(n_rel)]


@functools.lru_cache(maxsize=None)
def _model(kind, dims, fc, n_rel=1, out_col=0):
    """(plan, fp64 reference [ROWS, S] in the plan's column order), built once per model."""
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.nn import ConvStack
    ei, x = _graph()
    rels = [("n", "r%d" % r, "n") for r in range(n_rel)] if n_rel > 1 else None
    torch.manual_seed(11)
    arch = ConvStack(kind, list(dims), list(fc), hetero_rels=rels).eval()
    a = {"kind": kind, "dims": list(dims), "fc": list(fc)}
    if rels:
        a["hetero_rels"] = rels
    spec = oracle_spec({"arch_spec": a}, {k: v.detach().numpy().copy() for k, v in arch.state_dict().items()})
    if out_col:  # the oracle reads output column 0: hand it the picked row of the last head layer
        spec["fc"][-1]["W"] = spec["fc"][-1]["W"][out_col:out_col + 1]
        spec["fc"][-1]["b"] = spec["fc"][-1]["b"][out_col:out_col + 1]
    if rels:
        et, parts = _rel_edges(n_rel)
        ref = oracle.masked_all_outputs(spec, x.numpy(), dict(zip(rels, parts)), _masks())
        plan = pipeline.build_plan(arch.to(DEV), x.to(DEV), torch.as_tensor(ei, device=DEV),
                                   list(range(S)), None, torch.as_tensor(et, device=DEV), None, rels, None)
    else:
        ref = oracle.masked_all_outputs(spec, x.numpy(), {None: ei}, _masks())
        if out_col:
            prog = dataclasses.replace(pipeline.compiled_program(arch.to(DEV)), out_col=out_col)
            plan = _eng().ForwardPlan(prog, x.to(DEV), [torch.as_tensor(ei, device=DEV)], list(range(S)))
        else:
            plan = pipeline.build_plan(arch.to(DEV), x.to(DEV), torch.as_tensor(ei, device=DEV),
                                       list(range(S)))
    assert plan is not None and plan.n_out == S
    ref = ref[:, plan.frontiers[-1]]  # output column i is node frontiers[-1][i]
    ref.setflags(write=False)
    return plan, ref


def _check(plan, ref, want, label):
    """describe() first (the kernel pair that is about to run), then all S columns vs fp64."""
    assert plan.describe(ROWS) == want
    got = plan.forward(_bits()).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"[wide-variants] {label}: {want}  max|engine - fp64| = {err:.3e}")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ a. instantiation matrix
L2_PIPE = "k_wide_last_ws<8,32,8,1,pipe>"
# id: (kind, dims, fc, output column, environment, layer-1 kernel, layer-2 kernel)
MATRIX = {
    "01-sage32": ("sage", (16, 32, 32), (32, 1), 0, {}, "k_wide_tgt<2,0,0>", "k_wide_tgt<2,1,8>"),
    "02-gcn32": ("gcn", (16, 32, 32), (32, 1), 0, {}, "k_wide_tgt<2,0,0>", "k_wide_tgt<2,1,4>"),
    "03-gcn64": ("gcn", (16, 64, 32), (32, 1), 0, {}, "k_wide_l1s<1,1>", "k_wide_tgt<4,1,8>"),
    "04-sage64": ("sage", (16, 64, 64), (64, 1), 0, {}, "k_wide_l1s<1,0>", "k_wide_tgt<4,1,16>"),
    "05-gcn128": ("gcn", (16, 128, 64), (64, 1), 0, {}, "k_wide_l1s<2,1>", "k_wide_tgt<8,1,16>"),
    "06-sage192": ("sage", (16, 192, 64), (64, 1), 0, {}, "k_wide_tgt<12,0,0>", "k_wide_tgt<12,1,0>"),
    "07-gcn192": ("gcn", (16, 192, 64), (64, 1), 0, {}, "k_wide_tgt<12,0,0>", "k_wide_tgt<12,1,0>"),
    "08-sage256": ("sage", (16, 256, 64), (64, 1), 0, {}, "k_wide_l1s<4,0>", "k_wide_tgt<16,1,0>"),
    "09-gcn256": ("gcn", (16, 256, 64), (64, 1), 0, {}, "k_wide_l1s<4,1>", "k_wide_tgt<16,1,0>"),
    "10-sage64-out160": ("sage", (16, 64, 160), (160, 1), 0, {}, "k_wide_l1s<1,0>", "k_wide_tgt<4,1,0>"),
    "11-gcn32-out256": ("gcn", (16, 32, 256), (256, 1), 0, {}, "k_wide_tgt<2,0,0>", "k_wide_tgt<2,1,0>"),
    "12-sage128": ("sage", (16, 128, 128), (128, 1), 0, {}, "k_wide_l1s<2,0>", L2_PIPE),
    "13-sage128-exact": ("sage", (16, 128, 128), (128, 1), 0, {"XPG_WIDE_B3": "0"},
                         "k_wide_l1s<2,0>", "k_wide_last_ws<8,32,8,0>"),
    "14-sage128-head2": ("sage", (16, 128, 128), (128, 16, 1), 0, {}, "k_wide_l1s<2,0>", "k_wide_tgt<8,1,0>"),
    # four logits, output column 2: the head tile path with a column pick (no fused single logit)
    "15-sage128-col2": ("sage", (16, 128, 128), (128, 4), 2, {}, "k_wide_l1s<2,0>", "k_wide_tgt<8,1,0>"),
    # layer widths that are no multiple of 32 (padded to 64 / 32: zero columns in h1 and in K)
    "16-sage48": ("sage", (16, 48, 24), (24, 1), 0, {}, "k_wide_l1s<1,0>", "k_wide_tgt<4,1,16>"),
    # <8,1,0> with a GCN term: layer-2 output wider than 128
    "17-gcn128-out160": ("gcn", (16, 128, 160), (160, 1), 0, {}, "k_wide_l1s<2,1>", "k_wide_tgt<8,1,0>"),
    "18-sage192-out192": ("sage", (16, 192, 192), (192, 1), 0, {}, "k_wide_tgt<12,0,0>", "k_wide_tgt<12,1,0>"),
}
# every layer-1 width again on the 16-lane-group gather layer 1 (k_wide_tgt<NFI,0,0>)
for _id, _nfi in (("03-gcn64", 4), ("04-sage64", 4), ("05-gcn128", 8), ("12-sage128", 8),
                  ("13-sage128-exact", 8), ("08-sage256", 16), ("09-gcn256", 16)):
    _c = MATRIX[_id]
    MATRIX[_id + "-gather"] = _c[:4] + ({**_c[4], **GATHER}, f"k_wide_tgt<{_nfi},0,0>", _c[6])


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_instantiation_matrix(case, monkeypatch):
    kind, dims, fc, out_col, env, l1, l2 = MATRIX[case]
    plan, ref = _model(kind, dims, fc, 1, out_col)
    _setenv(monkeypatch, env)
    _check(plan, ref, f"wide l1={l1} l2={l2}", case)


# ------------------------------------------------------------------ b. single-type HeteroConv
# id: (kind, hidden, relations, layer-1 kernel, layer-2 kernel).  SAGE relations lower to one MEAN
# term each + one summed ROOT term, GCN relations to one GCN term each: layer 1 is the gather
# kernel (k_wide_l1s takes one aggregating term), layer 2 a generic k_wide_tgt.
HETERO = {
    "sage64": ("sage", 64, 2, "k_wide_tgt<4,0,0>", "k_wide_tgt<4,1,0>"),
    "gcn64": ("gcn", 64, 2, "k_wide_tgt<4,0,0>", "k_wide_tgt<4,1,16>"),
    "sage128": ("sage", 128, 2, "k_wide_tgt<8,0,0>", "k_wide_tgt<8,1,0>"),
    "gcn128": ("gcn", 128, 2, "k_wide_tgt<8,0,0>", "k_wide_tgt<8,1,0>"),
    # four 32-wide layer-2 terms (K = 128 at nfi 2): the wide layout took these plans and the
    # launch then failed with "unsupported layer width"; they run on k_wide_tgt<2,1,0>
    "sage32x3": ("sage", 32, 3, "k_wide_tgt<2,0,0>", "k_wide_tgt<2,1,0>"),
    "gcn32x4": ("gcn", 32, 4, "k_wide_tgt<2,0,0>", "k_wide_tgt<2,1,0>"),
}


@pytest.mark.parametrize("case", sorted(HETERO))
def test_single_type_hetero_on_wide_path(case):
    """HeteroConv over same-type relations on the wide path (n_rel > 1), against the oracle's
    per-relation sum."""
    kind, hid, n_rel, l1, l2 = HETERO[case]
    plan, ref = _model(kind, (F_IN, hid, hid), (hid, 1), n_rel)
    assert plan.desc.n_rel == n_rel
    _check(plan, ref, f"wide l1={l1} l2={l2}", "hetero-" + case)


# ------------------------------------------------------------------ hand-built layer-2 terms
# The warp-specialised layer 2 has four variants no module lowers to (program.py gives a layer
# with a ROOT term exactly one MEAN term and K = 2 x width; every other multi-term layer has two
# or more aggregating terms).  Programs written term by term reach them:
# id: (layer-1 terms, layer-2 terms, width, environment, layer-1 kernel, layer-2 kernel)
HAND = {
    "gcn-root-128": (("gcn",), ("gcn", "root"), 128, {}, "k_wide_l1s<2,1>", "k_wide_last_ws<8,32,8,1>"),
    "gcn-root-128-exact": (("gcn",), ("gcn", "root"), 128, {"XPG_WIDE_B3": "0"},
                           "k_wide_l1s<2,1>", "k_wide_last_ws<8,32,8,0>"),
    "mean-root2-128": (("mean", "root"), ("mean", "root", "root"), 128, {},
                       "k_wide_l1s<2,0>", "k_wide_last_ws<8,0,8,0>"),
    "mean-root3-64": (("mean", "root"), ("mean", "root", "root", "root"), 64, {},
                      "k_wide_l1s<1,0>", "k_wide_last_ws<4,32,8,0>"),
    "mean-root2-64": (("mean", "root"), ("mean", "root", "root"), 64, {},
                      "k_wide_l1s<1,0>", "k_wide_last_ws<4,0,8,0>"),
    "root-mean-128": (("mean", "root"), ("root", "mean"), 128, {}, "k_wide_l1s<2,0>", L2_PIPE),
}


def _term_fp64(kind, h, src, dst, W):
    """One aggregation term on the (already perturbed) union graph, in fp64 (xpgnn.h: GCN =
    D^-1/2 (A + I) D^-1/2 h W^T, MEAN = mean over kept in-edges (h W^T), ROOT = h W^T)."""
    n = h.shape[0]
    if kind == "gcn":
        return oracle.gcn_conv(h, src, dst, n, W, None)
    if kind == "mean":
        cnt = np.bincount(dst, minlength=n).astype(np.float64)
        return (oracle.segment_sum(h[src], dst, n) / np.maximum(cnt, 1.0)[:, None]) @ W.T
    return h @ W.T


@functools.lru_cache(maxsize=None)
def _hand_model(l1_terms, l2_terms, width):
    from bikg_graph_explainability_public_amd.program import ConvLayer, HeadLayer, ModelProgram, Term
    ei, x = _graph()
    g = torch.Generator().manual_seed(29 + width + len(l2_terms))
    convs, f_in = [], F_IN
    for kinds in (l1_terms, l2_terms):
        terms = [Term(k, 0 if k != "root" else -1,
                      torch.randn((width, f_in), generator=g) / np.sqrt(f_in * len(kinds)))
                 for k in kinds]
        convs.append(ConvLayer(terms, 0.1 * torch.randn(width, generator=g), "relu", f_in, width))
        f_in = width
    head = HeadLayer(torch.randn((1, width), generator=g) / np.sqrt(width),
                     0.1 * torch.randn(1, generator=g), "sigmoid")
    prog = ModelProgram(convs=convs, head=[head])
    plan = _eng().ForwardPlan(prog, x.to(DEV), [torch.as_tensor(ei, device=DEV)], list(range(S)))
    m = _masks()
    h, _ = oracle.concat_features(x.numpy().astype(np.float64), ROWS)
    keep, tiled = oracle.build_edge_mask(m, ei)
    src, dst = tiled[0][keep], tiled[1][keep]
    for conv in convs:
        out = sum(_term_fp64(t.kind, h, src, dst, t.weight.double().numpy()) for t in conv.terms)
        h = np.maximum(out + conv.bias.double().numpy(), 0)
    z = h @ head.weight.double().numpy().T + head.bias.double().numpy()
    ref = oracle.apply_act(z, "sigmoid")[:, 0].reshape(ROWS, S)[:, plan.frontiers[-1]]
    ref.setflags(write=False)
    return plan, ref


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_built_layer2_terms(case, monkeypatch):
    """Layer 2 with one aggregating non-MEAN term, with K of 192 / 384, and with the ROOT term
    first: the warp-specialised variants outside every lowering, vs an fp64 restatement of the
    terms on the reference's union graph."""
    l1_terms, l2_terms, width, env, l1, l2 = HAND[case]
    plan, ref = _hand_model(l1_terms, l2_terms, width)
    _setenv(monkeypatch, env)
    _check(plan, ref, f"wide l1={l1} l2={l2}", "hand-" + case)


# ------------------------------------------------------------------ c. row-count edges
@pytest.mark.parametrize("overlap", ["1", "0"])
def test_rows_are_independent_samples(overlap, monkeypatch):
    """Case 12 (the pipelined layer 2, with its active-first sample order): rows [0, R) of the
    70-row forward == a forward of those R rows alone, bitwise, for R on both sides of the
    32-sample pass; and a forward of one later pass's rows alone (then pass 0, buffer set 0)
    == those rows of the 70-row forward.  A sample must not depend on its pass's other lanes,
    on the pass's parity or on the buffer set, with the passes overlapped and on one stream."""
    plan, _ = _model("sage", (16, 128, 128), (128, 1))
    monkeypatch.setenv("XPG_WIDE_OVERLAP", overlap)
    assert plan.describe(ROWS) == f"wide l1=k_wide_l1s<2,0> l2={L2_PIPE}"
    bits = _bits()
    full = plan.forward(bits).clone()
    for lo, hi in [(0, 1), (0, 31), (0, 32), (0, 33), (0, 64), (32, 64), (64, 70), (33, 34)]:
        assert plan.describe(hi - lo) == plan.describe(ROWS)
        part = plan.forward(bits[lo:hi].contiguous())
        assert torch.equal(part, full[lo:hi]), (lo, hi)


def test_pass_overlap_does_not_change_outputs(monkeypatch):
    plan, _ = _model("sage", (16, 128, 128), (128, 1))
    outs = []
    for overlap in ("1", "0"):
        monkeypatch.setenv("XPG_WIDE_OVERLAP", overlap)
        outs.append(plan.forward(_bits()).clone())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ d. strict
# layer-1 width 96 has no 16-feature lane split (hidden 48 pads to 64 and IS taken: case 16)
DECLINED = [("sage", (16, 96, 32), (32, 1)), ("gcn", (16, 32, 32, 32), (32, 1))]


@pytest.mark.parametrize("kind,dims,fc", DECLINED)
def test_strict_wide_refuses_declined_plans(kind, dims, fc, monkeypatch):
    """wide + strict on a plan the wide layout declines raises and launches nothing (the output
    buffer keeps its sentinel); without strict the plan runs on the path describe() names."""
    plan, ref = _model(kind, dims, fc)
    out = torch.full((ROWS, S), 12345.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.describe(ROWS)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.forward(_bits(), out=out)
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    assert plan.describe(ROWS) == "unfused"
    plan.forward(_bits(), out=out)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=ATOL)


def test_strict_wide_does_not_run_the_rows_kernel(monkeypatch):
    """A 1-layer single-query plan: the wide layout declines it and the rows kernel takes it.
    wide + strict used to return the rows kernel's result; it must raise and launch nothing."""
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.nn import ConvStack
    ei, x = _graph()
    torch.manual_seed(11)
    arch = ConvStack("gcn", [F_IN, 32], [32, 1]).eval()
    spec = oracle_spec({"arch_spec": {"kind": "gcn", "dims": [F_IN, 32], "fc": [32, 1]}},
                       {k: v.detach().numpy().copy() for k, v in arch.state_dict().items()})
    q = 1  # the in-degree-140 hub
    ref = oracle.masked_query_outputs(spec, x.numpy(), {None: ei}, _masks(), q)
    plan = pipeline.build_plan(arch.to(DEV), x.to(DEV), torch.as_tensor(ei, device=DEV), [q])
    out = torch.full((ROWS, 1), 12345.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.describe(ROWS)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.forward(_bits(), out=out)
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    assert plan.describe(ROWS) == "rows"
    plan.forward(_bits(), out=out)
    np.testing.assert_allclose(out[:, 0].cpu().numpy(), ref, rtol=0, atol=ATOL)


# ------------------------------------------------------------------ coverage of the dispatcher
# variants the dispatcher can name that no case above can reach, each with its reason
UNREACHABLE = {}


def test_every_wide_variant_is_asserted():
    """The kernels asserted by the cases of this file + UNREACHABLE == every variant the wide
    dispatcher can name (engine.wide_variants: the table the selection picks from)."""
    asserted = set()
    for table in (MATRIX, HETERO, HAND):
        for c in table.values():
            asserted |= {"l1=" + c[-2], "l2=" + c[-1]}
    listed = set(_eng().wide_variants())
    assert not (asserted & set(UNREACHABLE)), "an asserted variant is listed as unreachable"
    assert asserted - listed == set(), "a case expects a kernel the dispatcher cannot name"
    assert listed - asserted - set(UNREACHABLE) == set()
