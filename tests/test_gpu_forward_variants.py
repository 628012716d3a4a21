"""Every kernel variant of the rows, fused and multi-kernel forward paths (k_rows_forward with its
run-time forms, k_fused_forward, k_agg_l1_rows, k_agg, k_dense with and without the HEAD epilogue)
against the fp64 oracle, with the variant pinned: each case of tests/forward_ref.py sets its
environment and asserts ForwardPlan.kernels() -- the picks the launches themselves dispatch on --
before it compares numbers, so a case cannot quietly test another kernel.

Inputs (forward_ref): one 300-node graph with hub targets of in-degree 70 and 130, a target
without in-edges, self-loops and duplicated edges; 130 mask rows (two 64-row blocks + 2) with an
all-on, an all-off and a 3 % row.  Bar: atol 1e-5 against fp64, rtol 0 (the bar of
test_gpu_parity.py and test_gpu_wide_variants.py) on every output column and every row.
tests/test_forward_variants_cpu.py checks that the cases name every instantiation in the library
(or list it as unreachable) and that the references can tell a wrong kernel."""
import functools

import numpy as np
import pytest
import torch

import forward_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in fr.ENV:
        monkeypatch.delenv(k, raising=False)


def _eng():
    from bikg_graph_explainability_public_amd import engine
    return engine


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _bits():
    return _eng().pack_masks(torch.as_tensor(fr.masks().copy()).to(DEV))


def _build(kind, dims, fc, queries, n_rel, out_col, key):
    from bikg_graph_explainability_public_amd import pipeline
    arch = fr._arch(key).to(DEV)
    x = fr.features(dims[0]).to(DEV)
    ei = torch.as_tensor(fr.graph().copy(), device=DEV)
    q = list(fr.QUERIES[queries])
    if n_rel > 1:
        et, _ = fr.relation_edges(n_rel)
        plan = pipeline.build_plan(arch, x, ei, q, None, torch.as_tensor(et, device=DEV), None,
                                   fr.relation_names(n_rel), None, out_col=out_col or None)
    else:
        plan = pipeline.build_plan(arch, x, ei, q, out_col=out_col or None)
    assert plan is not None and plan.n_out == len(q)
    assert plan.frontiers[-1].tolist() == q  # output column i is query i
    return plan


@functools.lru_cache(maxsize=None)
def _plan(name):
    """The case's plan, built once per module."""
    c = fr.case(name)
    return _build(c.kind, c.dims, c.fc, c.queries, c.n_rel, c.out_col, fr.model_key(name))


def _check(name, monkeypatch):
    """kernels() first (what is about to run), then every column and row vs fp64."""
    c = fr.CASES[name]
    plan = _plan(name)
    ref = fr.reference(name)[:c.rows]
    _setenv(monkeypatch, c.env)
    assert plan.kernels(c.rows) == c.want
    got = plan.forward(_bits()[:c.rows].contiguous()).cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"[forward-variants] {name}: {c.want}  max|engine - fp64| = {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=fr.ATOL)
    return got


# ------------------------------------------------------------------ the case matrix
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_variant_vs_fp64(name, monkeypatch):
    _check(name, monkeypatch)


def test_fused_declines_what_does_not_fit(monkeypatch):
    """XPG_FORWARD=fused on a plan whose tables pass the LDS limit: refused under strict with nothing
    launched (the output keeps its sentinel), the multi-kernel path without it."""
    c = fr.FUSED_DECLINED
    plan = _build(c.kind, c.dims, c.fc, c.queries, c.n_rel, c.out_col, fr.model_key(c))
    ref = fr.reference(c)
    _setenv(monkeypatch, fr.FUSED_ENV)
    out = torch.full((fr.ROWS, plan.n_out), 12345.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.kernels(fr.ROWS)
    with pytest.raises(RuntimeError, match="does not take this plan"):
        plan.forward(_bits(), out=out)
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    assert plan.kernels(fr.ROWS) == c.want
    plan.forward(_bits(), out=out)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=fr.ATOL)


# ------------------------------------------------------------------ two plans outside the table
def test_edge_mask_plan_on_generic_layer1_vs_fp64():
    """An edge-mask plan (mask columns = the 886 edges, link decoder on the 70-in-edge hub's last
    in-edge): layer 1, 32 wide, runs k_agg<1,8,1> without any switch; the decoder's score vs fp64."""
    from bikg_graph_explainability_public_amd import pipeline
    x = fr.features(fr.EDGE_MODEL[1][0]).to(DEV)
    ei = torch.as_tensor(fr.graph().copy(), device=DEV)
    u, v = fr.edge_query()
    plan = pipeline.build_edge_plan(fr.edge_model().to(DEV), x, ei, u, v)
    assert plan is not None and plan.edge_masks and plan.cols == ei.shape[1]
    assert plan.kernels(fr.ROWS) == fr.EDGE_WANT
    bits = _eng().pack_masks(torch.as_tensor(fr.edge_masks().copy()).to(DEV))
    got = plan.forward(bits)[:, 0].cpu().numpy()
    ref = fr.edge_reference()
    print(f"[forward-variants] edge-mask: {fr.EDGE_WANT}  max|engine - fp64| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=fr.ATOL)


def test_two_type_plan_per_type_bias_vs_fp64():
    """A two-node-type plan: its conv layer's dense launch adds the bias row of each target's node
    type (k_dense<2,0>g1t); per mask row vs the fp64 restatement of the per-copy forward."""
    from bikg_graph_explainability_public_amd import pipeline
    arch, c = fr.mt_setup()
    x = torch.as_tensor(c["x"], dtype=torch.float32, device=DEV)
    ei = torch.as_tensor(c["ei"], device=DEV)
    plan = pipeline.build_plan(arch.to(DEV), x, ei, [c["sub_ind"]], torch.as_tensor(c["nt"], device=DEV),
                               torch.as_tensor(c["et"], device=DEV), c["ntypes"], c["rels"], c["pads"])
    assert plan is not None and plan.multi_type
    assert plan.kernels(fr.ROWS) == fr.MT_WANT
    bits = _eng().pack_masks(torch.as_tensor(fr.mt_masks().copy()).to(DEV))
    y = plan.forward(bits)[:, 0]
    y = torch.where(pipeline.empty_copy_rows(bits, x.shape[0], ei), torch.zeros_like(y), y)  # a copy without edges
    got, ref = y.cpu().numpy(), fr.mt_reference()
    print(f"[forward-variants] two-type: {fr.MT_WANT}  max|engine - fp64| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=fr.ATOL)


# ------------------------------------------------------------------ bitwise promises of the design
@pytest.mark.parametrize("name", ["unfused-l1rows-gcn128", "unfused-l1rows-sage256", "unfused-l1rows-sage64-rel2",
                                  "unfused-l1rows-gcn128-rel2", "unfused-l1rows-add256-rel2"])
def test_l1_rows_kernel_equals_generic_agg_bitwise(name, monkeypatch):
    """k_agg_l1_rows at 2 and 4 feature slices (widths 128 / 256) and with ONE = 0 (two aggregating
    terms) against the generic k_agg<1, LPS, 1> (XPG_AGG_GENERIC=1): the same outputs bit for bit
    (test_gpu_parity covers one slice, widths 32 / 64, ONE = 1)."""
    c = fr.CASES[name]
    plan = _plan(name)
    _setenv(monkeypatch, c.env)
    assert plan.kernels(fr.ROWS) == c.want and "l1=k_agg_l1_rows<" in c.want
    y_rows = plan.forward(_bits()).clone()
    monkeypatch.setenv("XPG_DIAGNOSTICS", "1")
    monkeypatch.setenv("XPG_AGG_GENERIC", "1")
    lps = c.dims[1] // 4
    assert plan.kernels(fr.ROWS) == c.want.replace(c.want.split()[1], f"l1=k_agg<1,{lps},1>")
    assert torch.equal(plan.forward(_bits()), y_rows)


FORM_CASES = sorted(n for n in fr.CASES if n.startswith("rows-form-"))


@pytest.mark.parametrize("name", FORM_CASES)
def test_rows_forms_ignore_workspace_contents_and_row_split(name, monkeypatch):
    """Each run-time form of the rows kernel: the output does not depend on what the workspace
    held (its block-scheduling counters are reset by the launch) nor on splitting the 130 rows
    into two calls of 70 and 60 (a row does not depend on its block or on its lane)."""
    c = fr.CASES[name]
    plan = _plan(name)
    _setenv(monkeypatch, c.env)
    bits = _bits()
    assert plan.kernels(fr.ROWS) == plan.kernels(70) == plan.kernels(60) == c.want
    full = plan.forward(bits).clone()
    for fill in (0, 0xFF, 0x5A):
        ws = torch.full((plan.workspace_bytes(fr.ROWS),), fill, dtype=torch.uint8, device=DEV)
        assert torch.equal(plan.forward(bits, workspace=ws), full), fill
    lo, hi = plan.forward(bits[:70].contiguous()).clone(), plan.forward(bits[70:].contiguous()).clone()
    assert torch.equal(torch.cat([lo, hi]), full)


# ------------------------------------------------------------------ xpg_dense: tile counts and k tails
@pytest.mark.parametrize("M,K,N", [
    (70, 24, 96), (97, 40, 150), (33, 72, 192),   # 3, 5, 6 column tiles (one column group)
    (130, 8, 128), (65, 20, 100),                 # k_dense<1,0> with 4 column groups
    (70, 8, 20), (70, 24, 32), (40, 40, 7),       # one tile: the 32-deep unrolled k loop's partial trips
    (70, 56, 64), (70, 24, 70),                   # two tiles (16-deep trips, k_pad 56) and three (8-deep)
])
def test_dense_tile_counts_and_k_tails(M, K, N):
    """The tile counts (3, 5, 6; 4 as 4 groups of 1) and k_pad tails test_dense_mfma_vs_torch_fp32 does
    not reach, with row counts that end in a partial 32-row block; its reference and tolerance."""
    e = _eng()
    g = torch.Generator().manual_seed(M + K + N)
    A = torch.randn((M, K), generator=g)
    W = torch.randn((N, K), generator=g) * torch.linspace(0.5, 2.0, K)  # asymmetric
    b = torch.randn(N, generator=g)
    for act, fn in [(None, lambda x: x), ("relu", torch.relu), ("sigmoid", torch.sigmoid)]:
        got = e.dense(A.to(DEV), W.to(DEV), b.to(DEV), act).cpu()
        ref = fn(A.double() @ W.double().T + b.double()).float()
        torch.testing.assert_close(got, ref, rtol=0, atol=2e-5 * max(1.0, K ** 0.5))
