"""GPU parity of normalised / residual blocks on the engine: k_post (csrc/xpgnn.hip) on its own
against the fp64 NumPy restatement of tests/block_ref.py, then ForwardPlans of nn.BlockStack models
(BatchNorm folded or as a post-op affine, LayerNorm and skips as post-ops) against the fp64 reference
on the union graph.  Inputs are those of tests/test_gpu_gatv2.py: hub graph S = 400,
gatv2_ref.features, 64 rows of gatv2_ref.row_masks, queries [0, 7, 399].  Bars: atol 1e-5 against
fp64 with a sigmoid output; with an identity final activation max(1e-5, 4 x e32), e32 = the error
of the float32 CPU module against fp64 (printed); DataFrames atol 1e-4.  tests/test_blocks_cpu.py
shows on the reference alone that every case moves with the masks, its norms and its skips.

The kernel's own bar (test_post_rows_vs_numpy): inputs are N(0, 1) rows and vectors as in
block_ref.randomise_norms, so v = h * scale + shift stays below ~8 in magnitude.  The one step that
amplifies is the normalised deviation (v - mean) / sqrt(var + eps): the absolute error of
(v - mean) is a few 2^-24 x |v| (about 3 x 6e-8 x 4 = 7e-7), multiplied by 1 / sqrt(var) and
|gamma| <= 1.5.  The test asserts on its own inputs that no row's 1 / sqrt(var) exceeds 20 (a row
of 5 normal samples can come close to constant), so the amplified error stays below
7e-7 x 20 x 1.5 = 2e-5; everything else is ~10 rounded float32 operations on magnitudes <= 8, below
5e-6.  Hence atol 2e-5, rtol 1e-6.  Exact statements (the padded columns, an all-zero row) are
compared with ==."""
import copy
import warnings

import numpy as np
import pytest
import torch

import block_ref
import gatv2_ref
from block_ref import QUERIES, S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


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


def _check(got, ref, atol=1e-5):
    got = got.cpu().numpy()
    print("max |engine - fp64| =", float(np.abs(got - ref).max()), "bar", atol)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)


# ------------------------------------------------------------------ the kernel on its own
def _vecs(g, f_out, mode):
    u = lambda lo, hi: g.uniform(lo, hi, f_out).astype(np.float32)
    v = {"scale": None, "shift": None, "gamma": None, "beta": None, "norm": None}
    if mode in ("affine", "both"):
        v["scale"], v["shift"] = u(0.5, 1.5), u(-0.5, 0.5)
        v["scale"][::3] *= -1
    if mode in ("layer", "both"):
        v["norm"], v["gamma"], v["beta"] = "layer", u(0.5, 1.5), u(-0.5, 0.5)
        v["gamma"][::3] *= -1
    return v


@pytest.mark.parametrize("mode", ["affine", "layer", "both"])
@pytest.mark.parametrize("f_out,ld", [(5, 8), (5, 32), (8, 32), (32, 32), (40, 40), (40, 64), (70, 96),
                                      (256, 256)])
def test_post_rows_vs_numpy(f_out, ld, mode):
    """xpg_post_rows against fp64 NumPy: a partial float4 (5), padded columns (5 / 8 / 40 / 70),
    lane groups with idle lanes (ld 40: 10 chunks on 16 lanes; ld 96: 24 on 32), a full wave (256);
    M = 1, 63, 129 rows; with and without ReLU; with and without the skip through a shuffled
    tgt_prev (M = rows x n_tgt, n_prev = n_tgt + 5).  The buffer's padded columns hold NaN going in
    and exact 0 coming out."""
    from bikg_graph_explainability_public_amd import engine
    g = np.random.default_rng(1000 * f_out + ld)
    v = _vecs(g, f_out, mode)
    dv = {k: (None if a is None or k == "norm" else torch.as_tensor(a)) for k, a in v.items()}
    want_kernel = "k_post<%s,%%d>" % ("layer" if v["norm"] else "none")
    worst = 0.0
    for rows, n_tgt in ((1, 1), (3, 21), (3, 43)):
        M = rows * n_tgt
        for act in (None, "relu"):
            for res in (False, True):
                h = np.full((M, ld), np.nan, dtype=np.float32)
                h[:, :f_out] = g.standard_normal((M, f_out))
                hp = tp = None
                if res:
                    hp = g.standard_normal((rows, n_tgt + 5, ld)).astype(np.float32)
                    tp = g.permutation(n_tgt + 5)[:n_tgt].astype(np.int32)
                ref = block_ref.post_rows(h, f_out, v["scale"], v["shift"], v["norm"], v["gamma"], v["beta"],
                                          1e-5, act, hp, tp)
                if v["norm"]:  # the amplification the bar assumes (module docstring)
                    pre = block_ref.post_rows(h, f_out, v["scale"], v["shift"])[:, :f_out]
                    assert M == 1 or (1.0 / np.sqrt(pre.var(1) + 1e-5)).max() < 20.0
                assert engine.post_describe(M, ld, f_out, v["norm"], res).startswith(want_kernel % res)
                ht = torch.as_tensor(h, device=DEV)
                got = engine.post_rows(ht, f_out, dv["scale"], dv["shift"], v["norm"], dv["gamma"], dv["beta"],
                                       1e-5, act, None if hp is None else torch.as_tensor(hp, device=DEV),
                                       None if tp is None else torch.as_tensor(tp, device=DEV))
                assert got is ht
                got = got.cpu().numpy()
                assert np.isfinite(got).all()
                assert (got[:, f_out:] == 0).all() and not np.signbit(got[:, f_out:]).any()
                worst = max(worst, float(np.abs(got - ref).max()))
                np.testing.assert_allclose(got, ref, rtol=1e-6, atol=2e-5)
    print("max |k_post - fp64| =", worst, "bar 2e-5")


@pytest.mark.parametrize("f_out,ld", [(5, 32), (40, 64), (256, 256)])
def test_post_rows_zero_row_gives_beta_exactly(f_out, ld):
    """LayerNorm of an all-zero row: mean 0, variance 0, every deviation 0, so the output is beta
    bit for bit (also without affine: 0), whatever the other rows of the wave hold."""
    from bikg_graph_explainability_public_amd import engine
    g = np.random.default_rng(f_out)
    h = g.standard_normal((37, ld)).astype(np.float32)
    h[[0, 17, 36]] = 0
    h[:, f_out:] = np.nan
    v = _vecs(g, f_out, "layer")
    got = engine.post_rows(torch.as_tensor(h, device=DEV), f_out, norm="layer", gamma=torch.as_tensor(v["gamma"]),
                           beta=torch.as_tensor(v["beta"])).cpu().numpy()
    for r in (0, 17, 36):
        assert (got[r, :f_out] == v["beta"]).all() and (got[r, f_out:] == 0).all()
    assert np.abs(got[1, :f_out] - v["beta"]).max() > 1e-3
    got = engine.post_rows(torch.as_tensor(h, device=DEV), f_out, norm="layer").cpu().numpy()
    assert (got[[0, 17, 36]] == 0).all() and (got[:, f_out:] == 0).all()
    ref = block_ref.post_rows(h, f_out, norm="layer")
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=2e-5)


def test_post_rows_rejects_bad_arguments():
    from bikg_graph_explainability_public_amd import engine
    h = torch.zeros((6, 32), device=DEV)
    with pytest.raises(RuntimeError, match="finite eps > 0"):
        engine.post_rows(h, 5, norm="layer", eps=0.0)
    with pytest.raises(RuntimeError, match="f_out <= ld"):
        engine.post_rows(h, 33)
    with pytest.raises(ValueError, match="tgt_prev must index"):
        engine.post_rows(h, 5, hprev=torch.zeros((2, 3, 32), device=DEV),
                         tgt_prev=torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="ld_prev >= ld"):
        engine.post_rows(h, 5, hprev=torch.zeros((2, 3, 16), device=DEV),
                         tgt_prev=torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ plans
def _plan(c, queries=QUERIES):
    from bikg_graph_explainability_public_amd import pipeline
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # "generic torch path" would be a refusal
        plan = pipeline.build_plan(copy.deepcopy(c["arch"]).to(DEV), c["x"].to(DEV),
                                   torch.as_tensor(c["ei"], device=DEV), queries, attention=True)
    assert plan is not None
    return plan


LN0, LN1, AFF0 = "k_post<layer,0>", "k_post<layer,1>", "k_post<none,0>"
DESCRIBE = {
    "sage_ln_res": f"unfused post1={LN0} post2={LN1} post3={LN1}",
    "gcn_ln": f"unfused post1={LN0} post2={LN0}",
    "sagemax_bn": None, "gin_bn": None,  # folded: no post records, the plan's usual path
    "gat_bn": f"unfused post1={AFF0} post2={AFF0}",
    "gatv2_bn": f"unfused post1={AFF0} post2={AFF0}",
    "gat_ln_res": f"unfused post1={LN0} post2={LN1}",
    "gatv2_ln_res": f"unfused post1={LN0} post2={LN1}",
    "nohead": f"unfused post1={LN0} post2={LN1} post3={LN1}",
    "identity": f"unfused post1={LN0} post2={LN1} post3={LN1}",
}


def _bar(c):
    if c["name"] not in block_ref.IDENTITY_OUT:
        return 1e-5
    y32 = block_ref.module_outputs(c["arch"], c["x"].numpy(), c["ei"], c["masks"], torch.float32)
    e32 = float(np.abs((y32 if c["pooled"] else y32[:, QUERIES]) - c["ref"]).max())
    print("e32 =", e32, "output range", float(c["ref"].min()), float(c["ref"].max()))
    return max(1e-5, 4 * e32)


@pytest.mark.parametrize("name", block_ref.PLAN_CASES)
def test_plans_vs_fp64_union_graph(name):
    """sage LN + skip (3 blocks), gcn LN, sage-max BN (folded, a negative gamma after the max), gin
    BN (folded MLP), gat / gatv2 with BN (post affine) and with LN + skip, a model that ends in a
    post-op layer (no head: the output is that layer's column 0), an identity final activation."""
    c = block_ref.case(name)
    plan = _plan(c)
    want = DESCRIBE[name]
    if want is None:
        assert plan._post is None and not plan.program.has_post
        assert " post" not in plan.describe(64)
    else:
        assert plan.describe(64) == want
    if name == "nohead":
        assert plan.desc.n_head == 0
    _check(plan.forward(_pack(c["masks"])), c["ref"], _bar(c))


@pytest.mark.parametrize("name", block_ref.POOLED_CASES)
def test_pooled_models(name):
    """The readout follows the last layer's post-op (pooled sage LN + skip) or the folded GIN MLP."""
    c = block_ref.case(name)
    plan = _plan(c, [0])
    assert plan.pool == "mean" and plan.n_out == 1
    d = plan.describe(64)
    assert d == ("unfused" if name == "pooled_gin_bn" else f"unfused post1={LN0} post2={LN1}")
    _check(plan.forward(_pack(c["masks"]))[:, 0], c["ref"], _bar(c))


# ------------------------------------------------------------------ paths
@pytest.mark.parametrize("path", ["rows", "fused", "unfused"])
@pytest.mark.parametrize("name", block_ref.PATH_CASES)
def test_folded_batchnorm_keeps_every_path(name, path, monkeypatch):
    """A BN-folded 2-block gcn / sage model is an ordinary program: the rows and the fused kernels
    take it (forced, strict) and match the reference.  Query 7 alone: both kernels hold the plan's
    tables in LDS, and the receptive field of query 0 (the 300-in-edge hub) does not fit there,
    with or without a norm layer."""
    c = block_ref.case(name)
    plan = _plan(c, [7])
    assert plan._post is None
    monkeypatch.setenv("XPG_FORWARD", path)
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    assert plan.describe(64) == path
    _check(plan.forward(_pack(c["masks"])), c["full"][:, [7]])


def test_post_plans_refuse_forced_paths(monkeypatch):
    c = block_ref.case("sage_ln_res")
    plan = _plan(c)
    bits = _pack(c["masks"])
    y = plan.forward(bits)
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    assert plan.describe(64).startswith("unfused post1=")
    assert torch.equal(plan.forward(bits), y)
    for path in ("rows", "fused", "wide"):
        monkeypatch.setenv("XPG_FORWARD", path)
        with pytest.raises(RuntimeError, match="does not take this plan"):
            plan.describe(64)
        out = torch.full_like(y, -7.0)
        with pytest.raises(RuntimeError, match="does not take this plan"):
            plan.forward(bits, out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())  # no output produced
    monkeypatch.delenv("XPG_FORWARD_STRICT")
    monkeypatch.setenv("XPG_FORWARD", "rows")  # not strict: the multi-kernel path, same bits
    assert torch.equal(plan.forward(bits), y)


# ------------------------------------------------------------------ bitwise properties
def _ws_fill(ws, fill):
    if fill == "zero":
        ws.zero_()
    elif fill == "ff":
        ws.fill_(0xFF)
    else:
        ws.random_(0, 256, generator=torch.Generator(device=DEV).manual_seed(5))


@pytest.mark.parametrize("name", ["sage_ln_res", "gat_ln_res", "pooled_sage_ln_res"])
def test_outputs_independent_of_workspace_rows_and_chunks(name):
    """Bitwise identical outputs over caller workspaces pre-filled with zero bytes, 0xFF bytes
    (NaNs) and random bytes; forward(bits[:35]) || forward(bits[35:]) == forward(bits); a
    max_ws_bytes that forces 16-row chunks gives the same bits; two calls are equal."""
    c = block_ref.case(name)
    plan = _plan(c, [0] if c["pooled"] else QUERIES)
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


# ------------------------------------------------------------------ Explainer.run
def _explainer(kind, params=None, pathways=False):
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import BlockStack, PooledModel
    n = 60
    g = np.random.default_rng(1)
    ei = torch.as_tensor(g.integers(0, n, (2, 240)), dtype=torch.long)
    feat = torch.randn((n, 12), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    base = {"seed": 1, "interpret_samples": 10, "epochs": 8, "optimizer": "adam", "lr": 0.01,
            "lr_patience": 10, "l1_lambda": 1e-4, "verify_arch": True}
    names = [str(i) for i in range(n)]
    if kind == "node":
        arch = BlockStack("sage", [12, 8, 8, 8], [8, 1], norm="layer", residual=True)
        problem = "node_prediction"
    else:
        arch = PooledModel(BlockStack("gin", [12, 8, 8], [8], norm="batch"), "add", [8, 1])
        with torch.no_grad():
            arch.fc[0].weight.mul_(1.0 / n)  # a sum over 60 nodes, kept off the sigmoid's tails
        problem = "graph_prediction"
    arch = block_ref.randomise_norms(arch.eval(), 9)
    pw = [list(range(0, 8)), list(range(6, 20)), list(range(30, 45))] if pathways else None
    exp = Explainer(feat, ei, arch, dict(base, **(params or {})), names, pw,
                    ["a", "b", "c"] if pathways else None, None, problem=problem)
    return exp, str(int(np.bincount(ei[1].numpy(), minlength=n).argmax()))  # the busiest target


@pytest.mark.parametrize("kind,sampler,pathways", [("node", "compat", True), ("node", "device", False),
                                                   ("graph", "compat", True)])
def test_explainer_run_matches_the_generic_path(kind, sampler, pathways, monkeypatch):
    """Explainer.run, times=2, verify_arch on: the block models run on the engine without the
    "generic torch path" warning, with the arch check `verified`, and agree with a run forced onto
    the generic path (y within 1e-5 per row, both DataFrames within 1e-4)."""
    from bikg_graph_explainability_public_amd import pipeline
    params = {"mask_sampler": sampler}
    exp, el = _explainer(kind, params, pathways)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df, pdf = exp.run(el, 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified"
    if kind == "node":
        assert lr["plan"].describe(8).startswith("unfused post1=k_post<layer,0> post2=k_post<layer,1>")
    else:
        assert lr["plan"].pool == "sum" and lr["plan"]._post is None
    y = torch.stack([lr["repeats"][i]["y"].reshape(-1) for i in range(2)])
    assert float(y.std()) > 1e-4  # the masks move the output
    exp2, _ = _explainer(kind, params, pathways)
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
