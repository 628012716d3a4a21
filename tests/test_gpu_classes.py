"""GPU parity of multi-class explanations (k_class_out; xpgnn.h, xpg_class_out) against the fp64
restatement of tests/class_ref.py: the readout on its own (xpg_class_out_rows), plans of every
model family ending in softmax / log_softmax on the hub graph of tests/pool_ref.py (S = 400, 64
mask rows, the all-off and the all-on row among them), a non-zero out_col on the rows / fused /
multi-kernel / wide paths, and Explainer.run(target_class) / run_classes.  Bars, the project's
existing ones: bounded outputs (softmax) atol 1e-5 against fp64; unbounded ones (log_softmax)
max(1e-5, 4 x e32), e32 = float32 CPU torch against fp64 on the same inputs; DataFrames and fitted
weights atol 1e-4.  Every plan test first asserts the path it measures (ForwardPlan.describe)."""
import copy
import functools
import os
import socket
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch

import class_ref as cr
import pool_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = cr.ROWS
ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS", "XPG_AGG_GENERIC", "XPG_WIDE_B3")
NAN = float("nan")


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


# ------------------------------------------------------------------ the readout on its own
CS = [1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 129, 255, 256]
MS = [1, 3, 63, 64, 65, 70, 257]


def _rows(M, C, shift=0):
    """z [M, ld] float32, ld = C rounded up to 32, padding 1e30.  Row i has content (i + shift) % 6:
    0 normal(0, 3); 1 all-equal; 2 a +80 / -80 spread; 3 normal(0, 3) + 1e4; 4 its maximum in the
    last real column; 5 its maximum in the first column of the last float4 chunk."""
    ld = (C + 31) // 32 * 32
    g = np.random.default_rng(1000 * C + M)
    z = g.normal(0.0, 3.0, (M, ld)).astype(np.float32)
    for i in range(M):
        k = (i + shift) % 6
        if k == 1:
            z[i] = np.float32(g.normal(0.0, 3.0))
        elif k == 2:
            z[i] = np.where(g.random(ld) < 0.5, 80.0, -80.0)
            z[i, 0], z[i, C - 1] = 80.0, (-80.0 if C > 1 else 80.0)
        elif k == 3:
            z[i] += np.float32(1e4)
        elif k == 4:
            z[i, C - 1] = 40.0
        elif k == 5:
            z[i, 4 * ((C - 1) // 4)] = 40.0
    z[:, C:] = 1e30
    return z


def _out(shape):
    """An output buffer pre-filled with 0xFF bytes (every float a NaN)."""
    return torch.full((4 * int(np.prod(shape)),), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32) \
        .reshape(shape)


def _run(z, C, kind, col):
    e = _eng()
    zt = torch.as_tensor(z, device=DEV)
    M = z.shape[0]
    out = _out((M,) if col >= 0 else (M, C))
    assert bool(torch.isnan(out).all())
    got = e.class_out_rows(zt, C, kind, col, out=out)
    assert got is out
    return out.cpu().numpy()


MEASURED = {"softmax": 0.0, "sum": 0.0, "log_softmax": 0.0, "e32": 0.0}


@pytest.mark.parametrize("C", CS)
def test_class_out_rows(C):
    """Every M of the list for one C: none / all is bitwise the real columns, none / one bitwise the
    picked column (what k_take_col writes), C = 1 gives exactly 1.0 and 0.0, softmax within 1e-5 of
    fp64 with rows summing to 1 within C * 2^-23, log_softmax within max(1e-5, 4 * e32), two calls
    and the one-class / all-class outputs bitwise equal.  Measured maxima on an MI355X over every C
    and M: |softmax - fp64| 2.3e-7, |row sum - 1| 2.5e-7 (the tightest bar, C = 2: 2.4e-7 with 8.6e-8
    measured), |log_softmax - fp64| 8.0e-6 with e32 = 7.7e-6 (the +80 / -80 rows: one float32 ulp of
    160 is 1.5e-5)."""
    cols = sorted({0, C - 1, C // 2, 4 * ((C - 1) // 4)})
    for M in MS:
        for shift in (range(6) if M < 6 else (0,)):
            z = _rows(M, C, shift)
            z64 = z.astype(np.float64)
            all_none = _run(z, C, None, -1)
            assert all_none.shape == (M, C) and np.array_equal(all_none.view(np.uint32), z[:, :C].view(np.uint32))
            outs = {}
            for kind in (None, "softmax", "log_softmax"):
                a = _run(z, C, kind, -1)
                assert not np.isnan(a).any()
                assert np.array_equal(a, _run(z, C, kind, -1))           # two calls
                for c in cols:
                    one = _run(z, C, kind, c)
                    assert one.shape == (M,) and np.array_equal(one.view(np.uint32), a[:, c].view(np.uint32))
                outs[kind] = a
            for c in cols:
                assert np.array_equal(_run(z, C, None, c).view(np.uint32), z[:, c].view(np.uint32))
            ref_s, ref_l = cr.class_out(z64, "softmax", C), cr.class_out(z64, "log_softmax", C)
            if C == 1:
                assert (outs["softmax"] == 1.0).all() and (outs["log_softmax"] == 0.0).all()
                assert not np.signbit(outs["log_softmax"]).any()
            err_s = float(np.abs(outs["softmax"] - ref_s).max())
            err_sum = float(np.abs(outs["softmax"].astype(np.float64).sum(1) - 1.0).max())
            e32 = float(np.abs(torch.log_softmax(torch.as_tensor(z[:, :C]), -1).double().numpy() - ref_l).max())
            err_l = float(np.abs(outs["log_softmax"] - ref_l).max())
            for k, v in (("softmax", err_s), ("sum", err_sum), ("log_softmax", err_l), ("e32", e32)):
                MEASURED[k] = max(MEASURED[k], v)
            assert err_s <= 1e-5, (M, shift, err_s)
            assert err_sum <= C * 2.0 ** -23, (M, shift, err_sum)
            assert err_l <= max(1e-5, 4 * e32), (M, shift, err_l, e32)
    print(f"C = {C}: running maxima {MEASURED}")


@pytest.mark.parametrize("C", [3, 33, 129, 256])
def test_a_row_does_not_depend_on_its_launch(C):
    """Row r of an M = 257 launch is bitwise the same row launched alone, and as row 0 of a
    5-row launch (another lane group of another wave)."""
    z = _rows(257, C)
    for kind in ("softmax", "log_softmax"):
        big = _run(z, C, kind, -1)
        for r in (0, 1, 63, 64, 200, 255, 256):
            assert np.array_equal(_run(z[r:r + 1].copy(), C, kind, -1)[0], big[r])
            five = np.concatenate([z[r:r + 1], z[:4]])
            assert np.array_equal(_run(five, C, kind, -1)[0], big[r])


# ------------------------------------------------------------------ plans against fp64
def _plan(c, **kw):
    from bikg_graph_explainability_public_amd import pipeline
    ekw = {}
    if c["w"] is not None:
        ekw["edge_weight"] = torch.as_tensor(c["w"], dtype=torch.float32, device=DEV)
    if c["ea"] is not None:
        ekw["edge_attr"] = torch.as_tensor(c["ea"], dtype=torch.float32, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a generic-path warning fails the test
        plan = pipeline.build_plan(copy.deepcopy(c["arch"]).to(DEV), c["x"].to(DEV),
                                   torch.as_tensor(c["ei"], device=DEV), c["queries"],
                                   attention=c["name"] == "gatv2", **ekw, **kw)
    assert plan is not None
    return plan


def _bar(c):
    """1e-5 for softmax; max(1e-5, 4 x e32) for log_softmax, e32 = the module's own float32 CPU
    forward on the union graph against the restatement."""
    if c["kind"] == "softmax":
        return 1e-5, 0.0
    got = cr.module_outputs(c["name"], c["arch"], c["x"].numpy(), c["ei"], c["masks"], c["w"], c["ea"])
    e32 = float(np.abs(got - c["ref"]).max())
    return max(1e-5, 4 * e32), e32


@pytest.mark.parametrize("C", cr.CLASSES)
@pytest.mark.parametrize("name", cr.NAMES)
def test_plans_vs_fp64(name, C):
    """Both readouts of one (family, C): one class (the middle one) and all classes against the
    restatement, the all-class output in (query, class) order, the one-class output bitwise its
    column.  Measured on an MI355X over the 54 cases: softmax max |engine - fp64| 4.0e-9 ... 2.7e-7;
    log_softmax 9.9e-8 ... 1.8e-6 with e32 = 1.1e-7 ... 2.3e-6, so every bar is 1e-5."""
    for kind in cr.KINDS:
        c = cr.case(name, C, kind)
        Q, k = len(c["queries"]), c["c"]
        bar, e32 = _bar(c)
        bits = _pack(c["masks"])
        one, every = _plan(c, out_col=k), _plan(c, classes="all")
        assert one.out_norm == every.out_norm == kind and every.n_classes == C
        d1, da = one.describe(ROWS), every.describe(ROWS)
        assert d1.startswith("unfused") and d1.endswith(f" class=k_class_out<{kind},one>")
        assert da.startswith("unfused") and da.endswith(f" class=k_class_out<{kind},all>")
        tag = {"gine": "efeat=k_agg_e", "gcn-weighted": "weights=k_degree_w+k_agg_w", "block-layer": "post1=k_post<layer,0>"}
        assert tag.get(name, "") in da
        ya = every.forward(bits)
        assert tuple(ya.shape) == (ROWS, Q * C) and every.n_out == Q * C and every.n_targets == Q
        ya = ya.cpu().numpy().reshape(ROWS, Q, C)
        y1 = one.forward(bits)
        assert tuple(y1.shape) == (ROWS, Q)
        y1 = y1.cpu().numpy()
        assert np.isfinite(ya).all()
        err_a, err_1 = float(np.abs(ya - c["ref"]).max()), float(np.abs(y1 - c["ref"][..., k]).max())
        print(f"{name} C={C} {kind}: all {err_a:.3g} one {err_1:.3g} bar {bar:.3g} e32 {e32:.3g}")
        assert err_a <= bar and err_1 <= bar
        assert np.array_equal(y1, ya[..., k])
        assert float(np.abs(ya[..., k] - ya[..., 0]).max()) > 1e-3  # another class, another answer


def test_none_kind_is_the_plain_out_col(monkeypatch):
    """cls = {NONE, c} against the plain entry's out_col = c on the multi-kernel path: bitwise where
    the plain tail is k_take_col (a headless plan); where the plain entry computes the column in
    k_dense's HEAD epilogue (a head after a dense layer) the two sum in another order and agree to
    float32 rounding.  classes="all" without a softmax returns the real columns."""
    from bikg_graph_explainability_public_amd import _lib
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    for name in ("headless", "gcn"):
        c = dict(cr.case(name, 7, "softmax"))
        arch = copy.deepcopy(c["arch"])
        if name == "headless":
            arch.out = torch.nn.Identity()
        else:
            arch.fc[-1] = torch.nn.Identity()
        c["arch"] = arch
        bits = _pack(c["masks"])
        every = _plan(c, classes="all")
        assert every.out_norm is None and every.describe(ROWS) == "unfused class=k_class_out<none,all>"
        ya = every.forward(bits).reshape(ROWS, 3, 7)
        for col in (0, 3, 6):
            plain = _plan(c, out_col=col)
            assert plain._cls is None and plain.describe(ROWS) == "unfused"
            y = plain.forward(bits)
            if name == "headless":  # the same rows, picked by k_take_col
                assert torch.equal(y, ya[..., col])
            else:  # the HEAD epilogue sums in another order than the padded head tile
                print("head: max |HEAD epilogue - class readout| =", float((y - ya[..., col]).abs().max()))
                torch.testing.assert_close(y, ya[..., col], rtol=0, atol=1e-5)
            one = _plan(c, out_col=col)
            one._cls = _lib.ClassOut(kind=0, col=col)  # the C-ABI's {NONE, c}
            assert one.describe(ROWS) == "unfused class=k_class_out<none,one>"
            assert torch.equal(one.forward(bits), ya[..., col])
            if name == "headless":
                assert torch.equal(one.forward(bits), y)


def test_forced_rows_path_is_refused_under_strict(monkeypatch):
    c = cr.case("gcn", 7, "softmax")
    plan = _plan(c, classes="all")
    bits = _pack(c["masks"])
    y = plan.forward(bits)
    for forced in ("rows", "fused", "wide"):
        monkeypatch.setenv("XPG_FORWARD", forced)
        monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
        with pytest.raises(RuntimeError, match="forced XPG_FORWARD path"):
            plan.describe(ROWS)
        with pytest.raises(RuntimeError, match="forced XPG_FORWARD path"):
            plan.forward(bits)
        monkeypatch.delenv("XPG_FORWARD_STRICT")
        assert plan.describe(ROWS) == "unfused class=k_class_out<softmax,all>"
        assert torch.equal(plan.forward(bits), y)  # not strict: the multi-kernel path, same result


@pytest.mark.parametrize("name", ["gcn", "pooled-mean"])
def test_outputs_do_not_depend_on_workspace_or_chunks(name):
    c = cr.case(name, 33, "log_softmax")
    plan = _plan(c, classes="all")
    bits = _pack(c["masks"])
    nb = plan.workspace_bytes(ROWS)
    outs = []
    for fill in (0x00, 0xFF):  # 0xFF: every float of the workspace a NaN
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        out = torch.full((ROWS, plan.n_out), NAN, dtype=torch.float32, device=DEV)
        plan.forward(bits, out=out, workspace=ws)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    y = plan.forward(bits)
    assert torch.equal(y, outs[0])
    assert torch.equal(torch.cat([plan.forward(bits[:32]), plan.forward(bits[32:])]), y)
    for rows in (1, 33):
        assert torch.equal(plan.forward(bits[:rows]), y[:rows])
    small = plan.workspace_bytes(16)
    assert small < nb
    plan._ws = None
    assert torch.equal(plan.forward(bits, max_ws_bytes=small), y)


def test_plan_refusals():
    """A class outside [0, C) is an error of the request (no path could return it); edge-mask and
    link plans take no class readout."""
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.program import compile_arch
    c = cr.case("gcn", 7, "softmax")
    with pytest.raises(ValueError, match=r"target class 7 outside \[0, 7\)"):
        _plan(c, out_col=7)
    e = _eng()
    prog = compile_arch(c["arch"])
    eit = torch.as_tensor(c["ei"], device=DEV)
    cols = torch.arange(eit.shape[1])
    with pytest.raises(ValueError, match="class readout"):
        e.ForwardPlan(prog, c["x"].to(DEV), [eit], [0], edge_cols=[cols])
    with pytest.raises(ValueError, match="classes must be"):
        e.ForwardPlan(prog, c["x"].to(DEV), [eit], [0], classes="some")


# ------------------------------------------------------------------ out_col on every path
@functools.lru_cache(maxsize=None)
def _col_case(S, kind, dims, fc, all_targets):
    """ConvStack(kind, dims, fc) with a sigmoid head of fc[-1] = 5 columns (no head: dims[-1]
    columns after the last ReLU) on a random graph with self-loops and duplicate edges; the fp64
    columns [rows, targets, C] from the restatement."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    g = torch.Generator().manual_seed(S)
    x = torch.randn((S, dims[0]), generator=g)
    ei = torch.randint(0, S, (2, 6 * S), generator=g)
    ei[:, :10] = ei[0, :10]
    ei[:, 10:20] = ei[:, 20:30]
    ei = ei.numpy().astype(np.int64)
    torch.manual_seed(S + 1)
    arch = ConvStack(kind, list(dims), list(fc)).eval()
    rows = 40
    masks = pool_ref.row_masks(rows, S, 5)
    name = "gcn" if kind == "gcn" else "sage-max"  # the restatement that knows the conv
    h = cr.encoder_rows(name, arch, x.numpy(), ei, masks)
    z, _ = cr.head_rows(arch.fc, h)
    ref = z.reshape(rows, S, -1)
    queries = list(range(S)) if all_targets else [3, 17, S - 1]
    return {"x": x, "ei": ei, "arch": arch, "masks": masks, "ref": ref, "queries": queries}


@pytest.mark.parametrize("path,S,kind,dims,fc,all_targets", [
    ("rows", 60, "gcn", (12, 32, 32), (32, 5), False),
    ("rows", 60, "gcn", (12, 32, 32), (32,), False),
    ("fused", 60, "gcn", (12, 32, 32), (32, 5), False),
    ("fused", 60, "sage", (12, 32, 32), (32, 8, 5), False),
    ("unfused", 60, "gcn", (12, 32, 32), (32, 5), False),
    ("unfused", 60, "gcn", (12, 32, 32), (32,), False),
    ("wide", 2500, "sage", (16, 64, 64), (64, 5), True),
    ("wide", 2500, "sage", (16, 64, 64), (64,), True),
])
def test_out_col_on_every_path(path, S, kind, dims, fc, all_targets, monkeypatch):
    """The rows, fused and wide kernels read out_col, which had only ever been 0: the last and a
    middle column (and column 0) on each path, the path forced under strict and asserted through
    describe, against the fp64 restatement within 1e-5 (sigmoid heads; the headless outputs are
    the last conv's ReLU rows, same bar)."""
    from bikg_graph_explainability_public_amd import pipeline
    c = _col_case(S, kind, dims, fc, all_targets)
    C = c["ref"].shape[-1]
    monkeypatch.setenv("XPG_FORWARD", path)
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    bits = _pack(c["masks"])
    seen = []
    for col in (C - 1, C // 2, 0):
        plan = pipeline.build_plan(copy.deepcopy(c["arch"]).to(DEV), c["x"].to(DEV),
                                   torch.as_tensor(c["ei"], device=DEV), c["queries"], out_col=col)
        assert plan is not None and plan.describe(40).split()[0] == path
        got = plan.forward(bits).cpu().numpy()
        pos = [int(n) for n in plan.frontiers[-1]]  # output column i is node pos[i]
        ref = c["ref"][:, pos, col]
        err = float(np.abs(got - ref).max())
        print(f"{path} {kind} {fc} col {col}: max |engine - fp64| = {err:.3g}, |ref| max {np.abs(ref).max():.3g}")
        assert err <= 1e-5
        seen.append(got)
    assert np.abs(seen[0] - seen[2]).max() > 1e-3 and np.abs(seen[1] - seen[2]).max() > 1e-3


# ------------------------------------------------------------------ the generic path's columns
def test_generic_outputs_columns():
    """generic_outputs(out_col=c) / classes="all" read the module's own output: against the
    restatement for a node-level and a pooled model, one query and a query list."""
    from bikg_graph_explainability_public_amd import pipeline
    c = cr.case("gcn", 7, "softmax")
    arch = copy.deepcopy(c["arch"]).to(DEV)
    x, eit = c["x"].to(DEV), torch.as_tensor(c["ei"], device=DEV)
    mt = torch.as_tensor(c["masks"][:8], device=DEV)
    ref = c["ref"][:8]
    y = pipeline.generic_outputs(arch, x, eit, mt, 7, "node_prediction", out_col=3)
    np.testing.assert_allclose(y.cpu().numpy(), ref[:, 1, 3], rtol=0, atol=1e-5)
    ya = pipeline.generic_outputs(arch, x, eit, mt, 7, "node_prediction", classes="all")
    np.testing.assert_allclose(ya.cpu().numpy(), ref[:, 1], rtol=0, atol=1e-5)
    yq = pipeline.generic_outputs(arch, x, eit, mt, cr.QUERIES, "node_prediction", classes="all", batch=3)
    np.testing.assert_allclose(yq.cpu().numpy().reshape(8, 3, 7), ref, rtol=0, atol=1e-5)
    y1 = pipeline.generic_outputs(arch, x, eit, mt, cr.QUERIES, "node_prediction", out_col=6)
    np.testing.assert_allclose(y1.cpu().numpy(), ref[..., 6], rtol=0, atol=1e-5)
    with pytest.raises(ValueError, match=r"target class 7 outside \[0, 7\)"):
        pipeline.generic_outputs(arch, x, eit, mt, 7, "node_prediction", out_col=7)
    p = cr.case("pooled-mean", 7, "log_softmax")
    yp = pipeline.generic_outputs(copy.deepcopy(p["arch"]).to(DEV), x, eit, mt, 0, "graph_prediction",
                                  classes="all", batch=5)
    np.testing.assert_allclose(yp.cpu().numpy(), p["ref"][:8, 0], rtol=0, atol=1e-5)
    yp = pipeline.generic_outputs(copy.deepcopy(p["arch"]).to(DEV), x, eit, mt, 0, "graph_prediction", out_col=2)
    np.testing.assert_allclose(yp.cpu().numpy(), p["ref"][:8, 0, 2], rtol=0, atol=1e-5)


# ------------------------------------------------------------------ Explainer
BASE = {"seed": 1, "interpret_samples": 10, "epochs": 8, "optimizer": "adam", "lr": 0.01,
        "lr_patience": 10, "l1_lambda": 1e-4, "verify_arch": True}


class FunctionalLogSoftmax(torch.nn.Module):
    """A classifier whose log_softmax is a function call of its forward: no unit to lower."""

    def __init__(self, f, C):
        super().__init__()
        from bikg_graph_explainability_public_amd import nn as xnn
        self.conv = torch.nn.ModuleList([xnn.GCNConv(f, 8), torch.nn.ReLU()])
        self.fc = torch.nn.ModuleList([xnn.Linear(8, C)])

    def forward(self, x, edge_index):
        x = self.conv[1](self.conv[0](x, edge_index))
        return torch.nn.functional.log_softmax(self.fc[0](x), dim=-1)


def _explainer(kind, params=None, C=3):
    """node: ConvStack("gcn", [12, 8, 8], [8, C], softmax) under node_prediction on 60 nodes;
    pooled: PooledModel(ConvStack("gcn"), "mean", [8, C], log_softmax) under graph_prediction on 30
    nodes (a graph classifier); functional: FunctionalLogSoftmax under node_prediction."""
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack, PooledModel
    S = 30 if kind == "pooled" else 60
    g = np.random.default_rng(1)
    ei = g.integers(0, S, (2, 4 * S))
    q = int(ei[1, 0])
    feat = torch.randn((S, 12), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    if kind == "pooled":
        arch = PooledModel(ConvStack("gcn", [12, 8, 8], [8]), "mean", [8, C], final_act="log_softmax").eval()
        problem = "graph_prediction"
    elif kind == "functional":
        arch, problem = FunctionalLogSoftmax(12, C).eval(), "node_prediction"
    else:
        arch, problem = ConvStack("gcn", [12, 8, 8], [8, C], final_act="softmax").eval(), "node_prediction"
    with torch.no_grad():  # logits that tell the classes apart
        for m in arch.fc:
            if hasattr(m, "weight"):
                m.weight.mul_(4.0)
    exp = Explainer(feat, torch.as_tensor(ei, dtype=torch.long), arch, dict(BASE, **(params or {})),
                    [str(i) for i in range(S)], None, None, None, problem=problem)
    return exp, str(q)


def _ys(exp, times):
    return torch.stack([exp.last_run["repeats"][i]["y"].reshape(-1) for i in range(times)])


def _same(df_a, df_b, atol=1e-4):
    np.testing.assert_allclose(df_a.loc[df_b.index].values, df_b.values, rtol=0, atol=atol)


@pytest.mark.parametrize("kind,sampler", [("node", "compat"), ("node", "device"), ("pooled", "compat")])
def test_run_with_target_class_matches_the_generic_path(kind, sampler, monkeypatch):
    """Explainer.run with target_class = 2, times = 2: on the engine without a generic-path warning,
    arch check `verified`, agreeing with the run forced onto the generic path (y 1e-5, DataFrames
    1e-4) and differing from the target_class = 0 run."""
    from bikg_graph_explainability_public_amd import pipeline
    params = {"mask_sampler": sampler, "target_class": 2}
    exp, q = _explainer(kind, params)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        df, _ = exp.run(q, 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified" and lr["target_class"] == 2
    assert " class=k_class_out<" in lr["plan"].describe(16) and lr["plan"].out_col == 2
    y = _ys(exp, 2)
    assert float(y.std()) > 1e-4
    exp0, _ = _explainer(kind, dict(params, target_class=0))
    df0, _ = exp0.run(q, 2)
    assert exp0.last_run["target_class"] == 0 and exp0.last_run["engine"] is True
    assert float((_ys(exp0, 2) - y).abs().max()) > 1e-3
    assert np.abs(df.loc[df0.index].values - df0.values).max() > 1e-4
    exp2, _ = _explainer(kind, params)
    monkeypatch.setattr(pipeline, "build_plan", lambda *a, **k: None)
    df2, _ = exp2.run(q, 2)
    assert exp2.last_run["engine"] is False and exp2.last_run["target_class"] == 2
    torch.testing.assert_close(y, _ys(exp2, 2), rtol=0, atol=1e-5)
    _same(df, df2)


def test_target_class_out_of_range_and_unsupported_problems():
    exp, q = _explainer("node", {"target_class": 3})
    with pytest.raises(ValueError, match=r"target class 3 outside \[0, 3\)"):
        exp.run(q, 1)
    exp, q = _explainer("functional", {"target_class": 3})  # C from the module's own output
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=r"target class 3 outside \[0, 3\)"):
            exp.run(q, 1)
    with pytest.raises(ValueError, match="target_class"):
        _explainer("node", {"target_class": -1})[0].run(q, 1)


def test_changing_target_class_on_a_live_explainer():
    exp, q = _explainer("node", {"target_class": 1})
    df1, _ = exp.run(q, 1)
    exp.params["target_class"] = 2
    df2, _ = exp.run(q, 1)
    assert exp.last_run["query_cache"] == "miss" and exp.last_run["target_class"] == 2
    assert exp.last_run["arch_check"] == "verified"  # every requested class is checked once
    fresh, _ = _explainer("node", {"target_class": 2})
    df2f, _ = fresh.run(q, 1)
    np.testing.assert_array_equal(df2.loc[df2f.index].values, df2f.values)
    assert np.abs(df1.loc[df2.index].values - df2.values).max() > 1e-4
    exp.params["target_class"] = 1
    df1b, _ = exp.run(q, 1)
    assert exp.last_run["query_cache"] == "hit"
    np.testing.assert_array_equal(df1.loc[df1b.index].values, df1b.values)


@pytest.mark.parametrize("kind,sampler", [("node", "compat"), ("node", "device"), ("pooled", "compat")])
def test_run_classes_of_one_class_equals_run(kind, sampler):
    exp, q = _explainer(kind, {"mask_sampler": sampler, "target_class": 1})
    df, _ = exp.run(q, 2)
    y = _ys(exp, 2)
    exp2, _ = _explainer(kind, {"mask_sampler": sampler})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        (dfc, pdf), = exp2.run_classes(q, [1], 2)
    assert not [w for w in caught if "generic torch path" in str(w.message)]
    lr = exp2.last_run
    assert lr["engine"] is True and lr["arch_check"] == "verified" and lr["classes"] == [1] and pdf is None
    assert torch.equal(lr["y"][:, :, 0], y.reshape(2, -1))
    _same(df, dfc)


@pytest.mark.parametrize("kind,batch_bytes", [("node", None), ("node", 1), ("pooled", None)])
def test_run_classes_every_class_vs_standalone(kind, batch_bytes):
    """run_classes over all C = 3 classes (pooled: the graph classifier on 30 nodes): every class's
    column equals a one-class plan's forward on the same masks bitwise, its weights a standalone
    fit with that class's initial weights to 1e-4 (the run_queries rule); batch_bytes = 1 forces the
    one-launch-per-class branch.  The class rows are distributions."""
    from bikg_graph_explainability_public_amd import pipeline
    over = {} if batch_bytes is None else {"run_queries_batch_bytes": batch_bytes}
    exp, q = _explainer(kind, over)
    out = exp.run_classes(q, None, 2)
    lr = exp.last_run
    assert lr["engine"] is True and lr["classes"] == [0, 1, 2] and lr["n_classes"] == 3 and len(out) == 3
    assert lr["plan"].describe(16).endswith(",all>")
    p = lr["y"].double().exp() if kind == "pooled" else lr["y"].double()
    torch.testing.assert_close(p.sum(-1), torch.ones_like(p[..., 0]), rtol=0, atol=1e-5)
    S, batch = lr["S"], lr["batch"]
    ctx = exp.prepare(q, DEV)
    e = _eng()
    for k in range(3):
        plan = pipeline.build_plan(exp.arch, ctx["sub_feat"], ctx["sub_ei"], [ctx["sub_ind"]], out_col=k)
        for i in range(2):
            assert torch.equal(lr["y"][i, :, k], plan.forward(lr["bits"][i])[:, 0])
        w, _, _, _, _ = e.wlm_fit(lr["bits"], S, batch, lr["y"][:, :, k].contiguous(), lr["kernel"],
                                  lr["w0"][k], exp.params)
        torch.testing.assert_close(lr["weights"][k], w, rtol=0, atol=1e-4)
        df = out[k][0]
        np.testing.assert_allclose(df.reindex(ctx["sub_names"])["config_value_mean"].values,
                                   w.mean(0).cpu().numpy(), rtol=0, atol=1e-4)
    assert np.abs(out[0][0].loc[out[2][0].index].values - out[2][0].values).max() > 1e-4
    sub = exp.run_classes(q, [2, 0], 2)  # a subset, in the order asked for
    assert exp.last_run["classes"] == [2, 0] and len(sub) == 2
    for bad in ([3], [-1], [0, 0], [], [1.0]):
        with pytest.raises(ValueError, match="run_classes"):
            exp.run_classes(q, bad, 1)


def test_functional_log_softmax_runs_on_the_generic_path():
    """No Softmax unit to lower: the compiled program disagrees with the module, the run takes the
    generic path with the usual warning and reads the module's own column."""
    from bikg_graph_explainability_public_amd import pipeline
    exp, q = _explainer("functional", {"target_class": 2})
    with pytest.warns(UserWarning, match="generic torch path"):
        df, _ = exp.run(q, 1)
    lr = exp.last_run
    assert lr["engine"] is False and lr["arch_check"] == "failed" and lr["target_class"] == 2
    ctx = exp.prepare(q, DEV)
    rep = lr["repeats"][0]
    mask = _eng().unpack_masks(rep["bits"], lr["S"])
    cols = pipeline.generic_outputs(exp.arch, ctx["sub_feat"], ctx["sub_ei"], mask, ctx["sub_ind"],
                                    "node_prediction", classes="all", batch=rep["batch"])
    torch.testing.assert_close(cols.exp().sum(-1), torch.ones_like(cols[:, 0]), rtol=0, atol=1e-5)
    torch.testing.assert_close(rep["y"].reshape(-1), cols[:, 2], rtol=0, atol=1e-6)
    assert float((cols[:, 2] - cols[:, 0]).abs().max()) > 1e-3
    with pytest.warns(UserWarning, match="generic torch path"):
        out = exp.run_classes(q, None, 1)
    assert exp.last_run["engine"] is False and exp.last_run["n_classes"] == 3 and len(out) == 3
    torch.testing.assert_close(exp.last_run["y"][0], cols, rtol=0, atol=1e-6)
    with pytest.warns(UserWarning, match="generic torch path"):
        (df2, _), = exp.run_classes(q, [2], 1)
    _same(df, df2)


# ------------------------------------------------------------------ two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_run(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_classes as t
        torch.cuda.set_device(0)
        exp, q = t._explainer("node")
        out = exp.run_classes(q, None, 2)
        np.save(os.path.join(out_dir, f"y{rank}.npy"), exp.last_run["y"].cpu().numpy())
        np.save(os.path.join(out_dir, f"w{rank}.npy"),
                np.stack([df.sort_index()[["config_value_mean", "config_value_std"]].values for df, _ in out]))
    finally:
        dist.destroy_process_group()


def test_run_classes_on_two_ranks_matches_one_rank():
    """run_classes over 2 ranks (both on this card, gloo collectives; the harness of
    tests/test_gpu_coverage.py's two-rank Explainer.run): the forward rows and the class x repeat
    fits are sharded; y is bitwise the 1-rank y, the DataFrames within 1e-4."""
    import torch.multiprocessing as mp
    exp, q = _explainer("node")
    out = exp.run_classes(q, None, 2)
    y = exp.last_run["y"].cpu().numpy()
    ref = np.stack([df.sort_index()[["config_value_mean", "config_value_std"]].values for df, _ in out])
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank_run, args=(2, _free_port(), d), nprocs=2, join=True)
        for r in range(2):
            assert np.array_equal(np.load(os.path.join(d, f"y{r}.npy")), y)
            np.testing.assert_allclose(np.load(os.path.join(d, f"w{r}.npy")), ref, rtol=0, atol=1e-4)
