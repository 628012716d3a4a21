"""Multi-class explanations without a GPU: models ending in softmax / log_softmax against the fp64
restatement of tests/class_ref.py, the lowering (program.compile_arch: out_norm), the host side of
the C-ABI's class readout (xpg_class_out, the _c entry points, xpg_class_out_rows: host checks,
describe texts, workspace sizes) on synthetic descriptors whose device pointers are only tested for
NULL, the class selection of the generic path (pipeline.pick_classes; generic_outputs itself needs
the device's edge-keep kernel and is exercised in tests/test_gpu_classes.py), target_class
validation and, last, the non-vacuity conditions of the GPU parity cases, asserted on the reference
alone."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import class_ref as cr
from test_dispatch_cpu import make_plan, describe

from bikg_graph_explainability_public_amd import _lib, nn as xnn, pipeline
from bikg_graph_explainability_public_amd.explainer import Explainer
from bikg_graph_explainability_public_amd.program import ModelProgram, UnsupportedArch, compile_arch

ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS")
SAGE, GCN = ("mean", "root"), ("gcn",)
KIND = {None: 0, "softmax": 1, "log_softmax": 2}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------ module vs the restatement
@pytest.mark.parametrize("out", cr.KINDS)
@pytest.mark.parametrize("name", cr.NAMES)
def test_module_matches_restatement_fp64(name, out):
    """Every model family of the GPU cases in double against class_ref to 1e-12, on the hub graph
    with 6 mask rows (all-off and all-on among them), C = 7."""
    S, x, ei, w, ea, masks = cr._inputs(name)
    masks = masks[:6]
    arch = cr.build(name, 7, out).double()
    h = cr.encoder_rows(name, arch, x.numpy(), ei, masks, w, ea)
    ref = cr.outputs(name, arch, h, masks)
    got = cr.module_outputs(name, arch, x.numpy(), ei, masks, w, ea, dtype=torch.float64)
    assert got.shape == ref.shape == (6, 1 if name == "pooled-mean" else 3, 7)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    p = np.exp(ref) if out == "log_softmax" else ref
    np.testing.assert_allclose(p.sum(-1), 1.0, rtol=0, atol=1e-12)
    assert np.ptp(ref, axis=0).max() > 1e-4  # the masks matter


def test_readout_restatement_basics():
    z = np.array([[1.0, 2.0, 3.0, 1e30], [-80.0, 80.0, 0.0, 1e30]])
    np.testing.assert_array_equal(cr.class_out(z, None, 3), z[:, :3])
    s = cr.class_out(z, "softmax", 3)
    np.testing.assert_allclose(s[0], np.exp(z[0, :3]) / np.exp(z[0, :3]).sum(), rtol=1e-15)
    np.testing.assert_allclose(cr.class_out(z, "log_softmax", 3), np.log(s), rtol=1e-12, atol=1e-300)
    assert cr.class_out(z[:, :1], "softmax").tolist() == [[1.0], [1.0]]
    assert cr.class_out(z[:, :1], "log_softmax").tolist() == [[0.0], [0.0]]


def test_final_act_values_build_what_they_built():
    """sigmoid / anything else build Sigmoid / Identity as before; the two new values the class
    units, over the last dimension; no parameter is added."""
    for cls, kw in ((xnn.ConvStack, {}), (xnn.BlockStack, {"norm": "layer"})):
        for fa, want in (("sigmoid", "Sigmoid"), ("identity", "Identity"), (None, "Identity"),
                         ("softmax", "Softmax"), ("log_softmax", "LogSoftmax")):
            m = cls("gcn", [6, 5, 4], [4, 3], final_act=fa, **kw)
            assert type(m.fc[-1]).__name__ == want and type(m.fc[-2]).__name__ == "Linear"
            assert len(list(m.fc[-1].parameters())) == 0
            assert getattr(m.fc[-1], "dim", -1) == -1
    assert type(xnn.RGCNStack([6, 5], [5, 3], 3, final_act="softmax").fc[-1]).__name__ == "Softmax"
    pm = xnn.PooledModel(xnn.ConvStack("gcn", [6, 5], [5]), "mean", [5, 3], final_act="log_softmax")
    assert type(pm.fc[-1]).__name__ == "LogSoftmax"
    assert type(xnn.ConvStack("gcn", [6, 5], [5, 1]).fc[-1]).__name__ == "Sigmoid"  # the default


# ------------------------------------------------------------------ lowering
@pytest.mark.parametrize("out", cr.KINDS)
def test_compile_sets_out_norm(out):
    torch.manual_seed(1)
    arch = xnn.ConvStack("gcn", [6, 5, 4], [4, 8, 3], final_act=out)
    prog = compile_arch(arch)
    assert prog.out_norm == out and prog.n_classes == 3 and prog.out_col == 0
    assert [h.act for h in prog.head] == ["relu", None]
    assert torch.equal(prog.head[1].weight, arch.fc[2].weight.detach())
    pm = compile_arch(xnn.PooledModel(xnn.ConvStack("gin", [6, 5, 4], [4]), "add", [4, 5], final_act=out))
    assert pm.out_norm == out and pm.pool == "sum" and pm.head[-1].act is None and pm.n_classes == 5
    bs = compile_arch(xnn.BlockStack("gcn", [6, 5, 5], [5, 2], norm="layer", residual=True, final_act=out))
    assert bs.out_norm == out and bs.has_post and bs.n_classes == 2
    hl = compile_arch(cr.HeadlessGCN([6, 5, 4], out))
    assert hl.out_norm == out and not hl.head and hl.convs[-1].act is None and hl.n_classes == 4
    assert hl.convs[0].act == "relu"
    rg = compile_arch(xnn.RGCNStack([6, 5], [5, 3], 3, final_act=out))
    assert rg.out_norm == out and rg.n_classes == 3
    # dim=1 is the class dimension of a [rows, C] output too
    m = xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="identity")
    m.fc[-1] = torch.nn.Softmax(dim=1) if out == "softmax" else torch.nn.LogSoftmax(dim=1)
    assert compile_arch(m).out_norm == out


def test_compile_refusals():
    """A softmax anywhere but last, over another dimension, after an activation, on a link model or
    in the multi-node-type lowering stays UnsupportedArch."""
    m = xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="identity")
    m.fc[-1] = torch.nn.Softmax(dim=0)
    with pytest.raises(UnsupportedArch, match=r"dim=0"):
        compile_arch(m)
    m.fc[-1] = torch.nn.Softmax(dim=None)
    with pytest.raises(UnsupportedArch, match=r"dim=None"):
        compile_arch(m)
    m = xnn.ConvStack("gcn", [6, 5], [5, 4, 3], final_act="softmax")
    m.fc[1] = torch.nn.Softmax(dim=-1)  # between two head layers
    with pytest.raises(UnsupportedArch, match="unexpected module order at Softmax"):
        compile_arch(m)
    m = xnn.ConvStack("gcn", [6, 5, 4], [4, 3], final_act="softmax")
    m.conv[1] = torch.nn.LogSoftmax(dim=-1)  # between two convs
    with pytest.raises(UnsupportedArch, match="unexpected module order at LogSoftmax"):
        compile_arch(m)
    m = xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="sigmoid")
    m.fc.append(torch.nn.Softmax(dim=-1))
    with pytest.raises(UnsupportedArch, match=r"after an activation \(sigmoid\)"):
        compile_arch(m)
    hl = cr.HeadlessGCN([6, 5, 4], "softmax")
    hl.conv.append(torch.nn.ReLU())  # headless: the last conv with an activation of its own
    with pytest.raises(UnsupportedArch, match=r"after an activation \(relu\)"):
        compile_arch(hl)
    enc = xnn.ConvStack("sage", [6, 5], [5, 4], final_act="softmax")
    with pytest.raises(UnsupportedArch, match="LinkModel over an encoder ending in Softmax"):
        compile_arch(xnn.LinkModel(enc))
    with pytest.raises(UnsupportedArch, match="RelLinkModel over an encoder ending in Softmax"):
        compile_arch(xnn.RelLinkModel(xnn.RGCNStack([6, 5], [5, 4], 3, final_act="softmax"), 3))
    with pytest.raises(UnsupportedArch, match="encoder ending in Softmax"):
        compile_arch(xnn.PooledModel(cr.HeadlessGCN([6, 5, 4], "softmax"), "mean", [4, 2]))
    rels = [("a", "r", "b"), ("b", "s", "a")]
    multi = xnn.HeteroSageStack(rels, {"a": 6, "b": 6}, 5, 1, [5, 3])
    multi.fc[-1] = torch.nn.Softmax(dim=-1)
    with pytest.raises(UnsupportedArch, match="multi-node-type"):
        compile_arch(multi, edge_type_names=rels, node_type_names=["a", "b"])


def test_existing_programs_are_unchanged():
    """ModelProgram gained exactly one field, default None; an existing arch lowers to the same
    values in every other field."""
    names = [f.name for f in dataclasses.fields(ModelProgram)]
    assert names == ["convs", "head", "out_col", "n_types", "out_type", "link_act", "link_rel",
                     "extra_layers", "pool", "weighted", "edge_featured", "out_norm"]
    torch.manual_seed(2)
    arch = xnn.ConvStack("sage", [6, 5, 4], [4, 3, 1])
    prog = compile_arch(arch)
    assert (prog.out_col, prog.n_types, prog.out_type, prog.link_act, prog.link_rel, prog.extra_layers,
            prog.pool, prog.weighted, prog.edge_featured, prog.out_norm) == \
        (0, 1, None, None, None, 0, None, False, False, None)
    assert [h.act for h in prog.head] == ["relu", "sigmoid"] and [c.act for c in prog.convs] == ["relu"] * 2
    assert [[t.kind for t in c.terms] for c in prog.convs] == [["mean", "root"]] * 2
    assert torch.equal(prog.convs[1].terms[0].weight, arch.conv[2].lin_l.weight.detach())
    assert torch.equal(prog.head[1].weight, arch.fc[2].weight.detach())
    for other in (xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="identity"),
                  xnn.PooledModel(xnn.ConvStack("gcn", [6, 5], [5]), "max", [5, 1]),
                  xnn.LinkModel(xnn.ConvStack("sage", [6, 5], [5, 4], final_act="identity"))):
        assert compile_arch(other).out_norm is None


def test_program_cache_sees_a_replaced_last_unit():
    """The softmax unit has no parameter: the program cache keys on it separately."""
    pipeline.clear_programs()
    arch = xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="identity")
    assert pipeline.compiled_program(arch).out_norm is None
    arch.fc[-1] = torch.nn.Softmax(dim=-1)
    p1 = pipeline.compiled_program(arch)
    assert p1.out_norm == "softmax" and pipeline.compiled_program(arch) is p1
    arch.fc[-1] = torch.nn.LogSoftmax(dim=-1)
    assert pipeline.compiled_program(arch).out_norm == "log_softmax"
    pipeline.clear_programs()


# ------------------------------------------------------------------ descriptors (host only)
def _cls(kind, col):
    return _lib.ClassOut(kind=KIND.get(kind, kind), col=col)


def _plain(layers, heads=(7,), **kw):
    """make_plan with a last head layer (or, headless, last conv layer) that has no activation."""
    desc = make_plan(layers, heads, **kw)
    if heads:
        desc._keep[1][len(heads) - 1].act = 0
    else:
        desc._keep[0][len(layers) - 1].act = 0
    return desc


def _describe_c(desc, cls, rows=70, post=None):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().xpg_forward_describe_c(ctypes.byref(desc), post, None, None,
                                                  ctypes.byref(cls) if cls is not None else None, rows, buf, 256))
    return buf.value.decode()


def _ws_c(desc, cls, rows=70):
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_forward_workspace_c(ctypes.byref(desc), None, None, None,
                                                   ctypes.byref(cls) if cls is not None else None, rows,
                                                   ctypes.byref(n)))
    return n.value


def _ws_e(desc, rows=70):
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_forward_workspace_e(ctypes.byref(desc), None, None, None, rows, ctypes.byref(n)))
    return n.value


PLANS = [
    ([(GCN, 32), (GCN, 32)], {"n_nodes": 40, "n_tgt": 8}),              # rows kernel
    ([(SAGE, 128), (SAGE, 128)], {"n_nodes": 10000, "n_tgt": 10000}),   # wide path
    ([(SAGE, 128), (SAGE, 128)], {}),                                   # multi-kernel path
]


def test_abi_is_additive():
    assert _lib.ABI_VERSION == 28 and _lib.ForwardPlanDesc._fields_[-1][0] == "dot_scale"
    assert [f[0] for f in _lib.ClassOut._fields_] == ["kind", "col"] and ctypes.sizeof(_lib.ClassOut) == 8
    assert _lib.CLASS_KIND == {None: 0, "softmax": 1, "log_softmax": 2}
    assert {"xpg_forward_workspace_c", "xpg_masked_forward_c", "xpg_forward_describe_c",
            "xpg_class_out_rows"} <= set(_lib.EXPORTED)


@pytest.mark.parametrize("layers,kw", PLANS)
@pytest.mark.parametrize("heads", [(1,), (16, 7), ()])
def test_null_class_is_the_e_entry_point(layers, kw, heads, monkeypatch):
    """cls == NULL: describe text and workspace of the _c entry points are those of _e (and of the
    plain entry points) on every path, default and forced."""
    for forced in (None, "rows", "fused", "unfused", "wide"):
        if forced:
            monkeypatch.setenv("XPG_FORWARD", forced)
        desc = make_plan(layers, heads, **kw)
        assert _describe_c(desc, None) == describe(desc)
        for rows in (1, 70):
            assert _ws_c(desc, None, rows) == _ws_e(desc, rows)
    monkeypatch.delenv("XPG_FORWARD")
    paths = {describe(make_plan(l, (1,), **k)).split()[0] for l, k in PLANS}
    assert paths == {"rows", "wide", "unfused"}  # the three plans do take three paths


@pytest.mark.parametrize("layers,kw", PLANS)
def test_class_plans_take_the_multi_kernel_path(layers, kw, monkeypatch):
    """With cls: `unfused class=k_class_out<kind,one|all>` whatever path the plain plan takes, the
    workspace of the same plan forced onto the multi-kernel path, and a forced rows / fused / wide
    path refused under strict by describe and forward alike."""
    for heads in ((7,), (16, 33), ()):
        desc = _plain(layers, heads, **kw)
        for kind in (None, "softmax", "log_softmax"):
            for col, tag in ((0, "one"), (-1, "all")):
                assert _describe_c(desc, _cls(kind, col)) == f"unfused class=k_class_out<{kind or 'none'},{tag}>"
        monkeypatch.setenv("XPG_FORWARD", "unfused")
        want = {rows: _ws_e(desc, rows) for rows in (1, 70)}
        monkeypatch.delenv("XPG_FORWARD")
        for rows in (1, 70):
            assert _ws_c(desc, _cls("softmax", -1), rows) == _ws_c(desc, _cls(None, 2), rows) == want[rows]
    desc = _plain(layers, (7,), **kw)
    lib = _lib.load()
    cls = _cls("softmax", -1)
    for forced in ("rows", "fused", "wide"):
        monkeypatch.setenv("XPG_FORWARD", forced)
        monkeypatch.delenv("XPG_FORWARD_STRICT", raising=False)
        assert _describe_c(desc, cls) == "unfused class=k_class_out<softmax,all>"
        monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
        with pytest.raises(RuntimeError, match="forced XPG_FORWARD path does not take this plan"):
            _describe_c(desc, cls)
        rc = lib.xpg_masked_forward_c(ctypes.byref(desc), None, None, None, ctypes.byref(cls), None, 70, None,
                                      None, 1 << 40, None)
        assert rc == 1 and b"does not take this plan" in lib.xpg_last_error()


def test_class_token_follows_the_post_tokens():
    layers = [(SAGE, 64), (SAGE, 64)]
    desc = _plain(layers, (7,))
    desc._keep[0][1].act = 0
    post = (_lib.PostDesc * 2)()
    post[1].norm, post[1].eps, post[1].act = 1, 1e-5, 1
    assert _describe_c(desc, _cls("log_softmax", 3), post=post) == \
        "unfused post2=k_post<layer,0> class=k_class_out<log_softmax,one>"


def _refused(desc, cls, msg, post=None):
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(256)
    c = ctypes.byref(cls)
    for rc in (lib.xpg_forward_workspace_c(ctypes.byref(desc), post, None, None, c, 70, ctypes.byref(n)),
               lib.xpg_forward_describe_c(ctypes.byref(desc), post, None, None, c, 70, buf, 256),
               lib.xpg_masked_forward_c(ctypes.byref(desc), post, None, None, c, None, 70, None, None,
                                        1 << 40, None)):
        assert rc == 1  # XPG_EINVAL: no pointer was read, nothing launched
        assert msg in lib.xpg_last_error().decode()


def test_host_checks():
    layers = [(SAGE, 64), (SAGE, 64)]
    for bad in (3, -1, 99):
        _refused(_plain(layers), _cls(bad, 0), "class kind outside enum xpg_class_kind")
    for bad in (7, 8, -2, 1 << 20):
        _refused(_plain(layers, (7,)), _cls("softmax", bad), "class col outside [-1, C)")
    _refused(_plain(layers, ()), _cls(None, 64), "class col outside [-1, C)")  # headless: C = f_out
    assert _describe_c(_plain(layers, ()), _cls(None, 63)).endswith("<none,one>")
    d = _plain(layers)
    d.edge_masks = 1
    _refused(d, _cls(None, 0), "edge-mask plans (edge_masks)")
    d = _plain(layers)
    d.edge_dot = 1
    _refused(d, _cls(None, 0), "link decoder (edge_dot)")
    d = _plain(layers)
    d._keep[0][0].tgt_type = 256
    _refused(d, _cls(None, 0), "multi-node-type plans (tgt_type)")
    # an element-wise activation on the last linear map: refused under softmax / log_softmax only
    msg = "last layer with an element-wise activation"
    for kind in ("softmax", "log_softmax"):
        _refused(make_plan(layers, (7,)), _cls(kind, 0), msg)   # head act = sigmoid
        _refused(make_plan(layers, ()), _cls(kind, -1), msg)    # headless, conv act = relu
        d = _plain(layers, ())
        post = (_lib.PostDesc * 2)()
        post[1].act = 1                                          # headless, the post-op's relu
        _refused(d, _cls(kind, 0), msg, post=post)
    assert _describe_c(make_plan(layers, (7,)), _cls(None, 6)) == "unfused class=k_class_out<none,one>"


def test_class_out_rows_host_checks():
    lib = _lib.load()
    P = ctypes.c_void_p(256)
    ok = lambda *a: lib.xpg_class_out_rows(*a)
    assert ok(None, 0, 32, 7, 1, -1, None, None) == 0  # M = 0: nothing to do
    for args, msg in (((P, 4, 30, 7, 1, 0, P, None), "ld must be a multiple of 4"),
                      ((P, 4, 260, 7, 1, 0, P, None), "ld must be a multiple of 4"),
                      ((P, 4, 32, 33, 1, 0, P, None), "1 <= n_real <= ld"),
                      ((P, 4, 32, 0, 1, 0, P, None), "1 <= n_real <= ld"),
                      ((P, 4, 32, 7, 3, 0, P, None), "kind outside enum"),
                      ((P, 4, 32, 7, 1, 7, P, None), "col outside [-1, n_real)"),
                      ((P, 4, 32, 7, 1, -2, P, None), "col outside [-1, n_real)"),
                      ((P, -1, 32, 7, 1, 0, P, None), "M out of range"),
                      ((None, 4, 32, 7, 1, 0, P, None), "in must be non-null"),
                      ((ctypes.c_void_p(260), 4, 32, 7, 1, 0, P, None), "16-byte aligned"),
                      ((P, 4, 32, 7, 1, 0, None, None), "out must be non-null")):
        assert ok(*args) == 1 and msg in lib.xpg_last_error().decode()


# ------------------------------------------------------------------ the generic path's selection
def test_pick_classes():
    out = torch.arange(12.0).reshape(4, 3)
    assert torch.equal(pipeline.pick_classes(out, 4, 2, None), out[:, 2])
    assert torch.equal(pipeline.pick_classes(out, 4, None, None), out[:, 0])
    assert torch.equal(pipeline.pick_classes(out, 4, 1, "all"), out)
    assert torch.equal(pipeline.pick_classes(out[:, 0], 4, 0, None), out[:, 0])  # [rows]: C = 1
    assert tuple(pipeline.pick_classes(out[:, 0], 4, None, "all").shape) == (4, 1)
    with pytest.raises(ValueError, match=r"target class 3 outside \[0, 3\)"):
        pipeline.pick_classes(out, 4, 3, None)
    with pytest.raises(ValueError, match=r"target class 1 outside \[0, 1\)"):
        pipeline.pick_classes(out[:, 0], 4, 1, None)
    with pytest.raises(RuntimeError, match="has no"):
        pipeline.pick_classes(out, 3, 0, None)
    for bad in ({"classes": "some"}, {"out_col": -1}, {"out_col": 1.0}, {"out_col": True}):
        with pytest.raises(ValueError):
            pipeline.check_class_request(bad.get("out_col"), bad.get("classes"))
        with pytest.raises(ValueError):
            pipeline.generic_outputs(None, None, None, None, 0, "node_prediction", **bad)
        with pytest.raises(ValueError):
            pipeline.build_plan(None, None, None, [0], **bad)


def _explainer(params, problem="node_prediction"):
    feat = torch.randn(10, 6)
    ei = torch.randint(0, 10, (2, 30))
    arch = xnn.ConvStack("gcn", [6, 5], [5, 3], final_act="softmax")
    return Explainer(feat, ei, arch, params, [str(i) for i in range(10)], problem=problem)


def test_target_class_validation():
    assert _explainer({}).target_class == 0
    assert _explainer({"target_class": 2}).target_class == 2
    assert _explainer({"target_class": np.int64(1)}).target_class == 1
    for bad in (-1, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="target_class"):
            _explainer({"target_class": bad}).target_class
    e = _explainer({"target_class": 1})
    assert e._query_key("3", "cuda:0") != _explainer({"target_class": 2})._query_key("3", "cuda:0")
    assert e._query_key("3", "cuda:0") == _explainer({"target_class": 1})._query_key("3", "cuda:0")
    # edge problems and graphs of several node types have no class columns
    c = {"h_ntypes": None, "sub_nt": None}
    with pytest.raises(NotImplementedError, match="edge problems"):
        _explainer({"target_class": 1}, "edge_prediction")._check_class_support(c, "params['target_class'] = 1")
    c = {"h_ntypes": ["a", "b"], "sub_nt": torch.tensor([0, 1, 1])}
    with pytest.raises(NotImplementedError, match="more than one node type"):
        e._check_class_support(c, "run_classes")
    e._check_class_support({"h_ntypes": ["a"], "sub_nt": torch.tensor([0, 0])}, "run_classes")


# ------------------------------------------------------------------ the GPU cases' sensitivity
@pytest.mark.parametrize("out", cr.KINDS)
@pytest.mark.parametrize("C", cr.CLASSES)
@pytest.mark.parametrize("name", cr.NAMES)
def test_gpu_cases_are_not_vacuous(name, C, out):
    """On the reference alone, for the inputs tests/test_gpu_classes.py uses: every row a
    distribution, at least half of the explained-class probabilities in (0.02, 0.98), on at least
    half of the rows class c's output more than 100 x the GPU bar (1e-5) from class 0's, and the
    masks move the explained class by more than 10 x the bar."""
    c = cr.case(name, C, out)
    ref, k = c["ref"], c["c"]
    assert ref.shape == (cr.ROWS, len(c["queries"]), C) and 1 <= k < C
    assert c["masks"][1].all() and not c["masks"][0].any() and c["masks"].shape == (cr.ROWS, 400)
    p = np.exp(ref) if out == "log_softmax" else ref
    np.testing.assert_allclose(p.sum(-1), 1.0, rtol=0, atol=1e-12)
    assert np.mean((p[..., k] > 0.02) & (p[..., k] < 0.98)) >= 0.5
    assert np.mean(np.abs(ref[..., k] - ref[..., 0]) > 1e-3) >= 0.5
    assert np.ptp(ref[..., k], axis=0).max() > 1e-4
