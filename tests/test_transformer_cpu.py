"""TransformerConv without a GPU: nn.TransformerConv against the fp64 restatement of
tests/transformer_ref.py, the "qkv" lowering of program.compile_arch(..., attention=True) and its
refusals, the host side of the C-ABI (XPG_TERM_QKV: host checks, dispatch, workspace) on synthetic
descriptors whose device pointers are only tested for NULL, and the sensitivity conditions of the
GPU parity inputs (tests/test_gpu_transformer.py), asserted on the reference alone."""
import ctypes

import numpy as np
import pytest
import torch

import transformer_ref as tref
from test_dispatch_cpu import PTR, describe, make_plan, variants

from bikg_graph_explainability_public_amd import _lib, nn as xnn
from bikg_graph_explainability_public_amd.model import Model
from bikg_graph_explainability_public_amd.program import (UnsupportedArch, compile_arch,
                                                          count_message_passing)

ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------ module vs the restatement
def _conv_case(seed=3):
    """The hub graph, plus node 11 stripped of every in-edge (self-loops included)."""
    S = 400
    ei = tref.hub_graph(S)
    ei = ei[:, ei[1] != 11]
    x = torch.randn((S, 6), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return x, ei


@pytest.mark.parametrize("kw", [
    {}, {"heads": 1}, {"heads": 3}, {"heads": 1, "concat": False}, {"beta": True},
    {"beta": True, "heads": 1, "concat": False}, {"root_weight": False},
    {"root_weight": False, "beta": True}, {"bias": False}, {"bias": False, "beta": True, "heads": 3},
])
def test_module_matches_restatement_fp64(kw):
    x, ei = _conv_case()
    torch.manual_seed(5)
    args = dict(heads=2)
    args.update(kw)
    conv = xnn.TransformerConv(6, 5, **args).double().eval()
    with torch.no_grad():
        got = conv(x, torch.as_tensor(ei)).numpy()
    ref = tref.transformer_conv(x.numpy(), ei[0], ei[1], tref.conv_params(conv))
    assert got.shape == ref.shape == (400, 5 * (args["heads"] if args.get("concat", True) else 1))
    assert np.abs(got - ref).max() < 1e-12
    p = tref.conv_params(conv)
    if p["Ws"] is None:  # no in-edge, no skip: exactly 0
        assert (got[11] == 0).all()
    elif p["beta"] is None:  # no in-edge: the skip row alone
        xr = x.numpy() @ p["Ws"].T + (0 if p["bs"] is None else p["bs"])
        assert np.abs(got[11] - xr[11]).max() < 1e-12


def test_dropout_acts_in_training_mode_only():
    x, ei = _conv_case()
    torch.manual_seed(5)
    conv = xnn.TransformerConv(6, 5, heads=2, dropout=0.5).double()
    eit = torch.as_tensor(ei)
    with torch.no_grad():
        a, b = conv.eval()(x, eit), conv.eval()(x, eit)
        c = conv.train()(x, eit)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_module_state_dict_and_families():
    conv = xnn.TransformerConv(6, 5, heads=2, beta=True)
    shapes = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert shapes == {"lin_key.weight": (10, 6), "lin_key.bias": (10,), "lin_query.weight": (10, 6),
                      "lin_query.bias": (10,), "lin_value.weight": (10, 6), "lin_value.bias": (10,),
                      "lin_skip.weight": (10, 6), "lin_skip.bias": (10,), "lin_beta.weight": (1, 30)}
    avg = xnn.TransformerConv(6, 5, heads=3, concat=False, beta=True, bias=False)
    shapes = {k: tuple(v.shape) for k, v in avg.state_dict().items()}
    assert shapes["lin_skip.weight"] == (5, 6) and shapes["lin_beta.weight"] == (1, 15)
    assert "lin_skip.bias" not in shapes and shapes["lin_key.bias"] == (15,)
    noroot = xnn.TransformerConv(6, 5, root_weight=False, beta=True)  # lin_skip exists, no gate (PyG)
    assert "lin_skip.weight" in noroot.state_dict() and noroot.lin_beta is None
    other = xnn.TransformerConv(6, 5, heads=2, beta=True)
    other.load_state_dict(conv.state_dict())
    with pytest.raises(NotImplementedError):
        xnn.TransformerConv(6, 5, edge_dim=3)
    with pytest.raises(NotImplementedError):
        xnn.TransformerConv((6, 6), 5)
    arch = xnn.ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1], beta=True)
    assert arch.conv[2].in_channels == 16 and arch.conv[2].lin_beta is not None
    assert count_message_passing(arch) == 2 and Model(arch).get_hops(0) == 2
    assert not xnn.ConvStack("transformer", [4, 4], [4, 1], root_weight=False).conv[0].root_weight
    for kind in ("sage", "gatv2"):
        with pytest.raises(ValueError, match="beta applies to kind='transformer' only"):
            xnn.ConvStack(kind, [4, 4], [4, 1], beta=True)
        with pytest.raises(ValueError, match="root_weight applies to kind='transformer' only"):
            xnn.ConvStack(kind, [4, 4], [4, 1], root_weight=False)
        with pytest.raises(ValueError, match="beta applies to kind='transformer' only"):
            xnn.BlockStack(kind, [4, 4], [4, 1], beta=True)
        with pytest.raises(ValueError, match="root_weight applies to kind='transformer' only"):
            xnn.BlockStack(kind, [4, 4], [4, 1], root_weight=False)
    with pytest.raises(ValueError, match="heads must give one entry per conv layer"):
        xnn.ConvStack("transformer", [4, 4, 4], [4, 1], heads=[2])
    with pytest.raises(ValueError, match="share_weights applies to kind='gatv2' only"):
        xnn.ConvStack("transformer", [4, 4], [4, 1], share_weights=True)
    rels = [("n", "a", "n"), ("n", "b", "n")]
    het = xnn.ConvStack("transformer", [4, 4], [4, 1], hetero_rels=rels)
    assert isinstance(het.conv[0].convs["n__a__n"], xnn.TransformerConv)
    blk = xnn.BlockStack("transformer", [16, 16, 16], [32, 1], norm="layer", residual=True, heads=[2, 2],
                         beta=True)
    assert isinstance(blk.conv[0], xnn.TransformerConv) and blk.conv[1].normalized_shape == (32,)
    pooled = xnn.PooledModel(xnn.ConvStack("transformer", [16, 8], [8]), "mean", [8, 1])
    assert count_message_passing(pooled) == 1


# ------------------------------------------------------------------ lowering
class One(torch.nn.Module):
    def __init__(self, conv, width=8):
        super().__init__()
        self.conv = torch.nn.ModuleList([conv, torch.nn.ReLU()])
        self.fc = torch.nn.ModuleList([xnn.Linear(width, 1), torch.nn.Sigmoid()])


def test_lowering_fields():
    arch = xnn.ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1], beta=True).eval()
    prog = compile_arch(arch, attention=True)
    assert [len(c.terms) for c in prog.convs] == [1, 1] and prog.hops == 2
    for conv, layer, (H, C) in zip((arch.conv[0], arch.conv[2]), prog.convs, ((2, 8), (1, 8))):
        t = layer.terms[0]
        assert (t.kind, t.rel, t.heads, t.head_ch, t.self_loops) == ("qkv", 0, H, C, False)
        assert (layer.f_in, layer.f_out, layer.act) == (16, H * C, "relu")
        assert torch.equal(layer.bias, torch.zeros(H * C))
        for got, lin in ((t.weight, conv.lin_key), (t.weight_v, conv.lin_value),
                         (t.weight_q, conv.lin_query), (t.weight_s, conv.lin_skip)):
            assert torch.equal(got, lin.weight.detach())
        for got, lin in ((t.bias_l, conv.lin_key), (t.bias_v, conv.lin_value),
                         (t.bias_q, conv.lin_query), (t.bias_s, conv.lin_skip)):
            assert torch.equal(got, lin.bias.detach())
        w1, w2, w3 = conv.lin_beta.weight.detach().double().reshape(3, H * C)
        assert torch.equal(t.gate_out, (w1 + w3).float()) and torch.equal(t.gate_r, (w2 - w3).float())
    plain = compile_arch(One(xnn.TransformerConv(16, 8, bias=False)), attention=True).convs[0].terms[0]
    assert plain.gate_out is None and plain.gate_r is None and plain.bias_s is None
    assert plain.weight_s is not None and plain.bias_l is not None
    noroot = compile_arch(One(xnn.TransformerConv(16, 8, root_weight=False, beta=True)), attention=True)
    t = noroot.convs[0].terms[0]
    assert t.weight_s is None and t.bias_s is None and t.gate_out is None
    compile_arch(One(xnn.TransformerConv(16, 8, heads=1, concat=False, beta=True)), attention=True)
    rels = [("n", "a", "n"), ("n", "b", "n")]
    both = compile_arch(xnn.ConvStack("transformer", [16, 8], [8, 1], hetero_rels=rels), rels, attention=True)
    assert [(t.kind, t.rel) for t in both.convs[0].terms] == [("qkv", 0), ("qkv", 1)]
    mix = One(None)
    mix.conv = torch.nn.ModuleList([xnn.GCNConv(16, 8), torch.nn.ReLU(), xnn.TransformerConv(8, 4, heads=2),
                                    torch.nn.ReLU(), xnn.SAGEConv(8, 8), torch.nn.ReLU()])
    assert [c.terms[0].kind for c in compile_arch(mix, attention=True).convs] == ["gcn", "qkv", "mean"]
    pooled = xnn.PooledModel(xnn.ConvStack("transformer", [16, 8], [8]), "mean", [8, 1])
    prog = compile_arch(pooled, attention=True)
    assert prog.pool == "mean" and prog.convs[0].terms[0].kind == "qkv"
    blk = xnn.BlockStack("transformer", [16, 16, 16], [32, 1], norm="layer", residual=True, heads=[2, 2]).eval()
    prog = compile_arch(blk, attention=True)
    assert prog.convs[0].post.norm == "layer" and not prog.convs[0].post.residual
    assert prog.convs[1].post.residual and prog.convs[1].act is None
    bn = xnn.BlockStack("transformer", [16, 8], [8, 1], norm="batch").eval()
    post = compile_arch(bn, attention=True).convs[0].post  # not folded: the logits read the rows
    assert post.scale is not None and post.norm is None


def test_lowering_refusals():
    arch = xnn.ConvStack("transformer", [16, 8, 8], [8, 1], heads=[2, 1])
    with pytest.raises(UnsupportedArch, match="TransformerConv without the attention opt-in"):
        compile_arch(arch)
    with pytest.raises(UnsupportedArch, match="TransformerConv without the attention opt-in"):
        compile_arch(xnn.PooledModel(xnn.ConvStack("transformer", [16, 8], [8]), "mean", [8, 1]))
    with pytest.raises(UnsupportedArch, match=r"TransformerConv\(concat=False\) with several heads"):
        compile_arch(One(xnn.TransformerConv(16, 8, heads=2, concat=False)), attention=True)
    conv = xnn.TransformerConv(16, 8)
    conv.edge_dim = 3
    with pytest.raises(UnsupportedArch, match="TransformerConv with edge_dim"):
        compile_arch(One(conv), attention=True)
    conv = xnn.TransformerConv(16, 8)
    conv.lin_edge = xnn.Linear(3, 8, bias=False)
    with pytest.raises(UnsupportedArch, match="TransformerConv with edge_dim"):
        compile_arch(One(conv), attention=True)
    for name in ("lin_key", "lin_query", "lin_value", "lin_skip"):
        conv = xnn.TransformerConv(16, 8)
        setattr(conv, name, xnn.Linear(-1, 8))
        with pytest.raises(UnsupportedArch, match="uninitialised \\(lazy\\) weights"):
            compile_arch(One(conv), attention=True)
    conv = xnn.TransformerConv(16, 8)
    conv.in_channels = (16, 16)
    with pytest.raises(UnsupportedArch, match="bipartite relation / with tuple in_channels"):
        compile_arch(One(conv), attention=True)
    mrels = [("a", "r", "b"), ("b", "s", "a")]
    het = One(xnn.HeteroConv({r: xnn.TransformerConv(16, 8) for r in mrels}))
    with pytest.raises(UnsupportedArch, match="TransformerConv on a multi-node-type graph"):
        compile_arch(het, mrels, ["a", "b"], attention=True)
    same = [("a", "r", "a"), ("b", "s", "b")]
    het = One(xnn.HeteroConv({r: xnn.TransformerConv(16, 8) for r in same}))
    with pytest.raises(UnsupportedArch, match="TransformerConv on a multi-node-type graph"):
        compile_arch(het, same, ["a", "b"], attention=True)
    with pytest.raises(UnsupportedArch, match="bipartite relations need the multi-node-type path"):
        compile_arch(One(xnn.HeteroConv({mrels[0]: xnn.TransformerConv(16, 8)})), mrels[:1], attention=True)
    rels = [("n", "a", "n"), ("n", "b", "n")]
    for other in (xnn.SAGEConv(16, 8), xnn.GATv2Conv(16, 8), xnn.GATConv(16, 8)):
        mixed = One(xnn.HeteroConv({rels[0]: xnn.TransformerConv(16, 8), rels[1]: other}))
        with pytest.raises(UnsupportedArch, match="a conv layer mixing (TransformerConv|GATv2Conv|GATConv) "
                                                  "with other relations"):
            compile_arch(mixed, rels, attention=True)
    with pytest.raises(UnsupportedArch, match="TransformerConv wider than 256 columns"):
        compile_arch(One(xnn.TransformerConv(16, 65, heads=4), 260), attention=True)
    compile_arch(One(xnn.TransformerConv(16, 64, heads=4), 256), attention=True)
    link = xnn.LinkModel(xnn.ConvStack("transformer", [16, 8], [8, 4], final_act="identity"))
    with pytest.raises(UnsupportedArch, match="TransformerConv without the attention opt-in"):
        compile_arch(link)  # edge-mask and link programs never ask for the opt-in


# ------------------------------------------------------------------ descriptors (host only)
QKV, SAGE, GCN = ("att2",), ("mean", "root"), ("gcn",)  # "att2": make_plan's placeholder, re-kinded below


def _qkv_plan(layers=((QKV, 16), (QKV, 8)), heads=(1,), hc=((2, 8), (1, 8)), nb=4, gate=True, **kw):
    """make_plan's descriptor with the QKV layers filled in as the header describes them."""
    desc = make_plan(list(layers), heads, **kw)
    for li, (ld, (kinds, _)) in enumerate(zip(desc._keep[0], layers)):
        if "att2" not in kinds:
            continue
        ld.weight = None
        for k, kind in enumerate(kinds):
            if kind != "att2":
                continue
            t = ld.terms[k]
            t.kind = _lib.TERM_QKV
            t.heads, t.head_ch = hc[li]
            t.neg_slope, t.self_loops = float(hc[li][1]) ** -0.5, 0
            t.n_slices = nb
            t.table = PTR
            t.att_src = PTR if gate and nb == 4 else None
            t.att_dst = None
            t.coef = None if li == 0 else PTR
    return desc


def _ws(desc, rows=70):
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_forward_workspace(ctypes.byref(desc), rows, ctypes.byref(n)))
    return n.value


def _refused(desc, msg):
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(256)
    for rc in (lib.xpg_forward_workspace(ctypes.byref(desc), 70, ctypes.byref(n)),
               lib.xpg_forward_describe(ctypes.byref(desc), 70, buf, 256),
               lib.xpg_masked_forward(ctypes.byref(desc), None, 70, None, None, 1 << 40, None)):
        assert rc == 1  # XPG_EINVAL: no pointer was read, nothing launched
        assert msg in lib.xpg_last_error().decode()


def test_abi_is_unchanged():
    assert _lib.TERM_QKV == 8 and _lib.ABI_VERSION == 28
    assert _lib.TERM == {"gcn": 0, "mean": 1, "root": 2, "att": 3, "sum": 4, "max": 5, "rel": 6, "att2": 7}
    assert [f[0] for f in _lib.LayerDesc._fields_][-2:] == ["seg_rel", "pool"]
    assert _lib.ForwardPlanDesc._fields_[-1][0] == "dot_scale"
    assert len(variants()) == 27


def test_host_checks():
    d = _qkv_plan(layers=(((("att2", "mean")), 16), (QKV, 8)))
    d._keep[0][0].terms[1].table = PTR
    _refused(d, "QKV terms cannot be mixed with other kinds")
    d = _qkv_plan(layers=((QKV, 16), (("att2", "att"), 8)))
    _refused(d, "QKV terms cannot be mixed with other kinds")
    d = _qkv_plan()
    d.edge_masks = 1
    _refused(d, "edge-mask plans (edge_masks)")
    d = _qkv_plan()
    d._keep[0][1].tgt_type = PTR
    _refused(d, "multi-node-type plans (tgt_type)")
    d = _qkv_plan()
    d._keep[0][0].terms[0].dst_type = 0
    _refused(d, "dst_type must be -1")
    d = _qkv_plan(hc=((2, 17), (1, 8)))
    _refused(d, "heads * head_ch must fit")
    d = _qkv_plan(hc=((2, 8), (0, 8)))
    _refused(d, "heads * head_ch must fit")
    for nb in (0, 2, 5):
        d = _qkv_plan()
        d._keep[0][1].terms[0].n_slices = nb
        _refused(d, "n_slices must be 3 (K, V, Q) or 4 (and S)")
    d = _qkv_plan()
    d._keep[0][0].terms[0].n_slices = 3
    _refused(d, "a gate (att_src) needs the S block")
    for li, field, msg in ((0, "table", "missing table"), (1, "table", "missing table"),
                           (1, "coef", "deeper layer needs coef")):
        d = _qkv_plan()
        setattr(d._keep[0][li].terms[0], field, None)
        _refused(d, msg)
    d = _qkv_plan()
    d._keep[0][1].weight = PTR
    _refused(d, "weight must be NULL")
    d = _qkv_plan()
    d._keep[0][0].weight, d._keep[0][0].f_in_pad = PTR, 32
    _refused(d, "does not take the raw form")
    d = _qkv_plan()
    d._keep[0][1].f_in_pad = 64
    _refused(d, "f_in_pad must equal previous f_out_pad")
    for nb, gate in ((4, True), (4, False), (3, False)):  # the accepted forms
        assert _ws(_qkv_plan(nb=nb, gate=gate)) > 0


def test_weighted_and_featured_entry_points_refuse_qkv():
    lib = _lib.load()
    d = _qkv_plan()
    lw = (_lib.LayerWeights * 2)()
    wts = _lib.EdgeWeights(deg_w=PTR, loop_w=PTR, layers=lw)
    rc = lib.xpg_masked_forward_w(ctypes.byref(d), None, ctypes.byref(wts), None, 70, None, None, 1 << 40, None)
    assert rc == 1 and b"edge weights take GCN / MEAN / SUM / MAX / ROOT terms only" in lib.xpg_last_error()
    le = (_lib.LayerEfeat * 2)()
    fe = _lib.EdgeFeats(layers=le)
    rc = lib.xpg_masked_forward_e(ctypes.byref(d), None, None, ctypes.byref(fe), None, 70, None, None, 1 << 40,
                                  None)
    assert rc == 1 and b"edge features take SUM / ROOT terms only" in lib.xpg_last_error()


@pytest.mark.parametrize("kw", [{}, {"n_nodes": 10000, "n_tgt": 10000}, {"n_nodes": 40, "n_tgt": 8}])
def test_qkv_plans_take_the_multi_kernel_path(kw, monkeypatch):
    for layers in (((QKV, 16), (QKV, 8)), ((GCN, 32), (QKV, 32)), ((QKV, 32), (SAGE, 32))):
        desc = _qkv_plan(layers=layers, hc=((2, 8), (1, 8)), **kw)
        assert describe(desc) == "unfused"
        for forced in ("rows", "fused", "wide"):
            monkeypatch.setenv("XPG_FORWARD", forced)
            monkeypatch.delenv("XPG_FORWARD_STRICT", raising=False)
            assert describe(desc) == "unfused"
            monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
            with pytest.raises(RuntimeError, match="forced XPG_FORWARD path does not take this plan"):
                describe(desc)
            rc = _lib.load().xpg_masked_forward(ctypes.byref(desc), None, 70, None, None, 1 << 40, None)
            assert rc == 1 and b"does not take this plan" in _lib.load().xpg_last_error()
        monkeypatch.delenv("XPG_FORWARD")
        monkeypatch.delenv("XPG_FORWARD_STRICT")


def test_workspace_of_qkv_plans():
    """Per layer the output rows; per QKV layer past the first the transformed-rows region (rows *
    n_prev * (sum of the terms' n_slices) * f_out_pad floats, the largest); no dense-input and no
    score region for them."""
    up = lambda b: (b + 255) // 256 * 256
    rows, n = 70, 300
    fixed = up(4 * rows * n) + 2 * up(4 * rows * n * 32) + up(4 * 32)  # degrees, two head buffers, counters
    for nb in (4, 3):  # one term, with and without root
        got = _ws(_qkv_plan(nb=nb), rows)
        assert got == fixed + 2 * up(4 * rows * n * 32) + up(4 * rows * n * nb * 32)
        two = _qkv_plan(layers=((QKV, 16), (("att2", "att2"), 40)), hc=((2, 8), (1, 40)), nb=nb)
        assert _ws(two, rows) == fixed + up(4 * rows * n * 32) + up(4 * rows * n * 64) + \
            up(4 * rows * n * 2 * nb * 64)
    first = _qkv_plan(layers=((QKV, 32), (SAGE, 32)))
    plain = make_plan([(SAGE, 32), (SAGE, 32)])
    assert _ws(first, rows) == _ws(plain, rows)  # a QKV first layer adds no region


# ------------------------------------------------------------------ the GPU cases' sensitivity
@pytest.mark.parametrize("q_scale", [1.0, 32.0])
@pytest.mark.parametrize("root,beta", [(True, False), (True, True), (False, False)])
def test_gpu_cases_are_sensitive(root, beta, q_scale):
    """From the fp64 reference alone, for the inputs tests/test_gpu_transformer.py uses: at least
    half of the 64 rows more than 1e-3 (100 x the GPU bar) from the all-on row, at least a fifth of
    the 64 x 3 outputs more than 1e-3 from the same model under uniform attention (query weights
    and bias 0), and every output off the sigmoid's tails.  A kernel that ignores the masks, or the
    logits, cannot pass."""
    c = tref.hub_case(root, beta, q_scale)
    ref, uni, m = c["ref"], c["uniform"], c["masks"]
    assert ref.shape == uni.shape == (64, 3) and m[1].all() and not m[0].any()
    assert not m[2, 0] and not m[3, 7] and not m[4, 399]
    moved = (np.abs(ref - ref[1]) > 1e-3).any(1).sum()
    dyn = (np.abs(ref - uni) > 1e-3).sum()
    print("rows off the all-on row:", moved, "outputs off uniform attention:", dyn,
          "range:", ref.min(), ref.max())
    assert moved >= 32
    assert dyn >= 39  # a fifth of 192
    assert ((ref > 0.02) & (ref < 0.98)).all()


def test_spread_case_has_a_wide_logit_span():
    """lin_query x 32: the layer-1 logits span more than 89, so exp(z - max) underflows to 0 for
    some kept edge of fp32 softmax and a kernel without the running max would overflow."""
    c = tref.hub_case(True, True, 32.0)
    span = tref.layer1_logit_span(c["arch"], c["x"].numpy(), c["ei"])
    print("layer-1 logit span:", span)
    assert span > 89


def test_gate_case_differs_from_the_plain_sum():
    """beta: at least a fifth of the outputs more than 1e-3 from the model whose gate is replaced
    by out + x_r.  lin_beta is used as initialised (not scaled)."""
    for q_scale in (1.0, 32.0):
        c = tref.hub_case(True, True, q_scale)
        n = (np.abs(c["ref"] - c["plain"]) > 1e-3).sum()
        print("outputs off the plain sum:", n)
        assert n >= 39
