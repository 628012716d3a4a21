"""The rows / fused / multi-kernel forward variants on a machine without a GPU.

* Reachability: every case of tests/forward_ref.py, as a plan descriptor with the device plan's
  sizes and term kinds (forward_ref.descriptor), makes xpg_forward_kernels write exactly the text
  tests/test_gpu_forward_variants.py asserts before it compares numbers.
* Closure: the kernels named over all cases + UNREACHABLE + C_ABI_ONLY == xpg_forward_variants().
* Oracle-only conditions (strict; they keep a passing GPU comparison from meaning nothing): the
  fp64 reference varies over the mask rows, feels the hubs' last in-edges, and the compared set
  holds the all-off row and the target without in-edges.

The target without in-edges is the one column whose reference must NOT vary: GCN keeps its
self-loop and SAGE its root term whether or not the node is masked, and nothing reaches it, so its
fp64 output is one value on all 130 rows (asserted exactly below).  The range condition therefore
covers every other compared column."""
import ctypes
import re

import numpy as np
import pytest

import forward_ref as fr
from bikg_graph_explainability_public_amd import _lib
from test_dispatch_cpu import GCN, PTR, SAGE, make_plan

KERNEL = re.compile(r"k_(?:rows_forward|fused_forward|agg_l1_rows|agg|dense)<[0-9,]+>")

# Instantiations in the library that no plan and no switch reaches, with the dispatcher's reason.
UNREACHABLE = {
    # dense_pick: 4 or 8 column tiles (n_pad 128 / 256) always split over 4 column groups of 1 / 2
    # tiles per wave, so NT = tiles / groups is never 4 or 8
    "k_dense<4,0>": "n_pad = 128 dispatches to k_dense<1,0> with 4 column groups",
    "k_dense<4,1>": "n_pad = 128 dispatches to k_dense<1,1> with 4 column groups",
    "k_dense<8,0>": "n_pad = 256 dispatches to k_dense<2,0> with 4 column groups",
    "k_dense<8,1>": "n_pad = 256 dispatches to k_dense<2,1> with 4 column groups",
}
# Instantiations the library's dispatcher names only for descriptors engine.ForwardPlan never builds
# (it refuses conv layers wider than 256; a raw layer 1 wider than 256 is refused by the library
# itself): reachable through the C-ABI alone, not compared with fp64 by any GPU test.
C_ABI_ONLY = {
    "k_agg<1,64,2>": "a table-form layer 1 of width 512",
    "k_agg<1,64,4>": "a table-form layer 1 of width 1024",
    "k_agg<0,64,2>": "a layer past the first whose input is 512 wide",
    "k_agg<0,64,4>": "a layer past the first whose input is 1024 wide",
}
# A run-time form (no instantiation of its own, so outside the closure set) that no caller of
# engine.ForwardPlan reaches.
UNREACHABLE_FORMS = {
    "k_rows_forward without a control block (ctl == NULL: workgroup b takes 64-row block b)":
        "xpg_masked_forward hands the kernel workspace + the layout's ctl offset whenever a workspace "
        "is given, and the workspace is never empty (it holds the 128-byte control block itself): only "
        "a caller that passes a NULL workspace with a non-zero size gets this form",
}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in fr.ENV:
        monkeypatch.delenv(k, raising=False)


def kernels(desc, rows, size=1024):
    buf = ctypes.create_string_buffer(size)
    _lib.check(_lib.load().xpg_forward_kernels(ctypes.byref(desc), rows, buf, size))
    return buf.value.decode()


def describe(desc, rows):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().xpg_forward_describe(ctypes.byref(desc), rows, buf, 256))
    return buf.value.decode()


def variants():
    buf = ctypes.create_string_buffer(4096)
    _lib.check(_lib.load().xpg_forward_variants(buf, len(buf)))
    return buf.value.decode().split()


# ------------------------------------------------------------------ reachability
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_case_reaches_its_kernels(name, monkeypatch):
    c = fr.CASES[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    desc = fr.descriptor(name)
    assert kernels(desc, c.rows) == c.want
    assert describe(desc, c.rows) == c.want.split()[0]  # xpg_forward_describe's texts are unchanged
    if not c.env:  # the default path: forcing it names the same kernel
        monkeypatch.setenv("XPG_FORWARD", c.want.split()[0])
        monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
        assert kernels(desc, c.rows) == c.want


def test_rows_form_cases_are_one_step_apart(monkeypatch):
    """"overfill" is "fill" plus one target, and that one target (2 more frontier nodes) moves the
    plan from the rows kernel with its mask rows in global memory to the multi-kernel path: the
    bits=global case sits at the LDS limit, not merely somewhere past the staging threshold."""
    assert fr.QUERIES["overfill"][:-1] == fr.QUERIES["fill"]
    fill, over = "rows-form-bits-global", "rows-too-big"
    assert fr.CASES[fill].queries == "fill" and fr.CASES[over].queries == "overfill"
    assert fr.model_key(fill) == fr.model_key(over) and not fr.CASES[over].env
    n0 = [fr.plan_arrays(n)["frontiers"][0].size for n in (fill, over)]
    assert 0 < n0[1] - n0[0] <= 3
    assert " bits=global " in kernels(fr.descriptor(fill), fr.ROWS)
    assert kernels(fr.descriptor(over), fr.ROWS).startswith("unfused ")
    monkeypatch.setenv("XPG_FORWARD", "rows")  # forced and strict: the rows kernel refuses it
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="does not take this plan"):
        kernels(fr.descriptor(over), fr.ROWS)


def test_fused_declines_what_does_not_fit(monkeypatch):
    c = fr.FUSED_DECLINED
    desc = fr.descriptor(c)
    monkeypatch.setenv("XPG_FORWARD", "fused")
    assert kernels(desc, fr.ROWS) == c.want
    monkeypatch.setenv("XPG_FORWARD_STRICT", "1")
    with pytest.raises(RuntimeError, match="forced XPG_FORWARD path does not take this plan"):
        kernels(desc, fr.ROWS)


def test_edge_mask_plan_reaches_the_generic_layer1(monkeypatch):
    """A 32-wide layer 1 goes to k_agg_l1_rows on a node-mask plan and to k_agg<1,8,1> on an
    edge-mask plan (XPG_FORWARD unset, no diagnostics switch)."""
    desc = fr.edge_descriptor()
    assert desc.cols == fr.graph().shape[1] and desc.edge_masks == 1
    assert kernels(desc, fr.ROWS) == fr.EDGE_WANT and " l1=k_agg<1,8,1> " in fr.EDGE_WANT
    assert describe(desc, fr.ROWS) == "unfused"
    desc.edge_masks, desc.cols = 0, fr.S  # the same sizes as a node-mask plan: the rows-as-lanes kernel
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    assert " l1=k_agg_l1_rows<32,1>x1 " in kernels(desc, fr.ROWS)


def test_two_type_plan_reaches_the_per_type_bias_form():
    """Every dense launch of a conv layer of a multi-node-type plan carries row_type (`t`)."""
    desc = fr.mt_descriptor()
    assert kernels(desc, fr.ROWS) == fr.MT_WANT and "g1t " in fr.MT_WANT
    assert describe(desc, fr.ROWS) == "unfused"
    for l in range(desc.n_layers):  # without the type rows the same plan names the plain form
        desc.layers[l].tgt_type = None
    assert kernels(desc, fr.ROWS).replace("g1t", "g1") == kernels(desc, fr.ROWS)


# ------------------------------------------------------------------ closure
def test_every_variant_is_asserted_or_accounted_for():
    asserted = set()
    for want in [c.want for c in fr.CASES.values()] + [fr.EDGE_WANT, fr.MT_WANT, fr.FUSED_DECLINED.want]:
        asserted |= set(KERNEL.findall(want))
    listed = variants()
    assert len(listed) == len(set(listed)) == 49
    for other in (UNREACHABLE, C_ABI_ONLY):
        assert not (asserted & set(other)), "an asserted variant is listed as not reached"
    assert not (set(UNREACHABLE) & set(C_ABI_ONLY))
    assert asserted - set(listed) == set(), "a case expects a kernel the library does not hold"
    assert set(listed) - asserted - set(UNREACHABLE) - set(C_ABI_ONLY) == set()


def test_run_time_forms_are_all_asserted():
    wants = " ".join(c.want for c in fr.CASES.values())
    for token in ("bits=lds", "bits=global", "w2=lds", "w2=global", "w2=-", "head=lds", "head=global",
                  "head=global,lds", "layers=1", "layers=2", "layers=3", "layers=4", "tpp=8", "tpp=4",
                  "tpp=2", "tpp=1", ">x1 ", ">x2 ", ">x4 ", "g1", "g4", "tail=epilogue", "tail=k_take_col"):
        assert token in wants, token
    assert any(c.rows == 1 for c in fr.CASES.values())


def test_unreachable_dense_variants(monkeypatch):
    """Every padded width and both epilogue forms through the dispatcher: k_dense<4,*> and <8,*>
    are never named (dense_pick's column groups)."""
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    seen = set()
    for w in range(32, 257, 32):
        for heads in ((1,), (w, 1)):
            seen |= set(KERNEL.findall(kernels(make_plan([(GCN, 32), (SAGE, w)], heads), 70)))
    dense = {k for k in seen if k.startswith("k_dense")}
    assert dense == {k for k in variants() if k.startswith("k_dense")} - set(UNREACHABLE)


@pytest.mark.parametrize("width,nv", [(512, 2), (1024, 4)])
def test_c_abi_only_agg_variants(width, nv, monkeypatch):
    """What C_ABI_ONLY states: descriptors of layer width 512 / 1024 are named k_agg<*,64,2|4>; the
    raw form (the other way to a wide k_agg<0,...>) is refused past 256, and so is width 2048."""
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    text = kernels(make_plan([(GCN, width), (GCN, 32)]), 70)
    assert text.startswith(f"unfused l1=k_agg<1,64,{nv}> l2=k_agg<0,64,{nv}>+k_dense<1,1>g1")
    raw = make_plan([(("max",), 32), (GCN, 32)])
    raw.layers[0].weight, raw.layers[0].f_in_pad = PTR, width
    with pytest.raises(RuntimeError, match="raw layer 1"):
        kernels(raw, 70)
    with pytest.raises(RuntimeError, match="unsupported row width"):
        kernels(make_plan([(GCN, 2048), (GCN, 32)]), 70)


# ------------------------------------------------------------------ the query's own contract
def test_kernels_query_errors_and_siblings(monkeypatch):
    lib = _lib.load()
    desc = make_plan([(GCN, 32), (GCN, 32)], n_nodes=40, n_tgt=8)
    want = "rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=lds"
    assert kernels(desc, 70) == want
    buf = ctypes.create_string_buffer(1024)
    _lib.check(lib.xpg_forward_kernels_c(ctypes.byref(desc), None, None, None, None, 70, buf, 1024))
    assert buf.value.decode() == want
    small = ctypes.create_string_buffer(8)
    assert lib.xpg_forward_kernels(ctypes.byref(desc), 70, small, 8) == 3  # XPG_ENOSPC
    assert small.value == b""
    assert lib.xpg_forward_variants(small, 8) == 3
    cls = _lib.ClassOut(kind=1, col=-1)  # a class readout: the multi-kernel path, its own tail
    logits = make_plan([(GCN, 32), (GCN, 32)], (4,), n_nodes=40, n_tgt=8)
    logits.head[0].act = 0  # softmax takes the last layer's linear output
    _lib.check(lib.xpg_forward_kernels_c(ctypes.byref(logits), None, None, None, ctypes.byref(cls), 70, buf, 1024))
    assert buf.value.decode() == ("unfused l1=k_agg_l1_rows<32,1>x1 l2=k_agg<0,8,1>+k_dense<1,0>g1 "
                                  "head=k_dense<1,0>g1 tail=k_class_out<softmax,all>")
    monkeypatch.setenv("XPG_AGG_GENERIC", "1")  # a diagnostics switch without XPG_DIAGNOSTICS
    monkeypatch.setenv("XPG_FORWARD", "unfused")
    with pytest.raises(RuntimeError, match="XPG_DIAGNOSTICS"):
        kernels(desc, 70)
    big = make_plan([(SAGE, 128), (SAGE, 128)], n_nodes=10000, n_tgt=10000)
    monkeypatch.delenv("XPG_AGG_GENERIC")
    monkeypatch.delenv("XPG_FORWARD")
    assert kernels(big, 70) == describe(big, 70)  # the wide path: what describe says


# ------------------------------------------------------------------ inputs and oracle-only conditions
def test_graph_and_masks_are_what_the_cases_need():
    ei, m = fr.graph(), fr.masks()
    assert ei.max() < fr.S <= 300 and m.shape == (130, fr.S)
    indeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=fr.S)
    assert indeg[fr.HUB70] == 70 and indeg[fr.HUB130] == 130 and indeg[fr.NO_IN] == 0
    assert int((ei[0] == ei[1]).sum()) == 10
    pairs = ei[0] * fr.S + ei[1]
    assert ei.shape[1] - np.unique(pairs).size == 12  # the 10 duplicated edges + 2 of the random draw's own
    assert m[0].all() and not m[1].any() and 0 < m[2].mean() < 0.08
    dens = m[3:].mean(1)
    assert dens.min() > 0.1 and dens.max() < 0.97
    for q in fr.QUERIES.values():
        assert fr.NO_IN in q and len(set(q)) == len(q)


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_reference_alone_can_tell_a_wrong_kernel(name):
    c = fr.CASES[name]
    q = fr.QUERIES[c.queries]
    ref = fr.reference(name)
    # nothing is left out: one column per query, all 130 rows (the all-off row 1 among them)
    assert ref.shape == (fr.ROWS, len(q)) and np.isfinite(ref).all()
    assert fr.plan_arrays(name)["frontiers"][-1].tolist() == list(q)  # the plan's output order
    spread = ref.max(0) - ref.min(0)
    for col, node in enumerate(q):
        if node == fr.NO_IN:
            assert spread[col] == 0.0  # constant by construction (module docstring)
        else:
            assert spread[col] >= 1e-2, (node, spread[col])  # 1000 x the bar: no saturated head
    for hub in (fr.HUB70, fr.HUB130):
        if hub in q:  # the hub's last in-edge matters: > 10 x the bar in at least one row
            d = np.abs(fr.reference_hub_edge_dropped(name, hub)[:, q.index(hub)] - ref[:, q.index(hub)])
            assert d.max() > 1e-4, (hub, d.max())


def test_every_kernel_family_meets_both_hubs():
    """Cases of small receptive fields (the rows kernel's form cases, the fused kernel's deep plans)
    hold no hub; each kernel family still has cases with the 70- and the 130-in-edge target."""
    for family in ("rows ", "fused ", "unfused "):
        for hub in (fr.HUB70, fr.HUB130):
            assert any(c.want.startswith(family) and hub in fr.QUERIES[c.queries] for c in fr.CASES.values())
    for kernel in ("k_rows_forward<2,0>", "k_rows_forward<4,0>", "k_rows_forward<8,0>", "k_rows_forward<2,1>",
                   "k_rows_forward<4,1>", "k_rows_forward<8,1>"):
        assert any(kernel in c.want and (fr.HUB70 in fr.QUERIES[c.queries] or fr.HUB130 in fr.QUERIES[c.queries])
                   for c in fr.CASES.values()), kernel


def test_edge_and_two_type_references_can_tell_a_wrong_kernel():
    """The two plans outside the table: their fp64 references vary by 1000 x the bar over the rows;
    the all-off row is among them (an edge plan without edges; a copy without edges outputs 0)."""
    e = fr.edge_reference()
    m = fr.edge_masks()
    assert e.shape == (fr.ROWS,) and np.isfinite(e).all() and e.max() - e.min() >= 1e-2
    assert m[0].all() and not m[1].any()
    u, v = fr.edge_query()
    assert v == fr.HUB70 and (fr.graph()[1] == v).sum() == 70
    r = fr.mt_reference()
    c = fr.mt_setup()[1]
    keeps = (fr.mt_masks()[:, c["ei"][0]] & fr.mt_masks()[:, c["ei"][1]]).any(1)
    assert r.shape == (fr.ROWS,) and not keeps[1] and (r[~keeps] == 0).all()
    assert keeps.sum() >= 120 and r[keeps].max() - r[keeps].min() >= 1e-2
    assert len(c["ntypes"]) == 2 and len(np.unique(c["nt"])) == 2


def test_attention_last_layer_names_the_dense_launch_of_its_epilogue(monkeypatch):
    """An attention layer past the first ends in a dense launch; with one head layer that launch
    carries the output column, and the text names it before `tail=epilogue`."""
    desc = make_plan([(("att",), 32), (("att",), 64)], (1,))
    for l, ch in enumerate((32, 64)):
        t = desc.layers[l].terms[0]
        t.heads, t.head_ch, t.att_src, t.att_dst = 1, ch, PTR, PTR
    assert kernels(desc, 70) == "unfused l1=att l2=att+k_dense<2,1>g1 head=- tail=epilogue"
