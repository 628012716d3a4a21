"""One repeat of the explanation hot path on the device (explainer.py:490-519 loop body):

    mask rows (compat host sampler -> bit-pack, or device Philox sampler)
      -> per-row query logit      (ForwardPlan.forward: masked receptive-field message passing)
      -> KernelSHAP fp64 weights  (xpg_popcount_rows + xpg_shap_kernel)
      -> surrogate Adam epochs    (xpg_wlm_fit, one persistent workgroup)

Architectures the engine cannot compile run through `generic_outputs` (the user's torch module
on the B-fold union graph built with the HIP edge-keep kernel) — still on the GPU, with the
KernelSHAP and surrogate stages unchanged.
"""
import collections
import inspect
import warnings
import weakref

import torch

from . import engine
from .data import Data
from .model import Model
from .program import UnsupportedArch, check_rel_features, compile_arch


# generic multi-node-type path: one arch call over the per-type disjoint union of the copies
# (False: the reference's per-copy loop, model.py:118-253)
HETERO_BATCHED = True

def relation_edges(edge_index, edge_type, n_rel):
    if edge_type is None:
        return [edge_index]
    et = edge_type.to(edge_index.device)
    return [edge_index[:, et == r] for r in range(n_rel)]


def typed_relations(prog):
    """The relation count of a typed-relation (RGCNConv) program, 0 for every other program.
    ValueError when its convs disagree."""
    counts = {t.num_relations for c in prog.convs for t in c.terms if t.kind == "rel"}
    if len(counts) > 1:
        raise ValueError(f"RGCNConv layers with different num_relations {sorted(counts)}")
    return counts.pop() if counts else 0


def typed_relation_edges(edge_index, edge_type, n_rel, return_order=False):
    """relation_edges for a typed-relation program: it needs the edge types, all inside [0, n_rel).
    return_order: also the sort's permutation (each edge's position in `edge_index`, relation by
    relation): the mask columns of an edge-mask plan."""
    if edge_type is None:
        raise ValueError("a RGCNConv model needs edge_types")
    et = edge_type.reshape(-1)
    if et.numel() != edge_index.shape[1]:
        raise ValueError("edge_types must give one type per edge")
    if et.numel() and (int(et.min()) < 0 or int(et.max()) >= n_rel):
        raise ValueError(f"edge type outside [0, {n_rel})")
    # one stable sort on the host (the plan builder reads host arrays) instead of n_rel device
    # selections: each relation's edges in edge order, as relation_edges gives them
    ei, et = edge_index.detach().cpu(), et.detach().cpu().long()
    order = torch.argsort(et, stable=True)
    rels = list(torch.split(ei[:, order], torch.bincount(et, minlength=n_rel).tolist(), dim=1))
    return (rels, order) if return_order else rels


_PROGRAMS = collections.OrderedDict()  # compiled_program's cache: key -> (weakref(arch), program)


def clear_programs():
    """Drop every cached compiled program and its padded device weights (compiled_program)."""
    _PROGRAMS.clear()


def compiled_program(arch, edge_type_names=None, node_type_names=None, state=None,
                     attention=False, edge_weight=False, edge_attr=False):
    """compile_arch(arch, ...) once per module state: keyed by the module (identity, checked by
    weak reference), every parameter and buffer (storage + in-place version counter: an
    optimizer step, load_state_dict or a replaced tensor compiles again) and the type names.
    The program carries the plans' weight-derived device tensors (ForwardPlan._program_tensor),
    so a new query's plan neither lowers the module nor re-pads its weights.  8 programs kept.
    `state`: the caller's (parameters, buffers) state tuples of this walk (Explainer.run reads
    them once per call); None reads them here.  An edit through `param.data` (e.g.
    `p.data.copy_(w)`) bumps no version counter and is not seen: call clear_programs() (or
    Explainer.clear_cache()) after one."""
    if state is None:
        state = (tuple((t.data_ptr(), t._version) for t in arch.parameters()),
                 tuple((t.data_ptr(), t._version) for t in arch.buffers()))
    key = (id(arch), state,
           tuple(tuple(e) for e in edge_type_names) if edge_type_names is not None else None,
           tuple(node_type_names) if node_type_names is not None else None, bool(attention),
           bool(edge_weight), bool(edge_attr), module_out_norm(arch))
    hit = _PROGRAMS.get(key)
    if hit is not None and hit[0]() is arch:
        _PROGRAMS.move_to_end(key)
        return hit[1]
    prog = compile_arch(arch, edge_type_names, node_type_names, attention=bool(attention),
                        edge_weight=bool(edge_weight), edge_attr=bool(edge_attr))
    _PROGRAMS[key] = (weakref.ref(arch), prog)
    while len(_PROGRAMS) > 8:
        _PROGRAMS.popitem(last=False)
    return prog


def module_out_norm(arch):
    """The Softmax / LogSoftmax units of a module with their dims, in registration order: the part
    of compiled_program's key that sees such a (parameter-free) unit added, removed or replaced."""
    return tuple((type(m).__name__, getattr(m, "dim", None)) for m in arch.modules()
                 if type(m).__name__ in ("Softmax", "LogSoftmax"))


def check_class_request(out_col, classes):
    """out_col: None (the legacy single-output extraction) or an int >= 0; classes: None or "all"."""
    if classes not in (None, "all"):
        raise ValueError(f"classes must be None or 'all', got {classes!r}")
    if out_col is not None and (isinstance(out_col, bool) or not isinstance(out_col, int) or out_col < 0):
        raise ValueError(f"out_col must be an int >= 0, got {out_col!r}")


def pick_classes(out, rows, out_col, classes):
    """The requested class columns of a module output for `rows` output rows: out [rows, C] (or
    [rows], C = 1) -> [rows] for class out_col, [rows, C] for classes="all".  ValueError when the
    class is outside [0, C): C is the module's own output width."""
    if out.dim() == 1:
        out = out.reshape(-1, 1)
    if out.dim() != 2 or out.shape[0] != rows:
        raise RuntimeError(f"model output {tuple(out.shape)} has no [{rows}, classes] form")
    if classes == "all":
        return out.float()
    c = 0 if out_col is None else out_col
    if c >= out.shape[1]:
        raise ValueError(f"target class {c} outside [0, {out.shape[1]}): the model has "
                         f"{out.shape[1]} output column(s)")
    return out[:, c].float()


def build_plan(arch, feat, edge_index, queries, node_type=None, edge_type=None,
               node_type_names=None, edge_type_names=None, padded_dims=None, module_state=None,
               attention=False, edge_weight=None, edge_attr=None, out_col=None, classes=None):
    """ForwardPlan for `arch` on the (sub)graph, or None when the engine cannot run it.
    `attention=True` (opt-in, Explainer params["attention_engine"]) also compiles GATConv,
    GATv2Conv and TransformerConv relations, which otherwise run on the generic torch path.

    A stack of RGCNConv / FastRGCNConv layers (the 4-argument call arch(x, edge_index, node_types,
    edge_types), model.py:102-112) takes `edge_type` as its relations, with or without
    `edge_type_names`; every other program ignores the types of a graph without names, as before.

    Multi-node-type graphs (model.py:118-253): the program's terms are gated by destination
    node type and the query is the reference's `out[sub_ind, 0]` — row sub_ind of the output
    node type's block — so `queries` are positions inside that type and are mapped to subgraph
    nodes here.  The plan is marked `multi_type` (its per-row outputs then go through
    `multi_type_targets`).

    `edge_weight` ([E], one per edge of `edge_index`; homogeneous graphs): the arch is compiled
    for a weighted graph (GCNConv / GraphConv only) and the plan carries the weights.  A weight
    vector that is itself invalid (wrong length, not finite, negative with a GCNConv) raises
    ValueError: no path could run it.

    `edge_attr` ([E, D] or [E], one row per edge of `edge_index`; homogeneous graphs): the arch is
    compiled for a graph with edge features (GINEConv only) and the plan carries the rows.
    Attributes that are themselves invalid (wrong row count, integer, not finite) raise ValueError.

    `out_col` = c (None: column 0) / `classes` = "all": the class column(s) the plan returns
    (engine.ForwardPlan).  A class outside the compiled program's [0, C) raises ValueError: no path
    could return it."""
    check_class_request(out_col, classes)
    multi = node_type_names is not None and node_type is not None and \
        len(torch.unique(node_type)) >= 2
    hetero = edge_type_names is not None and edge_type is not None
    if edge_weight is not None:
        require_edge_weight_arch(arch)
        if multi or hetero or node_type is not None or edge_type is not None:
            raise NotImplementedError("edge_weight on a heterogeneous (typed) graph is not supported")
        edge_weight = checked_edge_weight(arch, edge_weight, edge_index.shape[1])
    if edge_attr is not None:
        if edge_weight is not None:
            raise NotImplementedError("edge_attr together with edge_weight is not supported")
        require_edge_attr_arch(arch)
        if multi or hetero or node_type is not None or edge_type is not None:
            raise NotImplementedError("edge_attr on a heterogeneous (typed) graph is not supported")
        edge_attr = engine.check_edge_attr(edge_attr, edge_index.shape[1])
    try:
        prog = compiled_program(arch, edge_type_names if hetero else None,
                                node_type_names if multi else None, module_state,
                                attention=attention, edge_weight=edge_weight is not None,
                                edge_attr=edge_attr is not None)
        check_rel_features(prog, feat)
    except UnsupportedArch as e:
        warnings.warn(f"engine cannot compile arch ({e}); using the generic torch path")
        return None
    if prog.link_act is not None:
        raise ValueError("a LinkModel scores edges: explain it with problem='edge_prediction' "
                         "and params['edge_masks'] = True")
    if out_col is not None and out_col >= prog.n_classes:
        raise ValueError(f"target class {out_col} outside [0, {prog.n_classes}): the model has "
                         f"{prog.n_classes} output column(s)")
    x = feat
    nt = None
    if prog.pool is not None:
        # graph-level readout: every node is a target of the last layer (every frontier is the
        # whole graph), the plan has one output per mask row and `queries` selects nothing
        queries = range(feat.shape[0])
    if multi:
        nt = node_type.long().reshape(-1)
        rows_t = torch.where(nt == prog.out_type)[0].cpu()
        queries = [int(q) for q in queries]
        if any(q >= rows_t.numel() for q in queries):
            raise IndexError("query index beyond the output node type's rows (model.py:247)")
        queries = [int(rows_t[q]) for q in queries]
    elif hetero and padded_dims is not None and padded_dims[0] > 0:
        x = feat[:, :feat.shape[1] - padded_dims[0]]
    try:
        typed = typed_relations(prog)
        if typed:
            # RGCNConv stacks: the relations are the edge types, named or not
            rels = typed_relation_edges(edge_index, edge_type, typed)
        else:
            rels = relation_edges(edge_index, edge_type if hetero else None,
                                  len(edge_type_names) if hetero else 1)
        plan = engine.ForwardPlan(prog, x, rels, queries, node_type=nt, edge_weight=edge_weight,
                                  edge_attr=edge_attr, out_col=out_col, classes=classes)
    except ValueError as e:
        warnings.warn(f"engine plan rejected ({e}); using the generic torch path")
        return None
    plan.multi_type = multi
    return plan


def build_edge_plan(arch, feat, edge_index, u, v, module_state=None, edge_type=None,
                    label_type=None):
    """ForwardPlan of an edge problem (edge masks, Data.perturb_edge data.py:500-554): mask
    columns = the subgraph's edges, output = the LinkModel decoder's score of edge (u, v).
    None when the engine cannot compile `arch` (generic torch path).

    A typed-relation program (nn.RelLinkModel over RGCNConv layers) takes `edge_type` (one type
    per subgraph edge) as its relations and `label_type`, the query edge's type, which picks the
    DistMult decoder's relation embedding."""
    try:
        prog = compiled_program(arch, state=module_state)
        check_rel_features(prog, feat)
    except UnsupportedArch as e:
        warnings.warn(f"engine cannot compile arch ({e}); using the generic torch path")
        return None
    if prog.link_act is None:
        warnings.warn("edge masks need an edge-level model (nn.LinkModel); using the generic "
                      "torch path")
        return None
    queries, link = ([u, v], (0, 1, prog.link_act)) if u != v else ([u], (0, 0, prog.link_act))
    cols = torch.arange(edge_index.shape[1], device=edge_index.device)
    try:
        typed = typed_relations(prog)
        if typed:
            # each relation's edges in edge order, with their positions in the subgraph's edge
            # list (the mask columns) in that same order
            rels, order = typed_relation_edges(edge_index, edge_type, typed, return_order=True)
            ecols = list(torch.split(order, [e.shape[1] for e in rels]))
            d = None
            if prog.link_rel is not None:
                if label_type is None or not 0 <= int(label_type) < prog.link_rel.shape[0]:
                    raise ValueError("the query edge's type is missing or has no relation embedding")
                d = prog.link_rel[int(label_type)]
            return engine.ForwardPlan(prog, feat, rels, queries, edge_cols=ecols, link=link + (d,))
        return engine.ForwardPlan(prog, feat, [edge_index], queries, edge_cols=[cols], link=link)
    except ValueError as e:
        warnings.warn(f"engine plan rejected ({e}); using the generic torch path")
        return None


def generic_edge_outputs(arch, feat, edge_index, mask, u, v, max_rows=None, edge_type=None,
                         label_type=None):
    """Edge problem through the user's module (torch, on the device): the B-fold union graph of
    Data.perturbator with perturb_edge (data.py:591-648, 500-554: copy b keeps edge e iff
    mask[b, e], copy-major order, node ids shifted by b * N) and `arch(x, ei,
    edge_label_index=...)` scoring each copy's (u, v) -> y [B].

    With `edge_type` (one type per edge) and `label_type` (the query edge's type) the module is a
    typed link model (nn.RelLinkModel) and is called `arch(x, ei, None, et, edge_label_index=...,
    edge_label_type=...)`: the kept edges' types follow the kept edges."""
    B, _ = mask.shape
    N = feat.shape[0]
    step = B if max_rows is None else max_rows
    typed = edge_type is not None and label_type is not None
    if typed:
        edge_type = edge_type.reshape(-1).to(edge_index.device)
    ys = []
    for b0 in range(0, B, step):
        m = mask[b0:b0 + step]
        nb = m.shape[0]
        rows, cols = torch.nonzero(m, as_tuple=True)
        ei = edge_index[:, cols] + rows * N
        x = feat.repeat(nb, 1).float()
        off = torch.arange(nb, device=feat.device) * N
        eli = torch.stack([off + u, off + v])
        with torch.no_grad():
            if typed:
                lt = torch.full((nb,), int(label_type), dtype=torch.long, device=feat.device)
                out = arch(x, ei, None, edge_type[cols], edge_label_index=eli, edge_label_type=lt)
            else:
                out = arch(x, ei, edge_label_index=eli)
            ys.append(out.reshape(-1).float())
    return torch.cat(ys)


def verify_edge_plan(plan, arch, feat, edge_index, u, v, rows=8, tol=1e-4, edge_type=None,
                     label_type=None):
    """The compiled edge plan against the user's module on a few random edge masks."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    mask = (torch.rand((rows, edge_index.shape[1]), generator=g) < 0.5).to(feat.device)
    mask[0] = True
    ref = generic_edge_outputs(arch, feat, edge_index, mask, u, v, edge_type=edge_type,
                               label_type=label_type)
    got = plan.forward(engine.pack_masks(mask))[:, 0]
    err = (ref - got).abs().max().item()
    return err <= tol * max(1.0, ref.abs().max().item()), err


def empty_copy_rows(bits, cols, edge_index):
    """bool [rows]: mask rows that keep no edge of the (sub)graph — the reference's
    multi-node-type loop outputs 0 for such copies instead of running the model
    (model.py:213-215).  One HIP pass over the rows (engine.rows_no_edge)."""
    rows, E = bits.shape[0], edge_index.shape[1]
    if E == 0:
        return torch.ones(rows, dtype=torch.bool, device=bits.device)
    return engine.rows_no_edge(bits, cols, edge_index[0], edge_index[1])


def multi_type_targets(y_rows, empty, batch, sub_ind, S, q4=True):
    """Regression targets of a multi-node-type repeat from per-row engine outputs.
    Copies without edges give 0 (model.py:213-215).  With q4 (the reference's behaviour,
    SURVEY.md quirk Q4) each batch's [B] outputs are cut again by
    extract_node_edge_output(out, sub_ind, S) (wlm.py:435-436): the one surviving value is
    the target of every row of the batch; q4=False keeps the per-copy outputs."""
    y = torch.where(empty, torch.zeros_like(y_rows), y_rows)
    if not q4:
        return y
    out = torch.empty_like(y)
    nfull = y.shape[0] // batch
    if nfull and sub_ind < batch <= S + sub_ind:
        # every full batch keeps exactly one value, row sub_ind: one vectorised broadcast
        out[:nfull * batch] = y[:nfull * batch].view(nfull, batch)[:, sub_ind:sub_ind + 1] \
            .expand(nfull, batch).reshape(-1)
        start = nfull * batch
    else:
        start = 0
    for r0 in range(start, y.shape[0], batch):
        yb = y[r0:r0 + batch]
        sel = yb[sub_ind::S]
        if sel.numel() == yb.numel():
            out[r0:r0 + batch] = sel
        elif sel.numel() == 1:
            out[r0:r0 + batch] = sel.expand(yb.numel())
        else:
            raise RuntimeError("model output does not broadcast against the mask batch "
                               "(the reference's weighted_mse_loss would fail here too)")
    return out


def pooled_call(arch):
    """True for a graph-level model: a forward of three parameters (x, edge_index, batch), the
    form Model.infer calls with the union graph's copy index per node (nn.PooledModel).  An
    optional `edge_weight` or `edge_attr` keyword is no part of the form."""
    forward = getattr(arch, "forward", None)
    if forward is None:
        return False
    try:
        names = [n for n in inspect.signature(forward).parameters if n not in ("edge_weight", "edge_attr")]
    except (TypeError, ValueError):
        return False
    return len(names) == 3 and names[2] != "edge_label_index"


def checked_edge_weight(arch, edge_weight, n_edges):
    """The validated host copy (float32 numpy [n_edges]) of a weight vector for `arch`: one finite
    weight per edge, none negative when the arch holds a GCNConv (matched by class name, as
    program.compile_arch matches it).  ValueError otherwise: no path could run such weights."""
    gcn = any(type(m).__name__ == "GCNConv" for m in arch.modules())
    return engine.check_edge_weight(edge_weight, n_edges, gcn)


def require_edge_weight_arch(arch):
    """TypeError unless `arch.forward` has an `edge_weight` parameter (or takes **kwargs): the
    weighted paths call arch(x, edge_index[, batch], edge_weight=w)."""
    try:
        ps = inspect.signature(arch.forward).parameters
    except (TypeError, ValueError, AttributeError):
        raise TypeError("edge_weight given, but arch.forward has no readable signature")
    if "edge_weight" not in ps and not any(p.kind == p.VAR_KEYWORD for p in ps.values()):
        raise TypeError(f"edge_weight given, but {type(arch).__name__}.forward has no edge_weight "
                        "parameter: the model cannot be called on a weighted graph")


def require_edge_attr_arch(arch):
    """TypeError unless `arch.forward` has an `edge_attr` parameter (or takes **kwargs): the paths
    of a graph with edge features call arch(x, edge_index[, batch], edge_attr=ea)."""
    try:
        ps = inspect.signature(arch.forward).parameters
    except (TypeError, ValueError, AttributeError):
        raise TypeError("edge_attr given, but arch.forward has no readable signature")
    if "edge_attr" not in ps and not any(p.kind == p.VAR_KEYWORD for p in ps.values()):
        raise TypeError(f"edge_attr given, but {type(arch).__name__}.forward has no edge_attr "
                        "parameter: the model cannot be called on a graph with edge features")


def generic_outputs(arch, feat, edge_index, mask, element_index, problem, node_type=None,
                    edge_type=None, node_type_names=None, edge_type_names=None,
                    padded_dims=None, batch=None, q4=True, edge_weight=None, edge_attr=None,
                    out_col=None, classes=None):
    """wlm.py:349-436 semantics per batch of mask rows with the user's module in torch.
    Returns y [R] (the regression target of each row; for multi-node-type graphs the
    reference's output[ind::S] collapse, quirk Q4, broadcast over its batch).  A list of
    element indices (single-node-type graphs) returns y [R, Q]: every query's extraction from
    the same union-graph forward.  `edge_weight` ([E], homogeneous graphs): each copy's kept
    edges carry their weights, `arch(x, edge_index[, batch], edge_weight=w)`.  `edge_attr` ([E, D],
    homogeneous graphs): they carry their attribute rows, `arch(..., edge_attr=ea)`.

    `out_col` = c: class column c of the module's own [rows, C] output instead of the legacy
    extraction (which needs a single-output module); `classes` = "all": every column, y [R, C]
    (a query list: [R, Q * C] in (query, class) order).  The module's output is read as it is, so a
    model that applies a functional softmax in its forward works here.  Single-node-type graphs."""
    check_class_request(out_col, classes)
    by_class = out_col is not None or classes is not None
    pooled = pooled_call(arch)
    if edge_attr is not None:
        if edge_weight is not None:
            raise NotImplementedError("edge_attr together with edge_weight is not supported")
        require_edge_attr_arch(arch)
        if node_type is not None or edge_type is not None:
            raise NotImplementedError("edge_attr on a heterogeneous (typed) graph is not supported")
        edge_attr = torch.as_tensor(edge_attr)
        edge_attr = (edge_attr.reshape(-1, 1) if edge_attr.dim() == 1 else edge_attr).to(
            device=mask.device, dtype=torch.float32)
    if edge_weight is not None:
        require_edge_weight_arch(arch)
        if node_type is not None or edge_type is not None:
            raise NotImplementedError("edge_weight on a heterogeneous (typed) graph is not supported")
        edge_weight = edge_weight.reshape(-1).to(device=mask.device, dtype=torch.float32)
    if isinstance(element_index, (list, tuple)):
        if pooled:
            raise ValueError("a pooled (graph-level) model has one output per graph: no query list")
        return _generic_multi(arch, feat, edge_index, mask, element_index, problem, node_type,
                              edge_type, node_type_names, edge_type_names, padded_dims, batch,
                              edge_weight, edge_attr, out_col, classes)
    data = Data(feat, edge_index)
    mc = Model(arch)
    R, S = mask.shape
    batch = R if batch is None else batch
    ys = []
    for r0 in range(0, R, batch):
        mb = mask[r0:r0 + batch]
        B = mb.shape[0]
        pew = pea = None
        if edge_attr is not None:
            cf, cnt, pei, pet, pea = data.perturbator(mb, problem, node_type, edge_type, edge_attr=edge_attr)
        elif edge_weight is not None:
            cf, cnt, pei, pet, pew = data.perturbator(mb, problem, node_type, edge_type, edge_weight)
        else:
            cf, cnt, pei, pet = data.perturbator(mb, problem, node_type, edge_type)
        pei = pei.long()
        n_types = 1 if node_type_names is None else len(torch.unique(node_type))
        if node_type is not None and edge_type is not None and node_type_names is not None \
                and edge_type_names is not None and n_types < 2:
            cf = data.homo2hetero(cf, cnt, node_type_names, padded_dims)
            pei = data.homo2hetero(pei, pet, edge_type_names)
        if pooled:
            # graph-level model: copy b's S nodes are graph b of the union graph (no node is ever
            # removed), one output row per copy; column out_col (0) is the regression target
            # (cf is a dict for a single-node-type graph with type names: the device is the mask's)
            gb = torch.arange(B, device=mb.device).repeat_interleave(S)
            out = mc.infer(cf, pei, batch=gb, edge_weight=pew, edge_attr=pea)
            if out.dim() != 2 or out.shape[0] != B:
                raise RuntimeError(f"a pooled model must return [{B}, out], got {tuple(out.shape)}")
            ys.append(pick_classes(out, B, out_col, classes) if by_class else out[:, 0].reshape(-1).float())
            continue
        if by_class and n_types >= 2:
            # the reference's multi-node-type extraction reads column 0 (model.py:247)
            if out_col or classes is not None:
                raise NotImplementedError("class columns on a multi-node-type graph are not supported")
            by_class = False
        if n_types < 2:
            out = mc.infer(cf, pei, cnt, pet, edge_weight=pew, edge_attr=pea)
        else:
            # one arch call over the disjoint union per node type (§8f2); HETERO_BATCHED =
            # False restores the reference's per-copy loop
            out = None
            if HETERO_BATCHED:
                out = mc.predict_hetero_output_batched(cf, pei, cnt, pet, node_type_names,
                                                       edge_type_names, B, S, element_index,
                                                       padded_dims, problem)
            if out is None:
                out = mc.predict_hetero_output(cf, pei, cnt, pet, node_type_names,
                                               edge_type_names, B, S, element_index,
                                               padded_dims, problem)
        if node_type is not None and edge_type is not None and isinstance(out, dict):
            out, _ = mc.hetero2homo_output(out)
        if element_index is not None and (q4 or n_types < 2):
            out = mc.extract_node_edge_output(out, element_index, S)
        if by_class:
            ys.append(pick_classes(out, B, out_col, classes))
            continue
        out = out.reshape(-1).float()
        if out.numel() == B:
            ys.append(out)
        elif out.numel() == 1:
            ys.append(out.expand(B))
        else:
            raise RuntimeError("model output does not broadcast against the mask batch "
                               "(the reference's weighted_mse_loss would fail here too)")
    return torch.cat(ys)


def _generic_multi(arch, feat, edge_index, mask, queries, problem, node_type, edge_type,
                   node_type_names, edge_type_names, padded_dims, batch, edge_weight=None,
                   edge_attr=None, out_col=None, classes=None):
    """generic_outputs for several queries of a single-node-type graph: [R, Q] ([R, Q * C] with
    classes="all", (query, class) order)."""
    by_class = out_col is not None or classes is not None
    data = Data(feat, edge_index)
    mc = Model(arch)
    R, S = mask.shape
    batch = R if batch is None else batch
    ys = []
    for r0 in range(0, R, batch):
        mb = mask[r0:r0 + batch]
        B = mb.shape[0]
        pew = pea = None
        if edge_attr is not None:
            cf, cnt, pei, pet, pea = data.perturbator(mb, problem, node_type, edge_type, edge_attr=edge_attr)
        elif edge_weight is not None:
            cf, cnt, pei, pet, pew = data.perturbator(mb, problem, node_type, edge_type, edge_weight)
        else:
            cf, cnt, pei, pet = data.perturbator(mb, problem, node_type, edge_type)
        pei = pei.long()
        if node_type is not None and edge_type is not None and node_type_names is not None \
                and edge_type_names is not None:
            cf = data.homo2hetero(cf, cnt, node_type_names, padded_dims)
            pei = data.homo2hetero(pei, pet, edge_type_names)
        out = mc.infer(cf, pei, cnt, pet, edge_weight=pew, edge_attr=pea)
        if isinstance(out, dict):
            out, _ = mc.hetero2homo_output(out)
        if by_class:
            ys.append(torch.stack([pick_classes(mc.extract_node_edge_output(out, int(q), S), B, out_col,
                                                classes) for q in queries], 1).reshape(B, -1))
            continue
        ys.append(torch.stack([mc.extract_node_edge_output(out, int(q), S).reshape(-1).float()
                               for q in queries], 1).reshape(B, len(queries)))
    return torch.cat(ys)


def verify_plan(plan, arch, feat, edge_index, query, node_type=None, edge_type=None,
                node_type_names=None, edge_type_names=None, padded_dims=None, rows=8, tol=1e-4,
                edge_weight=None, edge_attr=None):
    """Check the compiled program against the user's module on a few random masks (guards the
    registration-order lowering in program.compile_arch).  `query` may be the list of a
    multi-query plan's queries: every output column is then checked.  The plan's class request
    (its out_col, or classes="all") is the one checked: every requested class."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    S = feat.shape[0]
    mask = (torch.rand((rows, S), generator=g) < 0.5).to(feat.device)
    mask[0] = True
    multi = getattr(plan, "multi_type", False)
    # the class columns of the module's own output; a multi-node-type plan (class 0 only) keeps the
    # reference's extraction
    ckw = {} if multi else {"out_col": getattr(plan, "out_col", 0), "classes": getattr(plan, "classes", None)}
    if isinstance(query, (list, tuple)):
        assert not multi, "multi-query plans are single-node-type"
        ref = generic_outputs(arch, feat, edge_index, mask, list(query), "node", node_type,
                              edge_type, node_type_names, edge_type_names, padded_dims,
                              edge_weight=edge_weight, edge_attr=edge_attr, **ckw)
        got = plan.forward(engine.pack_masks(mask))[:, :ref.shape[1]]
        err = (ref - got).abs().max().item()
        return err <= tol * max(1.0, ref.abs().max().item()), err
    ref = generic_outputs(arch, feat, edge_index, mask, query, "node", node_type, edge_type,
                          node_type_names, edge_type_names, padded_dims, q4=not multi,
                          edge_weight=edge_weight, edge_attr=edge_attr, **ckw)
    bits = engine.pack_masks(mask)
    got = plan.forward(bits)
    got = got if ref.dim() == 2 else got[:, 0]
    if multi:  # per-copy outputs on both sides (zero for copies without edges)
        got = torch.where(empty_copy_rows(bits, S, edge_index), torch.zeros_like(got), got)
    err = (ref - got).abs().max().item()
    return err <= tol * max(1.0, ref.abs().max().item()), err


def fit_repeat(bits, cols, batch, y, w0, params):
    """KernelSHAP + surrogate fit for one repeat; returns (w_final, losses[list], best_epoch,
    kernel)."""
    kern = engine.shap_kernel(bits, cols)
    w, losses, best, _, _ = engine.wlm_fit(bits, cols, batch, y, kern, w0, params)
    return w, losses, best, kern
