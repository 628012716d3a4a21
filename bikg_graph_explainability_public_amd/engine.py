"""Device engine: builds receptive-field plans and drives the HIP kernels (libxpgnn.so).

Plan (per query, built once per Explainer.run — DESIGN.md §3):
  F_L = queries; F_{l-1} = F_l ∪ in-neighbours(F_l) (all relations), F_l first so the first
  n_l entries of F_{l-1} are F_l.  Degrees are needed at F_0 (their in-edges reach hop L+1,
  which is why the reference extracts L+1 hops, data.py:325-328).
  Layer-1 tables T_k = X[F_0] W_k^T are computed once by the MFMA dense kernel (features are
  never masked, data.py:582); per mask row only the masked aggregation and the deeper layers
  (aggregate-then-transform on MFMA) run.

All device memory is owned by torch tensors held by the plan; the C-ABI never allocates.
"""
import contextlib
import ctypes
import gc
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import ACT, REL_NORM, TERM, ForwardPlanDesc, HeadDesc, LayerDesc, WlmParams, call, ptr
from .program import fold_attention, relation_weights, stack_attention


def _rup(x, m):
    return ((int(x) + m - 1) // m) * m


def words_of(cols):
    return (int(cols) + 31) // 32


# ----------------------------------------------------------------------------- masks
def pack_masks(mask: torch.Tensor) -> torch.Tensor:
    """bool/uint8 [rows, cols] device tensor -> row bits uint32 [rows, words] (HIP)."""
    _lib.require_device(mask, "mask")
    m = mask.contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    rows, cols = m.shape
    bits = torch.empty((rows, words_of(cols)), dtype=torch.int32, device=m.device)
    call("xpg_pack_masks", ptr(m), rows, cols, ptr(bits), _lib.stream_of(m.device))
    return bits


def unpack_masks(bits: torch.Tensor, cols: int) -> torch.Tensor:
    _lib.require_device(bits, "bits")
    rows = bits.shape[0]
    out = torch.empty((rows, cols), dtype=torch.uint8, device=bits.device)
    call("xpg_unpack_masks", ptr(bits), rows, cols, ptr(out), _lib.stream_of(bits.device))
    return out.view(torch.bool)


class CaptureTopologyError(RuntimeError):
    """A stream dependency inside a HIP-graph capture that this HIP stack cannot end."""


@contextlib.contextmanager
def capture_guard():
    """Wrap every HIP-graph capture of the hot path (`with capture_guard(), torch.cuda.graph(g)`).

    1. Freeing a captured graph while another capture runs aborts the process on this HIP stack
       (tools/capture_probe.py, variant graph_gc, profiles/r3_capture_probe.log: the round-2
       `capture_end` crash of the pipelined bench).  A graph object reachable only from a
       reference cycle is freed whenever Python's cyclic collector runs, which can be
       mid-capture; the guard collects first and holds the collector off until the capture
       ends.  The graphs themselves must stay referenced by the caller.
    2. Two side streams that wait on each other in turn segfault hipStreamEndCapture (minimal
       construct, tools/capture_probe.py `pingpong`, profiles/r6_capture_bisect.log: A works;
       B waits A, works; A waits B, works; all joined): the guard tracks the capture's stream
       waits (Stream.wait_stream, Stream.wait_event on a recorded Event) and refuses a wait of
       side stream X on side stream Y once Y has waited on X, with CaptureTopologyError, before
       the wait is made; the side streams are joined to the capture's origin stream first, so
       the capture still ends cleanly (and its graph is not used).  Waits between the origin
       stream (the one current at the first wait) and a side stream are free in both
       directions (the bench's pipelined lanes alternate them)."""
    gc.collect()
    enabled = gc.isenabled()
    gc.disable()
    st = {"origin": None, "waited": {}, "streams": {}, "events": {}}
    S, E = torch.cuda.Stream, torch.cuda.Event
    orig_ws, orig_we, orig_rec = S.wait_stream, S.wait_event, E.record

    def note(x, y):  # stream x is about to wait on stream y
        if not torch.cuda.is_current_stream_capturing():
            return
        if st["origin"] is None:
            cur = torch.cuda.current_stream()
            st["origin"] = cur.cuda_stream
            st["streams"][cur.cuda_stream] = cur
        kx, ky = x.cuda_stream, y.cuda_stream
        st["streams"].setdefault(kx, x)
        st["streams"].setdefault(ky, y)
        if kx == ky:
            return
        o = st["origin"]
        if kx != o and ky != o and kx in st["waited"].get(ky, ()):
            origin = st["streams"][o]
            for k, s_ in st["streams"].items():
                if k != o:
                    orig_ws(origin, s_)
            raise CaptureTopologyError(
                "graph capture: side stream waits on a side stream that waited on it earlier in "
                "the capture (A -> B -> A); hipStreamEndCapture segfaults on such a capture on "
                "this HIP stack (tools/capture_probe.py pingpong).  Route the second wait through "
                "the capture's origin stream.")
        st["waited"].setdefault(kx, set()).add(ky)

    def wait_stream(self, stream):
        note(self, stream)
        return orig_ws(self, stream)

    def wait_event(self, event):
        src = st["events"].get(id(event))
        if src is not None:
            note(self, src)
        return orig_we(self, event)

    def record(self, stream=None):
        st["events"][id(self)] = stream if stream is not None else torch.cuda.current_stream()
        return orig_rec(self, stream)

    S.wait_stream, S.wait_event, E.record = wait_stream, wait_event, record
    try:
        yield
    finally:
        S.wait_stream, S.wait_event, E.record = orig_ws, orig_we, orig_rec
        if enabled:
            gc.enable()


def sample_shapley(seed: int, rows: int, cols: int, device, row_offset: int = 0,
                   with_counts: bool = False):
    """Device Shapley masks (masks.py:231-260 distribution: iid Bernoulli(1/2) bits).

    with_counts=True also returns the per-row popcounts (int32 [rows]) accumulated while
    sampling, for `shap_kernel(..., counts=...)`."""
    bits = torch.empty((rows, words_of(cols)), dtype=torch.int32, device=device)
    st = _lib.stream_of(torch.device(device))
    seed_c = ctypes.c_uint64(int(seed) & (2 ** 64 - 1))
    if not with_counts:
        call("xpg_sample_shapley", seed_c, row_offset, rows, cols, ptr(bits), st)
        return bits
    counts = torch.empty(rows, dtype=torch.int32, device=device)
    call("xpg_sample_shapley_counts", seed_c, row_offset, rows, cols, ptr(bits), ptr(counts), st)
    return bits, counts


def sample_shapley_sets(seeds, rows: int, cols: int, device):
    """len(seeds) independent `sample_shapley(seed, rows, cols)` draws as one [n, rows, words]
    tensor, in one native call (Explainer.run's repeats)."""
    n = len(seeds)
    bits = torch.empty((n, rows, words_of(cols)), dtype=torch.int32, device=device)
    arr = (ctypes.c_uint64 * max(n, 1))(*[int(s) & (2 ** 64 - 1) for s in seeds])
    call("xpg_sample_shapley_sets", arr, n, rows, cols, ptr(bits), _lib.stream_of(torch.device(device)))
    return bits


SAMPLER_SHAPLEY, SAMPLER_COMMUNITIES = 0, 1


def sampler_describe(kind: int, rows: int, cols: int, n_comm: int = 0, n_blocks: int = 0) -> str:
    """The kernel a device sampler launches for a shape under the current XPG_* switches
    (xpg_sampler_describe, a host query; the launchers make the same selection):
    `k_shapley_flat<ALIGN> grid=NBx1` / `k_shapley<ALIGN> grid=GXxGY` for kind = SAMPLER_SHAPLEY
    (`sample_shapley*`), `k_communities<SMALL,STAGED,CM> grid=NB lds=BYTES` for kind =
    SAMPLER_COMMUNITIES (`sample_communities` of n_comm communities in n_blocks plan blocks)."""
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.load().xpg_sampler_describe(kind, rows, cols, n_comm, n_blocks, buf, len(buf)))
    return buf.value.decode()


# torch.get_rng_state() of the CPU generator (at::CPUGeneratorImplState, legacy POD first):
# uint64 the_initial_seed | int32 left | int32 seeded | uint64 next | uint64 state[624] | ...
_RNG_LEFT, _RNG_NEXT, _RNG_STATE = 8, 16, 24


def compat_shapley_bits(rows: int, cols: int):
    """torch.randint(0, 2, (rows, cols), dtype=torch.bool) on torch's global CPU generator
    (masks.py:231-260), bit-identical, as bit-packed int32 [rows, ceil(cols / 32)] rows in host
    memory (pinned when a GPU is present), with the generator advanced past the draw exactly as
    torch would advance it: the library replays the generator's MT19937 state natively
    (xpg_mt19937_mask_bits, host code), without the [rows, cols] bool tensor."""
    raw, state, left, nxt = _rng_get()
    out = torch.empty((rows, words_of(cols)), dtype=torch.int32,
                      pin_memory=torch.cuda.is_available())
    call("xpg_mt19937_mask_bits", state.ctypes.data, left.ctypes.data, nxt.ctypes.data, int(rows),
         int(cols), out.data_ptr() if rows else None)
    _rng_set(raw, state, left, nxt)
    return out


_DRAWS_FORM = []  # [form] once probed: 0 / 1 (see _draws_form), None = no native form matches


def _draws_form():
    """How this torch build evaluates ATen's CPU uniform_real, x * (to - from) + from in float:
    as written (0) or contracted into one fused multiply-add (1) — the ATen kernels compiled for
    an FMA-capable CPU capability contract it, the DEFAULT build does not.  Probed once on a
    private generator (the global one is untouched) against both native forms; None when
    neither reproduces torch (the caller then draws through torch itself)."""
    if not _DRAWS_FORM:
        form = None
        g = torch.Generator().manual_seed(20260101)
        st = g.get_state()
        ref_seed = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        ref = torch.empty(1000).uniform_(-0.3, 0.3, generator=g)
        torch.empty((), dtype=torch.int64).random_(generator=g)
        ref_next = torch.rand(3, generator=g)
        for f in (1, 0):
            raw = st.numpy().copy()
            left = raw[_RNG_LEFT:_RNG_LEFT + 4].view(np.int32).copy()
            nxt = np.array([int(raw[_RNG_NEXT:_RNG_NEXT + 8].view(np.uint64)[0])], dtype=np.int32)
            state = raw[_RNG_STATE:_RNG_STATE + 624 * 8].view(np.uint64).astype(np.uint32)
            seeds = np.empty(1, dtype=np.int64)
            w = torch.empty(1000)
            call("xpg_mt19937_repeat_draws", state.ctypes.data, left.ctypes.data, nxt.ctypes.data, 1,
                 1000, -0.3, 0.3, f, seeds.ctypes.data, w.data_ptr())
            raw[_RNG_LEFT:_RNG_LEFT + 4] = left.view(np.uint8)
            raw[_RNG_NEXT:_RNG_NEXT + 8] = np.array([nxt[0]], dtype=np.uint64).view(np.uint8)
            raw[_RNG_STATE:_RNG_STATE + 624 * 8] = state.astype(np.uint64).view(np.uint8)
            g2 = torch.Generator()
            g2.set_state(torch.from_numpy(raw))
            if int(seeds[0]) == ref_seed and torch.equal(w, ref) and \
                    torch.equal(torch.rand(3, generator=g2), ref_next):
                form = f
                break
        _DRAWS_FORM.append(form)
    return _DRAWS_FORM[0]


def repeat_draws(times: int, S: int, fma: int = None):
    """Explainer.run's per-repeat draws on torch's global CPU generator with the device Shapley
    sampler, in the reference's order (explainer.py:490-519), replayed natively
    (xpg_mt19937_repeat_draws, host code): per repeat the sampler seed
    torch.randint(0, 2**62, (1,)), LinearRegression(S)'s initial weights (wlm.py:40-45:
    kaiming_uniform_(a=sqrt(5)) = uniform_(-bound, bound)) and the DataLoader iterator's seed
    draw.  Returns (seeds: list of int, w0: float32 [times, S] host tensor); the generator is
    left exactly where the torch calls leave it.  Returns None (nothing drawn) when this torch
    build's uniform_ rounding matches neither native form (`_draws_form`)."""
    from .wlm import LinearRegression
    if fma is None:
        fma = _draws_form()
        if fma is None:
            return None
    bound = LinearRegression.init_bound(S)
    seeds = np.empty(max(times, 1), dtype=np.int64)
    w0 = torch.empty((times, S), dtype=torch.float32)
    raw, state, left, nxt = _rng_get()
    call("xpg_mt19937_repeat_draws", state.ctypes.data, left.ctypes.data, nxt.ctypes.data, int(times),
         int(S), -bound, bound, int(fma), seeds.ctypes.data,
         w0.data_ptr() if times and S else None)
    _rng_set(raw, state, left, nxt)
    return seeds[:times].tolist(), w0


def compat_community_bits(cols: int, communities, blocks):
    """The reference's compat community draws (Mask.mask_generator with communities,
    masks.py:299-348 + pathways.py:234-385) on torch's global CPU generator, bit-identical, as
    UNSHUFFLED bit-packed int32 [rows, ceil(cols / 32)] host rows (pinned when a GPU is
    present); the generator is advanced exactly as the reference's torch calls advance it, so
    the caller's row shuffle (torch.randperm) follows on the same stream.  `communities`: every
    community's member columns (each sorted ascending, as the reference sorts them in place);
    `blocks`: int32 [n_blocks, 5] {row_start, size, size_internal, own, b} (Mask.community_plan).
    Host code in the library (xpg_mt19937_community_bits)."""
    blocks = np.ascontiguousarray(np.asarray(blocks), dtype=np.int32).reshape(-1, 5)
    lens = np.fromiter((len(c) for c in communities), dtype=np.int64, count=len(communities))
    ptr_ = np.zeros(lens.size + 1, dtype=np.int32)
    np.cumsum(lens, out=ptr_[1:])
    flat = np.fromiter(itertools.chain.from_iterable(communities), dtype=np.int64,
                       count=int(lens.sum()))
    flat = np.ascontiguousarray(flat if flat.size else np.zeros(1, np.int64), dtype=np.int32)
    rows = int(blocks[-1, 0]) + int(blocks[-1, 1])
    out = torch.empty((rows, words_of(cols)), dtype=torch.int32,
                      pin_memory=torch.cuda.is_available())
    raw, state, left, nxt = _rng_get()
    call("xpg_mt19937_community_bits", state.ctypes.data, left.ctypes.data, nxt.ctypes.data,
         int(cols), int(lens.size), ptr_.ctypes.data, flat.ctypes.data, blocks.ctypes.data,
         int(blocks.shape[0]), rows, out.data_ptr())
    _rng_set(raw, state, left, nxt)
    return out


def _rng_get():
    """torch's CPU generator state as (raw bytes, state[624] uint32, left int32[1], next int32[1])."""
    raw = torch.get_rng_state().numpy().copy()
    left = raw[_RNG_LEFT:_RNG_LEFT + 4].view(np.int32).copy()
    nxt = np.array([int(raw[_RNG_NEXT:_RNG_NEXT + 8].view(np.uint64)[0])], dtype=np.int32)
    state = raw[_RNG_STATE:_RNG_STATE + 624 * 8].view(np.uint64).astype(np.uint32)
    return raw, state, left, nxt


def _rng_set(raw, state, left, nxt):
    """Write an advanced (state, left, next) back into torch's CPU generator."""
    raw[_RNG_LEFT:_RNG_LEFT + 4] = left.view(np.uint8)
    raw[_RNG_NEXT:_RNG_NEXT + 8] = np.array([nxt[0]], dtype=np.uint64).view(np.uint8)
    raw[_RNG_STATE:_RNG_STATE + 624 * 8] = state.astype(np.uint64).view(np.uint8)
    torch.set_rng_state(torch.from_numpy(raw))


def sample_shapley_dev(seed: torch.Tensor, rows: int, cols: int, row_offset: int = 0,
                       out: torch.Tensor = None):
    """`sample_shapley` with the seed read on the device from `seed` (int64 [1], the bits of a
    uint64) when the kernel runs: a captured HIP graph draws new rows on every replay once the
    caller advances the tensor on the stream (xpg_sample_shapley_dev).  `out` (int32
    [rows, words]): write the rows there (no allocation, e.g. on a side stream in a capture)."""
    _lib.require_device(seed, "seed")
    if seed.dtype != torch.int64 or seed.numel() != 1:
        raise ValueError("seed must be a device int64 tensor of one element")
    if out is None:
        bits = torch.empty((rows, words_of(cols)), dtype=torch.int32, device=seed.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (rows, words_of(cols)) or \
            not out.is_contiguous():
        raise ValueError("out must be a contiguous int32 [rows, ceil(cols / 32)] tensor")
    else:
        bits = out
    call("xpg_sample_shapley_dev", ptr(seed), row_offset, rows, cols, ptr(bits),
         _lib.stream_of(seed.device))
    return bits


def community_columns(communities, cols):
    """Column -> community CSR (int32 col_ptr [cols+1], col_comm [nnz]) of a community list."""
    lens = np.array([len(c) for c in communities], dtype=np.int64)
    members = (np.concatenate([np.asarray(c, dtype=np.int64) for c in communities])
               if lens.sum() else np.zeros(0, dtype=np.int64))
    assert members.size == 0 or (members.min() >= 0 and members.max() < cols), \
        "community member outside the mask columns"
    comm = np.repeat(np.arange(len(communities), dtype=np.int64), lens)
    order = np.argsort(members, kind="stable")
    col_ptr = np.zeros(cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(members, minlength=cols), out=col_ptr[1:])
    return (torch.from_numpy(col_ptr.astype(np.int32)),
            torch.from_numpy(comm[order].astype(np.int32)))


def community_tables(plan, communities, cols: int, device, columns=None):
    """Device copies of a community plan (Mask.community_plan) and its column -> community CSR,
    uploaded once and reused by every repeat's `sample_communities(..., tables=...)`."""
    blocks, src_rows, rows, shuffle = plan
    dev = torch.device(device)
    col_ptr, col_comm = columns if columns is not None else community_columns(communities, cols)
    if col_comm.numel() == 0:
        col_comm = torch.zeros(1, dtype=torch.int32)
    up = lambda t: t.to(dev, torch.int32).contiguous()
    return (up(blocks), up(col_ptr), up(col_comm), int(src_rows), int(rows), bool(shuffle),
            len(communities), int(cols))


def sample_communities(seed: int, plan, communities, cols: int, device, columns=None,
                       tables=None, row_offset: int = 0, rows: int = None, out=None):
    """Device community masks (masks.py:81-194, pathways.py:234-385).

    plan = Mask.community_plan(); columns = community_columns(communities, cols); tables =
    community_tables(...) (skips the per-call uploads).  Returns (row bits int32 [rows, words],
    pathway_rows int32 [rows]).  row_offset / rows: only the global rows [row_offset,
    row_offset + rows) of the repeat (a rank's shard; the same rows as the full call's).  out:
    a contiguous int32 [rows, words] view to write the bits into (e.g. one repeat's slice of a
    multi-repeat buffer, instead of a torch.cat of per-repeat draws)."""
    if tables is None:
        tables = community_tables(plan, communities, cols, device, columns)
    blocks, col_ptr, col_comm, src_rows, total, shuffle, n_comm, cols = tables
    rows = total - row_offset if rows is None else rows
    if row_offset < 0 or rows < 0 or row_offset + rows > total:
        raise ValueError(f"community rows [{row_offset}, {row_offset + rows}) outside the "
                         f"repeat's {total} rows")
    dev = blocks.device
    if out is None:
        bits = torch.empty((rows, words_of(cols)), dtype=torch.int32, device=dev)
    else:
        if (out.dtype != torch.int32 or tuple(out.shape) != (rows, words_of(cols))
                or not out.is_contiguous() or out.device != dev):
            raise ValueError(f"out must be a contiguous int32 [{rows}, {words_of(cols)}] tensor "
                             f"on {dev}")
        bits = out
    prow = torch.empty(rows, dtype=torch.int32, device=dev)
    call("xpg_sample_communities_rows", ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), row_offset,
         rows, cols, n_comm, ptr(blocks), blocks.shape[0], src_rows, int(shuffle),
         ptr(col_ptr), ptr(col_comm), ptr(bits), ptr(prow), _lib.stream_of(dev))
    return bits, prow


def edge_keep(bits, cols, src, dst):
    """data.py:390-451 edge mask: [rows * n_edges] bool, copy-major."""
    _lib.require_device(bits, "bits")
    rows = bits.shape[0]
    s = src.to(device=bits.device, dtype=torch.int32).contiguous()
    d = dst.to(device=bits.device, dtype=torch.int32).contiguous()
    keep = torch.empty(rows * s.numel(), dtype=torch.uint8, device=bits.device)
    call("xpg_edge_keep", ptr(bits), rows, cols, ptr(s), ptr(d), s.numel(), ptr(keep),
         _lib.stream_of(bits.device))
    return keep.view(torch.bool)


def rows_no_edge(bits, cols, src, dst):
    """bool [rows]: mask rows that keep no edge (src[e], dst[e] both kept) — the multi-node-type
    loop's empty copies (model.py:213-215), without the rows x edges keep matrix."""
    _lib.require_device(bits, "bits")
    rows = bits.shape[0]
    s = src.to(device=bits.device, dtype=torch.int32).contiguous()
    d = dst.to(device=bits.device, dtype=torch.int32).contiguous()
    out = torch.empty(rows, dtype=torch.uint8, device=bits.device)
    call("xpg_rows_no_edge", ptr(bits), rows, cols, ptr(s), ptr(d), s.numel(), ptr(out),
         _lib.stream_of(bits.device))
    return out.view(torch.bool)


# ----------------------------------------------------------------------------- k-hop subgraph
def khop_subgraph(node_idx: int, num_hops: int, edge_index: torch.Tensor, num_nodes: int):
    """Data.comp_graph's k_hop_subgraph (data.py:331-333; PyG 2.0.4 semantics, relabel_nodes=True,
    flow='source_to_target') on device: (subset int64, relabelled edge_index int64 [2, E_sub],
    inv int64 [1], edge_mask bool [E]).  One host sync (the output sizes)."""
    _lib.require_device(edge_index, "edge_index")
    dev = edge_index.device
    ei = edge_index.to(torch.int64).contiguous()
    E, N, seed = ei.shape[1], int(num_nodes), int(node_idx)
    if not 0 <= seed < N:
        raise IndexError(f"k_hop_subgraph: node {seed} out of range for {N} nodes")
    nbytes = ctypes.c_size_t(0)
    call("xpg_khop_workspace", N, E, ctypes.byref(nbytes))
    ws = _workspace(dev, nbytes.value)
    subset = torch.empty(N, dtype=torch.int64, device=dev)
    sub = torch.empty((2, max(E, 1)), dtype=torch.int64, device=dev)
    emask = torch.empty(E, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    call("xpg_khop_subgraph", ptr(ei), E, N, seed, int(num_hops), ptr(subset), ptr(sub),
         ptr(sub[1]), ptr(emask), ptr(counts), ptr(ws), ws.numel(), _lib.stream_of(dev))
    n_sub, n_e, inv, bad = counts.tolist()
    if bad:
        raise IndexError("k_hop_subgraph: edge_index holds node ids outside [0, num_nodes)")
    # inv: the seed's position, already on the device in counts[2] (no host -> device copy)
    return subset[:n_sub], sub[:, :n_e].contiguous(), counts[2:3], emask.view(torch.bool)


# ----------------------------------------------------------------------------- KernelSHAP
def shap_kernel(bits: torch.Tensor, cols: int, counts: torch.Tensor = None,
                out: torch.Tensor = None, scratch: torch.Tensor = None) -> torch.Tensor:
    """Kernel.compute (kernels.py:115-174) on device: fp64 [rows].  `counts` (row popcounts from
    `sample_shapley(..., with_counts=True)`) skips the popcount pass over the bits.  `out`
    (fp64 [rows]) and `scratch` (int32 [rows], the popcounts) let a caller that launches this on
    a side stream inside a graph capture avoid allocating there."""
    _lib.require_device(bits, "bits")
    rows = bits.shape[0]
    if out is None:
        out = torch.empty(rows, dtype=torch.float64, device=bits.device)
    elif out.dtype != torch.float64 or out.numel() != rows or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 [rows] tensor")
    st = _lib.stream_of(bits.device)
    if counts is None:
        if scratch is None:
            scratch = torch.empty(rows, dtype=torch.int32, device=bits.device)
        elif scratch.dtype != torch.int32 or scratch.numel() != rows or not scratch.is_contiguous():
            raise ValueError("scratch must be a contiguous int32 [rows] tensor")
        counts = scratch
        call("xpg_popcount_rows", ptr(bits), rows, cols, ptr(counts), st)
    else:
        _lib.require_device(counts, "counts")
        if counts.dtype != torch.int32 or counts.numel() != rows:
            raise ValueError("counts must be int32 [rows]")
        counts = counts.contiguous()
    call("xpg_shap_kernel", ptr(counts), rows, cols, ptr(out), st)
    return out


# ----------------------------------------------------------------------------- dense
def dense(A: torch.Tensor, W: torch.Tensor, bias, act=None, n_real=None) -> torch.Tensor:
    """act(A W^T + b) on the fp32 MFMA kernel.  A [M, K] and W [N, K] are zero-padded here."""
    dev = A.device
    M, K = A.shape
    N = W.shape[0] if n_real is None else n_real
    k_pad, n_pad = _rup(K, 8), _rup(max(N, 1), 32)
    Ap = A if (K == k_pad and A.is_contiguous()) else \
        torch.nn.functional.pad(A.float(), (0, k_pad - K)).contiguous()
    Wp = torch.zeros((n_pad, k_pad), dtype=torch.float32, device=dev)
    Wp[:W.shape[0], :K] = W
    bp = torch.zeros(n_pad, dtype=torch.float32, device=dev)
    if bias is not None:
        bp[:bias.shape[0]] = bias
    C = torch.empty((M, n_pad), dtype=torch.float32, device=dev)
    call("xpg_dense", ptr(Ap), M, k_pad, ptr(Wp), k_pad, k_pad, ptr(bp), N, n_pad,
         ACT[act], ptr(C), n_pad, _lib.stream_of(dev))
    return C[:, :N]


# ----------------------------------------------------------------------------- kernel timing
PROF_SLOTS = ("wide_bits", "wide_f0", "wide_degree", "wide_l1", "wide_l2")


def profile_enable(on=True):
    """Per-kernel HIP-event timing of the wide forward path (xpg_profile_enable): measurement
    only, never around a graph capture."""
    _lib.check(_lib.load().xpg_profile_enable(1 if on else 0))


def profile_read():
    """{slot: (device ms summed over launches, launches)} since profile_enable (waits for the
    recorded events; xpg_profile_read)."""
    n = len(PROF_SLOTS)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    _lib.check(_lib.load().xpg_profile_read(ms, cnt, n))
    return {k: (ms[i], cnt[i]) for i, k in enumerate(PROF_SLOTS)}


def wide_variants():
    """Every "l1=<kernel>" / "l2=<kernel>" token ForwardPlan.describe can report for the wide
    path (xpg_wide_variants: the table the library's selection picks from)."""
    buf = ctypes.create_string_buffer(4096)
    _lib.check(_lib.load().xpg_wide_variants(buf, len(buf)))
    return buf.value.decode().split()


def forward_variants():
    """Every instantiation of k_rows_forward, k_fused_forward, k_agg_l1_rows, k_agg and k_dense in
    the library (xpg_forward_variants: the tables the launches pick from), by the names
    ForwardPlan.kernels reports."""
    buf = ctypes.create_string_buffer(4096)
    _lib.check(_lib.load().xpg_forward_variants(buf, len(buf)))
    return buf.value.decode().split()


# ----------------------------------------------------------------------------- readout
def pool_describe(rows: int, n: int, ld: int, kind: str) -> str:
    """The kernel(s) the readout launches for h [rows, n, ld] (xpg_pool_describe, a host query
    sharing the launcher's selection): `k_pool<KIND> parts=1 part_nodes=P`, or
    `k_pool<KIND>+k_pool_finish<KIND> parts=N part_nodes=P` when a row is split (n > P)."""
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.load().xpg_pool_describe(int(rows), int(n), int(ld), _lib.POOL[kind], buf, len(buf)))
    return buf.value.decode()


def pool_workspace_bytes(rows: int, n: int, ld: int) -> int:
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_pool_workspace(int(rows), int(n), int(ld), ctypes.byref(nb)))
    return nb.value


def pool_rows(h: torch.Tensor, kind: str, out: torch.Tensor = None,
              workspace: torch.Tensor = None) -> torch.Tensor:
    """Graph-level readout of h [rows, n, ld] fp32 (ld % 4 == 0, at most 256) -> [rows, ld]:
    column-wise "mean" / "sum" / "max" over each row's n node rows (xpg_pool_rows; the readout of
    a pooled ForwardPlan on its own).  Deterministic: a fixed reduction order that depends on
    (n, ld) only.  `out` / `workspace` (uint8, pool_workspace_bytes): caller-owned buffers."""
    _lib.require_device(h, "h")
    if h.dtype != torch.float32 or h.dim() != 3 or not h.is_contiguous():
        raise ValueError("h must be a contiguous float32 [rows, n, ld] tensor")
    rows, n, ld = h.shape
    if out is None:
        out = torch.empty((rows, ld), dtype=torch.float32, device=h.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, ld) or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [rows, ld] tensor")
    need = pool_workspace_bytes(rows, n, ld)
    if workspace is None:
        workspace = _workspace(h.device, need) if need else None
    elif workspace.dtype != torch.uint8 or workspace.numel() < need:
        raise ValueError("workspace must be a uint8 device tensor of pool_workspace_bytes")
    call("xpg_pool_rows", ptr(h), rows, n, ld, _lib.POOL[kind], ptr(out), ptr(workspace),
         workspace.numel() if workspace is not None else 0, _lib.stream_of(h.device))
    return out


# ----------------------------------------------------------------------------- class readout
def class_out_rows(z: torch.Tensor, n_real: int, kind=None, col: int = -1,
                   out: torch.Tensor = None) -> torch.Tensor:
    """The class readout of z [M, ld] fp32 (ld % 4 == 0, at most 256; the first n_real columns are
    the classes, the rest padding that is never read as a value) on its own (xpg_class_out_rows;
    the tail of a ForwardPlan with a class readout): `kind` None / "softmax" / "log_softmax" over
    the n_real columns, then class `col` -> [M], or every class (col = -1) -> [M, n_real].
    Deterministic: a row's result depends on its values and (n_real, ld) alone."""
    _lib.require_device(z, "z")
    if z.dtype != torch.float32 or z.dim() != 2 or not z.is_contiguous():
        raise ValueError("z must be a contiguous float32 [M, ld] tensor")
    M, ld = z.shape
    shape = (M,) if col >= 0 else (M, int(n_real))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=z.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {list(shape)} tensor")
    call("xpg_class_out_rows", ptr(z), M, ld, int(n_real), _lib.CLASS_KIND[kind], int(col), ptr(out),
         _lib.stream_of(z.device))
    return out


# ----------------------------------------------------------------------------- post-op
def _post_record(ld, norm, eps, act, residual, vecs, device, keep):
    pd = _lib.PostDesc(norm=_lib.NORM[norm], eps=float(eps), act=ACT[act], residual=int(bool(residual)))
    for name, v in vecs.items():
        if v is None:
            continue
        vp = _pad_vec(torch.as_tensor(v).reshape(-1), ld, device)
        keep.append(vp)
        setattr(pd, name, vp.data_ptr())
    return pd


def post_describe(M: int, ld: int, f_out: int, norm=None, residual=False) -> str:
    """The kernel post_rows launches for h [M, ld] (xpg_post_describe, a host query sharing the
    launcher's selection): `k_post<NORM,RES> group=G rows_per_wave=R`."""
    pd = _lib.PostDesc(norm=_lib.NORM[norm], eps=1.0, residual=int(bool(residual)))
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.load().xpg_post_describe(int(M), int(ld), int(f_out), ctypes.byref(pd), buf, len(buf)))
    return buf.value.decode()


def post_rows(h: torch.Tensor, f_out: int, scale=None, shift=None, norm=None, gamma=None, beta=None,
              eps=1e-5, act=None, hprev: torch.Tensor = None, tgt_prev: torch.Tensor = None):
    """One conv layer's post-op in place on h [M, ld] fp32 (xpg_post_rows; k_post on its own):
    h * scale + shift, norm "layer" over the first f_out columns with gamma / beta / eps, act, and
    with `hprev` [rows, n_prev, ld_prev] and `tgt_prev` int32 [n_tgt] (M = rows * n_tgt) the skip
    + hprev[r, tgt_prev[t]]; columns f_out.. come out 0.  The vectors hold f_out entries (or None).
    Returns h."""
    _lib.require_device(h, "h")
    if h.dtype != torch.float32 or h.dim() != 2 or not h.is_contiguous():
        raise ValueError("h must be a contiguous float32 [M, ld] tensor")
    M, ld = h.shape
    res = hprev is not None
    if res:
        if hprev.dtype != torch.float32 or hprev.dim() != 3 or not hprev.is_contiguous() or \
                tgt_prev is None or tgt_prev.dtype != torch.int32 or hprev.device != h.device or \
                tgt_prev.device != h.device:
            raise ValueError("hprev must be a contiguous float32 [rows, n_prev, ld_prev] tensor and "
                             "tgt_prev an int32 tensor, both on h's device")
        rows, n_prev, ld_prev = hprev.shape
        n_tgt = tgt_prev.numel()
        if n_tgt == 0 or M != rows * n_tgt or \
                (n_tgt and (int(tgt_prev.min()) < 0 or int(tgt_prev.max()) >= n_prev)):
            raise ValueError("M must be rows * len(tgt_prev) and tgt_prev must index hprev's rows")
    else:
        n_prev = ld_prev = n_tgt = 0
    keep = []
    pd = _post_record(ld, norm, eps, act, res, {"scale": scale, "shift": shift, "gamma": gamma,
                                                "beta": beta}, h.device, keep)
    call("xpg_post_rows", ptr(h), M, ld, int(f_out), ctypes.byref(pd), ptr(hprev), ld_prev, n_tgt,
         n_prev, ptr(tgt_prev), _lib.stream_of(h.device))
    return h


# ----------------------------------------------------------------------------- forward plan
def plan_arrays(S, rel_np, queries, L, rel_eid=None):
    """Receptive-field frontiers and CSR arrays of a ForwardPlan, built on the host by the
    library (xpg_plan_arrays_build / _take, include/xpgnn.h): the same arrays as
    `plan_arrays_numpy` below (its docstring has the layout), ~20 us instead of ~0.4 ms of numpy
    calls for a ~1k-node subgraph.  (No "pos" maps: every frontier is a prefix of F_0.)"""
    q = np.ascontiguousarray(queries, dtype=np.int64).reshape(-1)
    if q.size == 0 or q.min() < 0 or q.max() >= S:
        raise ValueError("query positions out of range")
    if q.size > 1 and np.unique(q).size != q.size:
        raise ValueError("duplicate query positions")
    n_rel = len(rel_np)
    rel_ptr = np.zeros(n_rel + 1, dtype=np.int64)
    for r, e in enumerate(rel_np):
        rel_ptr[r + 1] = rel_ptr[r] + e.shape[1]

    def cat(xs):
        if len(xs) == 1:
            return np.ascontiguousarray(xs[0], dtype=np.int64)
        return np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0), dtype=np.int64)
    src, dst = cat([e[0] for e in rel_np]), cat([e[1] for e in rel_np])
    eid = cat(list(rel_eid)) if rel_eid is not None else None
    sizes = np.zeros((L + 1) * 7, dtype=np.int64)
    h = ctypes.c_void_p()

    def vp(a):
        return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)
    call("xpg_plan_arrays_build", int(S), n_rel, vp(rel_ptr), vp(src), vp(dst), vp(eid), vp(q),
         int(q.size), int(L), ctypes.byref(h), vp(sizes))
    out = np.empty(max(int(sizes.sum()), 1), dtype=np.int64)
    call("xpg_plan_arrays_take", h, vp(out))
    parts, o = [], 0
    for n in sizes.tolist():
        parts.append(out[o:o + n])
        o += n
    fr = parts[:L + 1]
    names = ("ptr", "src", "eid", "smul", "sptr", "seid")
    csrs = [dict(zip(names, parts[L + 1 + 6 * i:L + 7 + 6 * i])) for i in range(L + 1)]
    deg = csrs[0]
    layers = [{"agg_ptr": c["ptr"], "agg_src": c["src"], "agg_f0": c["src"], "self_mult": c["smul"],
               "agg_eid": c["eid"], "self_ptr": c["sptr"], "self_eid": c["seid"]} for c in csrs[1:]]
    return {"frontiers": fr, "deg_ptr": deg["ptr"], "deg_src": deg["src"], "deg_eid": deg["eid"],
            "layers": layers}


def plan_arrays_numpy(S, rel_np, queries, L, rel_eid=None):
    """numpy restatement of `plan_arrays` (the arrays the native builder is tested against).

    frontiers[L] = queries; frontiers[l-1] = frontiers[l] + sorted new in-neighbours (all
    relations), so frontiers[l] is a prefix of frontiers[l-1].  deg_*: in-edges (self-loops
    excluded) of every F_0 node per relation, relation-major with absolute offsets.  layers[l-1]:
    in-edges of F_l targets (self-loops excluded) with source positions in F_{l-1} and F_0, plus
    the multiplicity of (t, t) edges per relation.

    rel_eid (edge-mask plans, Data.perturb_edge): per relation the mask column of every edge;
    the CSRs then also carry each entry's column (deg_eid, agg_eid) and every target's
    self-loop columns (self_ptr / self_eid)."""
    all_src = np.concatenate([e[0] for e in rel_np]) if rel_np else np.zeros(0, np.int64)
    all_dst = np.concatenate([e[1] for e in rel_np]) if rel_np else np.zeros(0, np.int64)
    fr = [None] * (L + 1)
    fr[L] = np.asarray(queries, dtype=np.int64).reshape(-1)
    if fr[L].size == 0 or fr[L].min() < 0 or fr[L].max() >= S:
        raise ValueError("query positions out of range")
    if np.unique(fr[L]).size != fr[L].size:
        raise ValueError("duplicate query positions")
    for lvl in range(L, 0, -1):
        cur = fr[lvl]
        mark = np.zeros(S, dtype=bool)
        mark[cur] = True
        nb = np.unique(all_src[mark[all_dst]])
        fr[lvl - 1] = np.concatenate([cur, nb[~mark[nb]]])
    pos = []
    for lvl in range(L + 1):
        p = np.full(S, -1, dtype=np.int64)
        p[fr[lvl]] = np.arange(fr[lvl].size)
        pos.append(p)
    n0 = fr[0].size

    eids = rel_eid if rel_eid is not None else [np.zeros(e.shape[1], np.int64) for e in rel_np]

    def csr(targets_pos, n_t, src_pos_maps):
        ptrs, cols, off = [], [[] for _ in src_pos_maps], 0
        smul, eid, sptr, seid, soff = [], [], [], [], 0
        for (s, d), ecol in zip(rel_np, eids):
            k = s != d
            s2, d2, e2 = s[k], d[k], ecol[k]
            sel = targets_pos[d2] >= 0
            key = targets_pos[d2[sel]]
            order = np.argsort(key, kind="stable")
            src_nodes = s2[sel][order]
            eid.append(e2[sel][order])
            for j, m in enumerate(src_pos_maps):
                cols[j].append(m(src_nodes))
            cnt = np.bincount(key, minlength=n_t)
            ptrs.append(np.concatenate([[0], np.cumsum(cnt)]) + off)
            off += int(cnt.sum())
            loops, lcol = s[~k], ecol[~k]
            ls = targets_pos[loops] >= 0
            lkey = targets_pos[loops[ls]]
            smul.append(np.bincount(lkey, minlength=n_t))
            lorder = np.argsort(lkey, kind="stable")
            seid.append(lcol[ls][lorder])
            sptr.append(np.concatenate([[0], np.cumsum(smul[-1])]) + soff)
            soff += int(smul[-1].sum())
        cat = [np.concatenate(c) if c else np.zeros(0, np.int64) for c in cols]
        return (np.concatenate(ptrs), cat, np.concatenate(smul), np.concatenate(eid),
                np.concatenate(sptr), np.concatenate(seid))

    deg_ptr, (deg_src,), _, deg_eid, _, _ = csr(pos[0], n0, [lambda v: v])
    layers = []
    for lvl in range(1, L + 1):
        ptr_, (a_src, a_f0), smul, a_eid, s_ptr, s_eid = csr(
            pos[lvl], fr[lvl].size, [lambda v, l=lvl: pos[l - 1][v], lambda v: pos[0][v]])
        layers.append({"agg_ptr": ptr_, "agg_src": a_src, "agg_f0": a_f0, "self_mult": smul,
                       "agg_eid": a_eid, "self_ptr": s_ptr, "self_eid": s_eid})
    return {"frontiers": fr, "pos": pos, "deg_ptr": deg_ptr, "deg_src": deg_src,
            "deg_eid": deg_eid, "layers": layers}


WEIGHT_KINDS = ("gcn", "mean", "sum", "max", "root")  # term kinds a weighted plan takes


def check_edge_weight(edge_weight, n_edges, gcn):
    """float32 numpy [n_edges] copy of `edge_weight`: one finite weight per edge, none negative
    when the program holds a GCN term (gcn_norm's deg^-1/2); ValueError otherwise."""
    w = np.asarray(torch.as_tensor(edge_weight).detach().cpu().numpy())
    if w.ndim == 2 and w.shape[1] == 1:
        w = w[:, 0]
    if w.ndim != 1 or w.shape[0] != int(n_edges):
        raise ValueError(f"edge_weight must give one weight per edge ({int(n_edges)}), got shape "
                         f"{tuple(w.shape)}")
    if not np.issubdtype(w.dtype, np.floating):
        raise ValueError("edge_weight must be a floating-point tensor")
    if not np.isfinite(w).all():
        raise ValueError("edge_weight must be finite (NaN or inf found)")
    if gcn and w.size and float(w.min()) < 0:
        raise ValueError("edge_weight must be >= 0 for GCNConv (gcn_norm takes deg^-1/2)")
    return np.ascontiguousarray(w, dtype=np.float32)


def weight_arrays(arr, src, dst, w):
    """The edge weights of a plan in its CSR orders (xpgnn.h, xpg_edge_weights), on the host.
    `arr`: plan_arrays(..., rel_eid=[arange(E)]) of a one-relation graph, so that deg_eid / agg_eid
    / self_eid are edge ids; src / dst [E] the subgraph's edges, w [E] their weights.  Returns
    {"deg_w" [n_deg_edges], "loop_w" [n0], "layers": [{"agg_w" [n_edges], "self_sum", "self_wmax",
    "self_wmin" [n_tgt]}]}, float32: loop_w = the weight of a node's LAST self-loop in edge order (1
    without one), self_* = sum / max / min over the target's self-loops (sum 0, max / min 1 without
    one; the sum is taken in fp64 and rounded once)."""
    w = np.asarray(w, dtype=np.float32)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    fr0 = np.asarray(arr["frontiers"][0], dtype=np.int64)
    S = int(max(src.max(initial=-1), dst.max(initial=-1), fr0.max(initial=-1))) + 1
    lw = np.ones(S, dtype=np.float32)
    loops = np.nonzero(src == dst)[0]
    if loops.size:
        # the last loop of each node by edge position: the first occurrence in reversed order
        rev = loops[::-1]
        nodes, first = np.unique(src[rev], return_index=True)
        lw[nodes] = w[rev[first]]
    out = {"deg_w": w[np.asarray(arr["deg_eid"], dtype=np.int64)], "loop_w": lw[fr0], "layers": []}
    for lay in arr["layers"]:
        sptr = np.asarray(lay["self_ptr"], dtype=np.int64)
        ws = w[np.asarray(lay["self_eid"], dtype=np.int64)]
        n_t = sptr.size - 1
        cnt = np.diff(sptr)
        seg = np.repeat(np.arange(n_t), cnt)
        ssum = np.zeros(n_t, dtype=np.float64)
        np.add.at(ssum, seg, ws.astype(np.float64))
        smax = np.full(n_t, -np.inf, dtype=np.float32)
        smin = np.full(n_t, np.inf, dtype=np.float32)
        np.maximum.at(smax, seg, ws)
        np.minimum.at(smin, seg, ws)
        smax[cnt == 0] = 1.0
        smin[cnt == 0] = 1.0
        out["layers"].append({"agg_w": w[np.asarray(lay["agg_eid"], dtype=np.int64)],
                              "self_sum": ssum.astype(np.float32), "self_wmax": smax, "self_wmin": smin})
    return out


_EDGE_TABLE_MAX_BYTES = 1 << 30  # the edge tables of an edge-featured plan (a resource guard)


def check_edge_attr(edge_attr, n_edges):
    """float32 numpy [n_edges, D] copy of `edge_attr`: one finite float row per edge (a 1-D tensor
    of length n_edges is D = 1); ValueError otherwise."""
    a = np.asarray(torch.as_tensor(edge_attr).detach().cpu().numpy())
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[0] != int(n_edges) or a.shape[1] < 1:
        raise ValueError(f"edge_attr must give one row per edge ({int(n_edges)}), got shape "
                         f"{tuple(a.shape)}")
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError("edge_attr must be a floating-point tensor")
    if not np.isfinite(a).all():
        raise ValueError("edge_attr must be finite (NaN or inf found)")
    return np.ascontiguousarray(a, dtype=np.float32)


def edge_feature_arrays(arr, convs, ea, x0):
    """The edge features of a plan in its CSR orders (xpgnn.h, xpg_edge_feats), on the host.
    `arr`: plan_arrays(..., rel_eid=[arange(E)]) of a one-relation graph, so that agg_eid / self_eid
    are edge ids; `convs`: the program's conv layers; ea [E, D] float32 the attribute rows; x0
    [n0, f_in] float32 the feature rows of the F_0 nodes.  Per conv layer with a "sum" term (None
    for a ROOT-only layer) {"agg_e" [n_edges, f_in_pad], "self_e" [n_self, f_in_pad]}, float32 with
    zero padded columns: the rows of E_l = ea edge_lin_w^T + edge_lin_b (fp64, rounded once; ea
    itself without an edge map) gathered by the CSRs' edge ids.  Layer 1 also holds "msg_rows"
    [n_edges + n_self, f_in_pad]: relu(x_j + agg_e[e]) per in-edge, then relu(x_t + self_e[k]) per
    self-loop, in fp32 (the sources of layer 1 are the feature rows, the same for every mask row).
    ValueError for attribute rows whose width fits neither the edge map nor the layer input."""
    ea = np.asarray(ea, dtype=np.float32)
    out = []
    for li, (conv, lay) in enumerate(zip(convs, arr["layers"])):
        sums = [t for t in conv.terms if t.kind == "sum"]
        if not sums:
            out.append(None)
            continue
        term = sums[0]
        if term.edge_lin_w is not None:
            w = term.edge_lin_w.detach().cpu().numpy().astype(np.float64)
            if w.shape[1] != ea.shape[1]:
                raise ValueError(f"edge_attr of width {ea.shape[1]} on a GINEConv with edge_dim {w.shape[1]}")
            ee = ea.astype(np.float64) @ w.T
            if term.edge_lin_b is not None:
                ee = ee + term.edge_lin_b.detach().cpu().numpy().astype(np.float64)
            ee = ee.astype(np.float32)
        else:
            if ea.shape[1] != conv.f_in:
                raise ValueError(f"edge_attr of width {ea.shape[1]} on a GINEConv(edge_dim=None) whose "
                                 f"input has width {conv.f_in}")
            ee = ea
        pad = _rup(conv.f_in, 32)
        agg_eid = np.asarray(lay["agg_eid"], dtype=np.int64)
        self_eid = np.asarray(lay["self_eid"], dtype=np.int64)
        agg_e = np.zeros((agg_eid.size, pad), dtype=np.float32)
        agg_e[:, :conv.f_in] = ee[agg_eid]
        self_e = np.zeros((self_eid.size, pad), dtype=np.float32)
        self_e[:, :conv.f_in] = ee[self_eid]
        d = {"agg_e": agg_e, "self_e": self_e}
        if li == 0:
            xp = np.zeros((x0.shape[0], pad), dtype=np.float32)
            xp[:, :conv.f_in] = np.asarray(x0, dtype=np.float32)
            sptr = np.asarray(lay["self_ptr"], dtype=np.int64)
            tgt = np.repeat(np.arange(sptr.size - 1), np.diff(sptr))  # F_1 is a prefix of F_0
            msg = np.concatenate([xp[np.asarray(lay["agg_f0"], dtype=np.int64)] + agg_e,
                                  xp[tgt] + self_e])
            d["msg_rows"] = np.maximum(msg, np.float32(0))
        out.append(d)
    return out


_STAGING = {}  # device index -> [next slot, [(pinned host tensor, event of its last copy)] * _STAGING_SLOTS]
_STAGING_MAX = 16 << 20  # bytes: larger arrays take the pageable copy
_STAGING_SLOTS = 4  # a call's uploads take consecutive slots: none waits for the previous copy


def h2d(a, device):
    """A host numpy array (int32 / int64 / float32) as a new device tensor, copied from a pinned
    staging buffer without a host wait: a pageable host -> device copy waits for everything queued
    on the stream first (~40 us of an Explainer.run first call per plan upload, the device idle
    meanwhile).  Uploads rotate over a few pinned buffers; a buffer is reused once its previous
    copy has completed (its event: with one buffer the second upload of a call waited for the
    first copy, i.e. for everything queued before it)."""
    a = np.ascontiguousarray(a)
    dev = torch.device(device)
    if a.nbytes > _STAGING_MAX or a.nbytes == 0:
        return torch.from_numpy(a).to(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ring = _STAGING.get(key)
    if ring is None:  # every slot pinned up front: a pinned allocation costs ~0.2 ms per call
        ring = _STAGING[key] = [0, [(torch.empty(1 << 20, dtype=torch.uint8, pin_memory=True), None)
                                    for _ in range(_STAGING_SLOTS)]]
    slot = ring[0]
    ring[0] = (slot + 1) % _STAGING_SLOTS
    buf, ev = ring[1][slot]
    if ev is not None:
        ev.synchronize()
    if buf is None or buf.numel() < a.nbytes:
        buf = torch.empty(max(a.nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    buf[:a.nbytes].numpy()[:] = a.view(np.uint8).reshape(-1)
    out = torch.empty(a.shape, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    out.view(-1).view(torch.uint8).copy_(buf[:a.nbytes], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ring[1][slot] = (buf, ev)
    return out


_ATT_MAX_SLICES = 32  # (relation, head) slices of one attention layer's dense input; also the
                      # relation / basis slices of a typed-relation ("rel") layer past the first
_REL_TABLE_MAX_BYTES = 1 << 30  # per-relation layer-1 tables of a "rel" plan (a resource guard)


def relation_segments(agg_ptr, self_mult, n_rel, n_tgt):
    """Per-target relation lists of a "rel" layer from its CSR: (seg_ptr int64 [n_tgt + 1], seg_rel
    int64 [n_seg]), target t's relations seg_rel[seg_ptr[t]:seg_ptr[t + 1]] = those with an in-edge
    (agg_ptr [n_rel * (n_tgt + 1)], absolute offsets) or a self-loop (self_mult [n_rel * n_tgt]) at
    t, ascending.  The kernel visits only these instead of n_rel pointer pairs per item."""
    ptr_ = np.asarray(agg_ptr, dtype=np.int64).reshape(n_rel, n_tgt + 1)
    has = (np.diff(ptr_, axis=1) > 0) | (np.asarray(self_mult).reshape(n_rel, n_tgt) > 0)
    t_idx, r_idx = np.nonzero(has.T)  # row-major: by target, then relation ascending
    seg_ptr = np.zeros(n_tgt + 1, dtype=np.int64)
    np.cumsum(np.bincount(t_idx, minlength=n_tgt), out=seg_ptr[1:])
    return seg_ptr, r_idx.astype(np.int64)


def _rel_tables(X0, W, f_out_pad, device):
    """Layer-1 tables [R][n0][f_out_pad] of a "rel" term: X0 times the stacked relation weights
    W [R, f_out, f_in], on the dense kernel in column groups of at most 256."""
    R, f_out, _ = W.shape
    n0 = X0.shape[0]
    T = torch.zeros((R, n0, f_out_pad), dtype=torch.float32, device=device)
    per = max(1, 256 // f_out_pad)
    for r0 in range(0, R, per):
        n = min(per, R - r0)
        Wg = torch.zeros((n, f_out_pad, W.shape[2]), dtype=torch.float32, device=device)
        Wg[:, :f_out] = W[r0:r0 + n]
        C = dense(X0, Wg.reshape(n * f_out_pad, -1), None, None)  # [n0, n * f_out_pad]
        T[r0:r0 + n] = C.reshape(n0, n, f_out_pad).permute(1, 0, 2)
    return T


def _dev(t, device):
    return None if t is None else t.to(device)


def _pad_vec(v, n, device):
    out = torch.zeros(n, dtype=torch.float32, device=device)
    out[:v.numel()] = v.to(device=device, dtype=torch.float32)
    return out


def _pad_table(T, n):
    """[rows, n] fp32 copy of T with zero columns past its own."""
    out = torch.zeros((T.shape[0], n), dtype=torch.float32, device=T.device)
    out[:, :T.shape[1]] = T
    return out


def _qkv_blocks(term):
    """The (weight, bias) blocks of a "qkv" term in the order the engine stores them: K, V, Q and,
    with root_weight, S."""
    blocks = [(term.weight, term.bias_l), (term.weight_v, term.bias_v), (term.weight_q, term.bias_q)]
    if term.weight_s is not None:
        blocks.append((term.weight_s, term.bias_s))
    return blocks


# ForwardPlan drops the relation terms of other destination types from a layer whose targets
# share one node type (they add exactly 0); False keeps every term (the parity suite's reference)
PLAN_DROP_OTHER_TYPES = True


class ForwardPlan:
    """Receptive-field plan of one (subgraph, model program, query set)."""

    def __init__(self, program, sub_feat, rel_edges, queries, device=None, node_type=None,
                 edge_cols=None, link=None, edge_weight=None, edge_attr=None, out_col=None, classes=None):
        """`node_type` ([S] node type of every subgraph node) is required by multi-node-type
        programs: per layer, every target's type gates the relation terms (xpgnn.h).

        Edge problems (Data.perturb_edge, data.py:500-554): `edge_cols` = per relation the mask
        column of every edge (mask columns are the subgraph's edges; `cols` becomes their
        count) and `link` = (a, b, act): the output is the link decoder act(<h_a, h_b>) of
        queries a and b instead of one column per query; `link` = (a, b, act, d) with a vector d
        of the output width scales the columns, act(sum_f h_a[f] d[f] h_b[f]) (DistMult, d = the
        query relation's embedding).  A typed-relation ("rel") program takes one entry of
        `rel_edges` / `edge_cols` per edge type.

        A pooled program (`program.pool`, nn.PooledModel): after the last conv layer the rows of
        the `queries` (pipeline.build_plan passes every node) reduce to one row per mask row
        (xpg_layer_desc.pool), the head runs on it and forward returns [rows, 1]; node masks,
        single-node-type programs only.

        `edge_weight` ([E], one finite float per edge of the one relation; PyG 2.0.4's edge_weight
        of GCNConv / GraphConv): the plan carries the weights gathered into its CSR orders
        (weight_arrays; xpgnn.h, xpg_edge_weights) and runs on k_degree_w / k_agg_w.  Node masks,
        one relation, one node type, gcn / mean / sum / max / root terms only; weights >= 0 with a
        gcn term.  None: the plan is exactly the unweighted one.

        `edge_attr` ([E, D] or [E], one finite float row per edge of the one relation; PyG 2.0.4's
        edge_attr of GINEConv): needed by, and only taken by, a program compiled with
        edge_attr=True.  The plan carries each layer's mapped edge rows gathered into its CSR
        orders (edge_feature_arrays; xpgnn.h, xpg_edge_feats) and runs on k_agg_e; every layer takes
        the aggregate-then-transform form, so the input may be at most 256 columns wide after
        padding to 32.  Node masks, one relation, one node type; not together with edge_weight.

        `out_col` (class c of a model with C output columns; None: the program's own out_col, 0)
        and `classes` (None, or "all"): which output columns forward returns.  On a program without `out_norm`, `out_col`
        alone fills the descriptor's out_col and the plan keeps every path.  A program that ends in
        softmax / log_softmax (`program.out_norm`), or classes="all", carries a class readout
        (xpgnn.h, xpg_class_out; k_class_out on the multi-kernel path): forward returns
        [rows, n_targets] for one class, [rows, n_targets * C] in (target, class) order for all.
        Node masks, single-node-type programs, no link decoder."""
        device = torch.device(device) if device is not None else sub_feat.device
        _lib.require_device(torch.empty(0, device=device), "plan device")
        if len(program.convs) == 0:
            raise ValueError("program has no conv layer")
        self.device = device
        self.program = program
        S = int(sub_feat.shape[0])  # subgraph nodes
        self.n_rel = len(rel_edges)
        self._keep = []  # device tensors referenced by descriptors
        self._staged = []  # (descriptor, field, int32 array) awaiting the one upload

        rel_np = [np.asarray(e.detach().cpu().numpy(), dtype=np.int64).reshape(2, -1)
                  for e in rel_edges]
        rel_eid = None
        if edge_cols is not None:
            rel_eid = [np.asarray(torch.as_tensor(c).detach().cpu().numpy(), dtype=np.int64).reshape(-1)
                       for c in edge_cols]
            if len(rel_eid) != len(rel_np) or any(c.size != e.shape[1] for c, e in zip(rel_eid, rel_np)):
                raise ValueError("edge_cols must give one mask column per edge of every relation")
            if program.n_types > 1:
                raise ValueError("edge masks on multi-node-type programs are not supported")
        self.pool = getattr(program, "pool", None)
        if self.pool is not None:
            # graph-level readout after the last conv layer (xpgnn.h, enum xpg_pool): one output
            # per mask row over the plan's last frontier (pipeline.build_plan: every node)
            if self.pool not in _lib.POOL:
                raise ValueError(f"unknown pool {self.pool!r}")
            if rel_eid is not None or link is not None:
                raise ValueError("pooled (graph-level) programs on edge-mask plans are not supported")
            if program.n_types > 1:
                raise ValueError("pooled (graph-level) multi-node-type programs are not supported")
        self.edge_masks = rel_eid is not None
        self.cols = (int(max((int(c.max()) for c in rel_eid if c.size), default=-1)) + 1
                     if self.edge_masks else S)
        if self.edge_masks:
            ncol = sum(c.size for c in rel_eid)
            allc = np.concatenate(rel_eid) if ncol else np.zeros(0, np.int64)
            if ncol and (allc.min() < 0 or np.unique(allc).size != ncol or self.cols != ncol):
                raise ValueError("edge mask columns must be 0..E-1, one per edge")
            if ncol == 0:
                raise ValueError("edge masks need at least one edge")
        L = len(program.convs)
        w_np = None
        if edge_weight is not None:
            kinds = {t.kind for c in program.convs for t in c.terms}
            if not kinds <= set(WEIGHT_KINDS):
                raise ValueError(f"edge_weight on a program with {sorted(kinds - set(WEIGHT_KINDS))} "
                                 "terms is not supported (GCNConv / GraphConv only)")
            if self.edge_masks or link is not None:
                raise ValueError("edge_weight on edge-mask plans is not supported")
            if self.n_rel != 1 or program.n_types > 1:
                raise ValueError("edge_weight on multi-relation or multi-node-type graphs is not supported")
            w_np = check_edge_weight(edge_weight, rel_np[0].shape[1], "gcn" in kinds)
            # the CSRs carry each entry's edge id, which gathers the weights below
            rel_eid = [np.arange(rel_np[0].shape[1], dtype=np.int64)]
        ea_np = None
        if edge_attr is not None or getattr(program, "edge_featured", False):
            if edge_attr is not None and edge_weight is not None:
                raise ValueError("edge_attr and edge_weight together are not supported")
            if edge_attr is None:
                raise ValueError("a program compiled for edge features needs the plan's edge_attr")
            kinds = {t.kind for c in program.convs for t in c.terms}
            if not getattr(program, "edge_featured", False) or not kinds <= {"sum", "root"}:
                raise ValueError("edge_attr on a program that was not compiled for edge features "
                                 "(GINEConv only) is not supported")
            if self.edge_masks or link is not None:
                raise ValueError("edge_attr on edge-mask plans is not supported")
            if self.n_rel != 1 or program.n_types > 1:
                raise ValueError("edge_attr on multi-relation or multi-node-type graphs is not supported")
            ea_np = check_edge_attr(edge_attr, rel_np[0].shape[1])
            # the CSRs carry each entry's edge id, which gathers the edge rows below
            rel_eid = [np.arange(rel_np[0].shape[1], dtype=np.int64)]
        arr = plan_arrays(S, rel_np, queries, L, rel_eid)
        self.arrays = arr
        fr = arr["frontiers"]
        n0 = fr[0].size
        self.n0 = n0
        self.frontiers = fr

        X0 = sub_feat.to(device=device, dtype=torch.float32)[h2d(fr[0], device)]
        f_in0 = program.convs[0].f_in
        nt_np = None
        if program.n_types > 1:
            if node_type is None:
                raise ValueError("multi-node-type program needs the subgraph node types")
            nt_np = np.asarray(torch.as_tensor(node_type).detach().cpu().numpy()).astype(np.int64)
            if nt_np.shape != (S,) or nt_np.min() < 0 or nt_np.max() >= program.n_types:
                raise ValueError("node types out of range")
            if X0.shape[1] > f_in0:  # widest types are zero-padded beyond every relation's input
                X0 = X0[:, :f_in0]
        if X0.shape[1] != f_in0:
            raise ValueError(f"feature width {X0.shape[1]} != first conv input {f_in0}")

        self._layers = (LayerDesc * L)()
        prev_pad = None
        self.terms_kept = []  # per layer: terms after dropping other node types' relations
        self.lowering = []  # per layer: (kind, relation, destination type) of every kept term
        for li, conv in enumerate(program.convs):
            lvl = li + 1
            n_t = fr[lvl].size
            f_out_pad = _rup(conv.f_out, 32)
            if f_out_pad > 256 or len(conv.terms) > _lib.MAX_TERMS:
                raise ValueError("conv wider than 256 or more than 8 terms is not supported")
            terms = list(conv.terms)
            att = any(t.kind == "att" for t in terms)
            if att and not all(t.kind == "att" for t in terms):
                raise ValueError("a conv layer mixing attention with other terms is not supported")
            if att and self.edge_masks:
                raise ValueError("attention terms on edge-mask plans are not supported")
            att2 = any(t.kind == "att2" for t in terms)
            if att2 and not all(t.kind == "att2" for t in terms):
                raise ValueError("a conv layer mixing dynamic attention with other terms is not supported")
            if att2 and (self.edge_masks or program.n_types > 1):
                raise ValueError("dynamic-attention terms on edge-mask or multi-node-type plans "
                                 "are not supported")
            qkv = any(t.kind == "qkv" for t in terms)
            if qkv and not all(t.kind == "qkv" for t in terms):
                raise ValueError("a conv layer mixing dot-product attention with other terms is not supported")
            if qkv and (self.edge_masks or program.n_types > 1):
                raise ValueError("dot-product-attention terms on edge-mask or multi-node-type plans "
                                 "are not supported")
            if self.edge_masks and any(t.kind in ("sum", "max") for t in terms):
                raise ValueError("sum / max terms on edge-mask plans are not supported")
            rel = [t for t in terms if t.kind == "rel"]
            if rel:
                if len(rel) != 1 or terms[0] is not rel[0] or len(terms) > 2 or \
                        any(t.kind != "root" for t in terms[1:]):
                    raise ValueError("a typed-relation layer holds one rel term and at most one root term")
                if program.n_types > 1:
                    raise ValueError("rel terms on multi-node-type programs are not supported")
                if rel[0].num_relations != self.n_rel:
                    raise ValueError(f"conv with {rel[0].num_relations} relations on a plan of "
                                     f"{self.n_rel} edge types")
                if li > 0 and rel[0].slices > _ATT_MAX_SLICES:
                    raise ValueError(f"typed-relation layer past the first with more than "
                                     f"{_ATT_MAX_SLICES} relation / basis slices is not supported")
                if li == 0 and self.n_rel * n0 * f_out_pad * 4 > _REL_TABLE_MAX_BYTES:
                    raise ValueError("typed-relation layer-1 tables exceed "
                                     f"{_REL_TABLE_MAX_BYTES >> 20} MiB")
            elif any(any(t.kind == "rel" for t in c.terms) for c in program.convs):
                raise ValueError("a program mixing typed-relation layers with other layers is not supported")
            if nt_np is not None:
                # every target of this layer has one node type: a relation term of another
                # destination type adds exactly 0 to every target (HeteroConv sums per
                # destination), so it is dropped — fewer aggregate columns and a shorter K of
                # the layer's dense product (the query layer of a multi-type plan)
                tt = np.unique(nt_np[fr[lvl]])
                if tt.size == 1 and PLAN_DROP_OTHER_TYPES:
                    kept = [t for t in terms if t.dst_type < 0 or t.dst_type == int(tt[0])]
                    terms = kept or terms
            self.terms_kept.append(len(terms))
            if att and li > 0 and sum(t.heads for t in terms) > _ATT_MAX_SLICES:
                raise ValueError(f"attention layer with more than {_ATT_MAX_SLICES} head slices "
                                 "is not supported")
            self.lowering.append(tuple((t.kind, t.rel, t.dst_type) for t in terms))
            ld = self._layers[li]
            ld.n_terms = len(terms)
            ld.act = ACT[conv.act]
            ld.f_out = conv.f_out
            ld.f_out_pad = f_out_pad
            ld.n_tgt = n_t
            ld.n_edges = int(arr["layers"][li]["agg_src"].size)
            # max is not linear: a first conv with a "max" term takes the raw form (aggregate the
            # raw feature rows, then the dense product), like every deeper layer
            raw = li == 0 and (any(t.kind == "max" for t in terms) or ea_np is not None)
            if raw:
                prev_pad = _rup(f_in0, 32)
                if prev_pad > 256:
                    raise ValueError("a first conv with a max term and an input wider than 256 "
                                     "is not supported" if ea_np is None else
                                     "edge features with an input wider than 256 are not supported")
            ld.f_in_pad = prev_pad if (li > 0 or raw) else 0
            nz = lambda a: a if a.size else np.zeros(1)
            self._i32(ld, "tgt_prev", np.arange(n_t))  # F_l is a prefix of F_{l-1}
            self._i32(ld, "tgt_f0", np.arange(n_t))  # F_l is a prefix of F_0 too
            lay = arr["layers"][li]
            self._i32(ld, "agg_ptr", lay["agg_ptr"])
            self._i32(ld, "agg_src", nz(lay["agg_src"]))
            self._i32(ld, "agg_f0", nz(lay["agg_f0"]))
            self._i32(ld, "self_mult", lay["self_mult"])
            if rel:
                seg_ptr, seg_rel = relation_segments(lay["agg_ptr"], lay["self_mult"], self.n_rel, n_t)
                self._i32(ld, "seg_ptr", seg_ptr)
                self._i32(ld, "seg_rel", nz(seg_rel))
            if self.edge_masks:
                self._i32(ld, "agg_eid", nz(lay["agg_eid"]))
                self._i32(ld, "self_ptr", lay["self_ptr"])
                self._i32(ld, "self_eid", nz(lay["self_eid"]))
            if ea_np is not None:  # k_agg_e walks the self-loops; their rows are in self_eid's order
                self._i32(ld, "self_ptr", lay["self_ptr"])
            n_types = program.n_types

            def make_bias(conv=conv, f_out_pad=f_out_pad):
                b = torch.zeros((n_types, f_out_pad), dtype=torch.float32, device=device)
                b[:, :conv.f_out] = conv.bias.to(device).reshape(-1, conv.f_out)
                return b
            bias = self._program_tensor(program, ("bias", li), make_bias)
            self._keep.append(bias)
            ld.bias = bias.data_ptr()
            ld.n_types = n_types
            if nt_np is not None:
                self._i32(ld, "tgt_type", nt_np[fr[lvl]])
            else:
                ld.tgt_type = None
            for k, term in enumerate(terms):
                ld.terms[k].kind = _lib.TERM_QKV if term.kind == "qkv" else TERM[term.kind]
                ld.terms[k].rel = term.rel
                ld.terms[k].dst_type = term.dst_type
                if term.kind == "att":
                    ld.terms[k].heads, ld.terms[k].head_ch = term.heads, term.head_ch
                    ld.terms[k].neg_slope = term.neg_slope
                    ld.terms[k].self_loops = int(term.self_loops)
                if term.kind == "att2":
                    ld.terms[k].heads, ld.terms[k].head_ch = term.heads, term.head_ch
                    ld.terms[k].neg_slope = term.neg_slope
                    ld.terms[k].self_loops = int(term.self_loops)
                    ld.terms[k].dst_type = -1
                    att_p = self._program_tensor(
                        program, ("att2_att", li, id(term)),
                        lambda term=term, f_out_pad=f_out_pad: _pad_vec(term.att.reshape(-1), f_out_pad, device))
                    self._keep.append(att_p)
                    ld.terms[k].att_src = att_p.data_ptr()
                if term.kind == "qkv":
                    ld.terms[k].heads, ld.terms[k].head_ch = term.heads, term.head_ch
                    # the logit scale 1 / sqrt(head_ch), rounded once from fp64, travels in neg_slope
                    ld.terms[k].neg_slope = float(np.float32(1.0 / np.sqrt(np.float64(term.head_ch))))
                    ld.terms[k].self_loops = 0
                    ld.terms[k].dst_type = -1
                    ld.terms[k].n_slices = len(_qkv_blocks(term))
                    ld.terms[k].att_dst = None
                    if term.gate_out is not None:
                        gate = self._program_tensor(
                            program, ("qkv_gate", li, id(term)),
                            lambda term=term, f_out_pad=f_out_pad: torch.stack(
                                [_pad_vec(term.gate_out, f_out_pad, device),
                                 _pad_vec(term.gate_r, f_out_pad, device)]).contiguous())
                        self._keep.append(gate)
                        ld.terms[k].att_src = gate.data_ptr()
                    else:
                        ld.terms[k].att_src = None
                if term.kind == "rel":
                    ld.terms[k].n_slices = self.n_rel if li == 0 else term.slices
                    ld.terms[k].norm = REL_NORM[term.norm]
            if raw:
                # one zero-padded X[F_0] table shared by the terms (and by every mask row)
                X0p = torch.zeros((n0, prev_pad), dtype=torch.float32, device=device)
                X0p[:, :f_in0] = X0
                self._keep.append(X0p)
                for k in range(len(terms)):
                    ld.terms[k].table = X0p.data_ptr()
            if li == 0 and not raw:
                for k, term in enumerate(terms):
                    if term.kind == "rel":
                        # one table per relation (bases folded into W_r): an edge reads one row
                        Wr = self._program_tensor(program, ("rel_l1", li, id(term)),
                                                  lambda term=term: relation_weights(term).to(device))
                        Tp = _rel_tables(X0, Wr, f_out_pad, device)
                        self._keep.append(Tp)
                        ld.terms[k].table = Tp.data_ptr()
                        continue
                    if term.kind == "att2":
                        # XL / XR of the F_0 nodes, shared by every mask row (features are never
                        # masked): X0 W_l^T + b_l and X0 W_r^T + b_r, padded columns 0
                        XL = _pad_table(dense(X0, term.weight.to(device), _dev(term.bias_l, device)),
                                        f_out_pad)
                        XR = XL if term.weight_r is None else \
                            _pad_table(dense(X0, term.weight_r.to(device), _dev(term.bias_r, device)),
                                       f_out_pad)
                        self._keep += [XL, XR]
                        ld.terms[k].table, ld.terms[k].att_dst = XL.data_ptr(), XR.data_ptr()
                        continue
                    if term.kind == "qkv":
                        # K | V | Q (| S) of the F_0 nodes with their biases, one f_out_pad-wide
                        # block each, shared by every mask row; padded columns 0
                        T = torch.cat([_pad_table(dense(X0, w.to(device), _dev(b, device)), f_out_pad)
                                       for w, b in _qkv_blocks(term)], dim=1).contiguous()
                        self._keep.append(T)
                        ld.terms[k].table = T.data_ptr()
                        continue
                    T = dense(X0, term.weight.to(device), None, None)
                    Tp = torch.zeros((n0, f_out_pad), dtype=torch.float32, device=device)
                    Tp[:, :conv.f_out] = T
                    self._keep.append(Tp)
                    ld.terms[k].table = Tp.data_ptr()
                    if term.kind == "att":
                        # per-plan score tables a_s / a_d [n0][heads], shared by every mask row:
                        # X0 times the attention vectors folded through W_src / W_dst
                        v_s, v_d = self._program_tensor(
                            program, ("att_l1", li, id(term)),
                            lambda term=term: tuple(v.to(device).contiguous()
                                                    for v in fold_attention(term)))
                        a_s = dense(X0, v_s, None, None).contiguous()
                        a_d = dense(X0, v_d, None, None).contiguous()
                        self._keep += [a_s, a_d]
                        ld.terms[k].att_src, ld.terms[k].att_dst = a_s.data_ptr(), a_d.data_ptr()
                ld.weight = None
            elif att2:
                # transform-then-aggregate: per term the stacked [W_l; W_r] (one block when
                # shared) and [b_l; b_r], zero-padded; the layer itself has no weight
                ld.weight = None
                for k, term in enumerate(terms):
                    def make_att2(term=term, prev_pad=prev_pad, f_out_pad=f_out_pad):
                        ws = [term.weight] + ([] if term.weight_r is None else [term.weight_r])
                        bs = [term.bias_l] + ([] if term.weight_r is None else [term.bias_r])
                        w = torch.zeros((len(ws), f_out_pad, prev_pad), dtype=torch.float32, device=device)
                        b = torch.zeros((len(ws), f_out_pad), dtype=torch.float32, device=device)
                        for i, (wi, bi) in enumerate(zip(ws, bs)):
                            w[i, :wi.shape[0], :wi.shape[1]] = wi.to(device)
                            if bi is not None:
                                b[i, :bi.shape[0]] = bi.to(device)
                        return w, b
                    w2, b2 = self._program_tensor(program, ("att2_w", li, id(term)), make_att2)
                    self._keep += [w2, b2]
                    ld.terms[k].table, ld.terms[k].coef = w2.data_ptr(), b2.data_ptr()
                    ld.terms[k].n_slices = w2.shape[0]  # 1: shared weights
            elif qkv:
                # transform-then-aggregate: per term the stacked [W_k; W_v; W_q (; W_s)] and their
                # biases, zero-padded; the layer itself has no weight
                ld.weight = None
                for k, term in enumerate(terms):
                    def make_qkv(term=term, prev_pad=prev_pad, f_out_pad=f_out_pad):
                        blocks = _qkv_blocks(term)
                        w = torch.zeros((len(blocks), f_out_pad, prev_pad), dtype=torch.float32, device=device)
                        b = torch.zeros((len(blocks), f_out_pad), dtype=torch.float32, device=device)
                        for i, (wi, bi) in enumerate(blocks):
                            w[i, :wi.shape[0], :wi.shape[1]] = wi.to(device)
                            if bi is not None:
                                b[i, :bi.shape[0]] = bi.to(device)
                        return w, b
                    w4, b4 = self._program_tensor(program, ("qkv_w", li, id(term)), make_qkv)
                    self._keep += [w4, b4]
                    ld.terms[k].table, ld.terms[k].coef = w4.data_ptr(), b4.data_ptr()
            elif att:
                # one f_in_pad-wide slice of the dense input per (term, head): head h's rows of
                # W_src in slice (k, h), zeros elsewhere, so the layer stays aggregate-then-transform
                def make_att(terms=terms, prev_pad=prev_pad, f_out_pad=f_out_pad):
                    w, vecs = stack_attention(terms, prev_pad, f_out_pad)
                    return (w.to(device=device, dtype=torch.float32).contiguous(),
                            [tuple(v.to(device=device, dtype=torch.float32).contiguous() for v in pr)
                             for pr in vecs])
                Wc, vecs = self._program_tensor(program, ("wc_att", li, tuple(id(t) for t in terms)),
                                                make_att)
                self._keep.append(Wc)
                ld.weight = Wc.data_ptr()
                for k, (v_s, v_d) in enumerate(vecs):
                    self._keep += [v_s, v_d]
                    ld.terms[k].att_src, ld.terms[k].att_dst = v_s.data_ptr(), v_d.data_ptr()
            elif rel:
                # slice s of the dense input meets V_s^T / W_r^T, the root slice the root weight
                def make_rel(conv=conv, terms=terms, prev_pad=prev_pad, f_out_pad=f_out_pad):
                    t0 = terms[0]
                    w = torch.zeros((f_out_pad, (t0.slices + len(terms) - 1) * prev_pad),
                                    dtype=torch.float32, device=device)
                    for s_ in range(t0.slices):
                        w[:conv.f_out, s_ * prev_pad:s_ * prev_pad + conv.f_in] = t0.weight[s_].to(device)
                    for k, term in enumerate(terms[1:]):
                        c0 = (t0.slices + k) * prev_pad
                        w[:conv.f_out, c0:c0 + conv.f_in] = term.weight.to(device)
                    coef = None if t0.coef is None else \
                        t0.coef.to(device=device, dtype=torch.float32).contiguous()
                    return w, coef
                Wc, coef = self._program_tensor(program, ("wc_rel", li, tuple(id(t) for t in terms)),
                                                make_rel)
                self._keep.append(Wc)
                ld.weight = Wc.data_ptr()
                if coef is not None:
                    self._keep.append(coef)
                    ld.terms[0].coef = coef.data_ptr()
            else:
                def make_wc(conv=conv, terms=terms, prev_pad=prev_pad, f_out_pad=f_out_pad):
                    w = torch.zeros((f_out_pad, len(terms) * prev_pad), dtype=torch.float32,
                                    device=device)
                    for k, term in enumerate(terms):
                        w[:conv.f_out, k * prev_pad:k * prev_pad + conv.f_in] = term.weight.to(device)
                    return w
                Wc = self._program_tensor(program, ("wc", li, tuple(id(t) for t in terms)), make_wc)
                self._keep.append(Wc)
                ld.weight = Wc.data_ptr()
            prev_pad = f_out_pad
        if self.pool is not None:
            self._layers[L - 1].pool = _lib.POOL[self.pool]
        # post-ops (xpgnn.h, xpg_post_desc): one host record per conv layer, all zero = none; their
        # vectors are the program's, zero-padded to the layer's width
        self._post = None
        if any(getattr(c, "post", None) is not None for c in program.convs):
            if self.edge_masks or link is not None:
                raise ValueError("post-ops (LayerNorm, residual, BatchNorm after attention) on "
                                 "edge-mask plans are not supported")
            if program.n_types > 1:
                raise ValueError("post-ops on multi-node-type programs are not supported")
            self._post = (_lib.PostDesc * L)()
            for li, conv in enumerate(program.convs):
                q = conv.post
                if q is None:
                    continue
                pd = self._post[li]
                pd.norm, pd.eps = _lib.NORM[q.norm], float(q.eps)
                pd.act, pd.residual = ACT[q.act], int(bool(q.residual))
                for name in ("scale", "shift", "gamma", "beta"):
                    v = getattr(q, name)
                    if v is None:
                        continue
                    vp = self._program_tensor(
                        program, ("post", li, name),
                        lambda v=v, n=self._layers[li].f_out_pad: _pad_vec(v.reshape(-1), n, device))
                    self._keep.append(vp)
                    setattr(pd, name, vp.data_ptr())

        self._head = (HeadDesc * max(1, len(program.head)))()
        for i, h in enumerate(program.head):
            n_real, k_real = h.weight.shape
            n_pad = _rup(n_real, 32)
            if n_pad > 256:
                raise ValueError("head layer wider than 256 is not supported")
            def make_head(h=h, n_real=n_real, k_real=k_real, n_pad=n_pad, prev_pad=prev_pad):
                w = torch.zeros((n_pad, prev_pad), dtype=torch.float32, device=device)
                w[:n_real, :k_real] = h.weight.to(device)
                b = torch.zeros(n_pad, dtype=torch.float32, device=device)
                if h.bias is not None:
                    b[:n_real] = h.bias.to(device)
                return w, b
            Wp, bp = self._program_tensor(program, ("head", i), make_head)
            self._keep += [Wp, bp]
            hd = self._head[i]
            hd.k_pad, hd.n_real, hd.n_pad, hd.act = prev_pad, n_real, n_pad, ACT[h.act]
            hd.weight, hd.bias = Wp.data_ptr(), bp.data_ptr()
            prev_pad = n_pad

        self.n_out = fr[L].size
        # the output column(s): descriptor out_col, or a class readout beside the plan
        self.n_classes = program.n_classes
        self.out_norm = getattr(program, "out_norm", None)
        if classes not in (None, "all"):
            raise ValueError(f"classes must be None or 'all', got {classes!r}")
        if out_col is None:
            out_col = program.out_col
        if isinstance(out_col, bool) or not isinstance(out_col, (int, np.integer)):
            raise TypeError("out_col must be an int")
        if not 0 <= int(out_col) < self.n_classes:
            raise ValueError(f"out_col {out_col} outside [0, {self.n_classes})")
        self.out_col, self.classes = int(out_col), classes
        self._cls = None
        if self.out_norm is not None or classes == "all":
            if self.out_norm not in _lib.CLASS_KIND:
                raise ValueError(f"unknown out_norm {self.out_norm!r}")
            if self.edge_masks or link is not None:
                raise ValueError("a class readout (softmax / all classes) on edge-mask plans is not supported")
            if program.n_types > 1:
                raise ValueError("a class readout (softmax / all classes) on multi-node-type programs "
                                 "is not supported")
            self._cls = _lib.ClassOut(kind=_lib.CLASS_KIND[self.out_norm],
                                      col=-1 if classes == "all" else self.out_col)
        elif self.out_col != 0 and link is not None:
            raise ValueError("out_col on a link decoder plan is not supported")
        self.desc = ForwardPlanDesc(
            cols=self.cols, n_rel=self.n_rel, n0=n0,
            n_deg_edges=int(arr["deg_src"].size), n_layers=L,
            layers=self._layers, n_head=len(program.head), head=self._head,
            out_col=program.out_col if self._cls is not None else self.out_col)
        self._i32(self.desc, "f0_node", fr[0])
        self._i32(self.desc, "deg_ptr", arr["deg_ptr"])
        self._i32(self.desc, "deg_src", arr["deg_src"] if arr["deg_src"].size else np.zeros(1))
        if self.edge_masks:
            self.desc.edge_masks = 1
            self._i32(self.desc, "deg_eid", arr["deg_eid"] if arr["deg_eid"].size else np.zeros(1))
        self.link = link
        if link is not None:
            a, b, act = link[:3]
            if not (0 <= a < self.n_out and 0 <= b < self.n_out):
                raise ValueError("link decoder targets out of range")
            self.desc.edge_dot, self.desc.dot_a, self.desc.dot_b = 1, int(a), int(b)
            self.desc.dot_act = ACT[act]
            if len(link) > 3 and link[3] is not None:
                # DistMult: the query relation's embedding, zero-padded to the last layer's width
                n_real = program.head[-1].weight.shape[0] if program.head else program.convs[-1].f_out
                d = torch.as_tensor(link[3]).detach().reshape(-1)
                if d.numel() != n_real:
                    raise ValueError(f"link scale vector of {d.numel()} entries on an output of "
                                     f"width {n_real}")
                dp = torch.zeros(prev_pad, dtype=torch.float32, device=device)
                dp[:n_real] = d.to(device=device, dtype=torch.float32)
                self._keep.append(dp)
                self.desc.dot_scale = dp.data_ptr()
            self.n_out = 1
        if self.pool is not None:
            self.n_out = 1  # forward returns [rows, 1], as link plans do
        self.n_targets = self.n_out
        if classes == "all":
            self.n_out = self.n_targets * self.n_classes  # (target, class) order
        self._upload_i32()
        # edge weights (xpgnn.h, xpg_edge_weights): every array in one upload
        self._weights = None
        self.weight_arrays = None
        if w_np is not None:
            wa = weight_arrays(arr, rel_np[0][0], rel_np[0][1], w_np)
            self.weight_arrays = wa
            nz = lambda a: a if a.size else np.zeros(1, np.float32)
            parts = [nz(wa["deg_w"]), nz(wa["loop_w"])]
            for lay in wa["layers"]:
                parts += [nz(lay[k]) for k in ("agg_w", "self_sum", "self_wmax", "self_wmin")]
            offs = np.concatenate([[0], np.cumsum([(a.size + 15) // 16 * 16 for a in parts])]).astype(np.int64)
            host = np.zeros(int(offs[-1]), dtype=np.float32)
            for a, o in zip(parts, offs):
                host[o:o + a.size] = a
            buf = h2d(host, device)
            self._keep.append(buf)
            at = lambda i: buf.data_ptr() + 4 * int(offs[i])
            self._layer_weights = (_lib.LayerWeights * L)()
            for li in range(L):
                lw = self._layer_weights[li]
                lw.agg_w, lw.self_sum, lw.self_wmax, lw.self_wmin = (at(2 + 4 * li + j) for j in range(4))
            self._weights = _lib.EdgeWeights(deg_w=at(0), loop_w=at(1), layers=self._layer_weights)
        # edge features (xpgnn.h, xpg_edge_feats): every table in one upload
        self._feats = None
        self.edge_feature_arrays = None
        if ea_np is not None:
            # a resource guard, before anything is built: rows of f_in_pad floats per CSR entry of
            # every SUM layer (twice for layer 1, which also stores the messages)
            need = sum(4 * _rup(c.f_in, 32) * (len(lay["agg_eid"]) + len(lay["self_eid"])) * (2 if li == 0 else 1)
                       for li, (c, lay) in enumerate(zip(program.convs, arr["layers"]))
                       if any(t.kind == "sum" for t in c.terms))
            if need > _EDGE_TABLE_MAX_BYTES:
                raise ValueError(f"edge-feature tables of {need >> 20} MiB exceed "
                                 f"{_EDGE_TABLE_MAX_BYTES >> 20} MiB")
            x0 = sub_feat.detach().to(dtype=torch.float32).cpu().numpy()[np.asarray(fr[0], dtype=np.int64)]
            fa = edge_feature_arrays(arr, program.convs, ea_np, x0)
            self.edge_feature_arrays = fa
            names = ("agg_e", "self_e", "msg_rows")
            parts = [(li, k, lay[k].reshape(-1)) for li, lay in enumerate(fa) if lay is not None
                     for k in names if k in lay]
            parts = [(li, k, a if a.size else np.zeros(1, np.float32)) for li, k, a in parts]
            offs = np.concatenate([[0], np.cumsum([(a.size + 15) // 16 * 16 for _, _, a in parts])]).astype(np.int64)
            host = np.zeros(int(offs[-1]), dtype=np.float32)
            for (_, _, a), o in zip(parts, offs):
                host[o:o + a.size] = a
            buf = h2d(host, device)
            self._keep.append(buf)
            self._layer_efeat = (_lib.LayerEfeat * L)()
            for (li, k, _), o in zip(parts, offs):
                setattr(self._layer_efeat[li], k, buf.data_ptr() + 4 * int(o))
            self._feats = _lib.EdgeFeats(layers=self._layer_efeat)
        self._ws = None
        self._ws_stream = None  # raw handle of the stream that last used self._ws

    def _program_tensor(self, program, key, make):
        """Device tensors derived from the program's weights alone (padded biases, the stacked
        dense weights of layers >= 1, head layers): built once per (program, device) and shared by
        every plan of that program (pipeline.compiled_program reuses a program while the module's
        parameters are unchanged), so a new query's plan only builds its own arrays and tables."""
        cache = program.__dict__.setdefault("_device_tensors", {})
        k = (str(self.device),) + key
        if k not in cache:
            cache[k] = make()
        return cache[k]

    def _i32(self, obj, field, a):
        """Stage an int32 array for descriptor field `obj.field`; `_upload_i32` moves every
        staged array to the device in ONE host -> device copy (a plan has ~15-25 of them: one
        synchronous copy each was ~0.4 ms of Explainer.run) and fills the pointers."""
        self._staged.append((obj, field, np.ascontiguousarray(a, dtype=np.int32).reshape(-1)))

    def _upload_i32(self):
        sizes = [(a.size + 15) // 16 * 16 for _, _, a in self._staged]  # 64-B aligned slices
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        host = np.zeros(int(offs[-1]), dtype=np.int32)
        for (_, _, a), o in zip(self._staged, offs):
            host[o:o + a.size] = a
        buf = h2d(host, self.device)
        self._keep.append(buf)
        self.int_arrays = buf  # every staged array, one allocation
        base = buf.data_ptr()
        for (obj, field, _), o in zip(self._staged, offs):
            setattr(obj, field, base + 4 * int(o))
        self._staged = []

    def device_bytes(self):
        """Device memory the plan holds: its arrays, tables, weights and forward workspace."""
        held = self._keep + ([self._ws] if self._ws is not None else [])
        return sum(t.numel() * t.element_size() for t in held)

    def _entry(self, name):
        """The entry point and its leading arguments: `name`(plan, ...), or with post-ops
        `name`_post(plan, post records, ...)."""
        if self._cls is not None:  # `name`_c(plan, post records, weights, features (each or NULL), class readout, ...)
            return name + "_c", (ctypes.byref(self.desc), self._post,
                                 ctypes.byref(self._weights) if self._weights is not None else None,
                                 ctypes.byref(self._feats) if self._feats is not None else None,
                                 ctypes.byref(self._cls))
        if self._feats is not None:  # `name`_e(plan, post records or NULL, NULL weights, features, ...)
            return name + "_e", (ctypes.byref(self.desc), self._post, None, ctypes.byref(self._feats))
        if self._weights is not None:  # `name`_w(plan, post records or NULL, weights, ...)
            return name + "_w", (ctypes.byref(self.desc), self._post, ctypes.byref(self._weights))
        if self._post is None:
            return name, (ctypes.byref(self.desc),)
        return name + "_post", (ctypes.byref(self.desc), self._post)

    def workspace_bytes(self, rows):
        n = ctypes.c_size_t(0)
        name, lead = self._entry("xpg_forward_workspace")
        _lib.check(getattr(_lib.load(), name)(*lead, rows, ctypes.byref(n)))
        return n.value

    def describe(self, rows):
        """The path forward() takes for `rows` mask rows under the current environment: "rows",
        "fused", "unfused", or "wide l1=<kernel> l2=<kernel>" with the kernels' template
        arguments; a plan with post-ops: "unfused post<l>=k_post<NORM,RES> ..." (each post layer's
        kernel); a weighted plan: "unfused weights=k_degree_w+k_agg_w" before those tokens; an
        edge-featured plan: "unfused efeat=k_agg_e" before them; a plan with a class readout ends in
        " class=k_class_out<kind,one|all>".  A host query of the library's own dispatch (nothing is launched); raises
        where forward() would refuse the plan (XPG_FORWARD_STRICT=1)."""
        buf = ctypes.create_string_buffer(1024)
        name, lead = self._entry("xpg_forward_describe")
        _lib.check(getattr(_lib.load(), name)(*lead, rows, buf, len(buf)))
        return buf.value.decode()

    def kernels(self, rows):
        """What forward() launches for `rows` mask rows under the current environment, by
        instantiation and run-time form (xpg_forward_kernels, a host query of the picks the launches
        use), e.g. "rows k_rows_forward<4,0> layers=2 bits=lds w2=global head=lds,global",
        "fused k_fused_forward<4> layers=3 tpp=8,4" or "unfused l1=k_agg_l1_rows<64,1>x2
        l2=k_agg<0,24,1>+k_dense<3,0>g1 head=k_dense<1,1>g1 tail=epilogue"; the wide path reads as
        in describe().  Raises where forward() would refuse the plan."""
        buf = ctypes.create_string_buffer(1024)
        lib = _lib.load()
        if self._post is None and self._weights is None and self._feats is None and self._cls is None:
            _lib.check(lib.xpg_forward_kernels(ctypes.byref(self.desc), rows, buf, len(buf)))
        else:
            _lib.check(lib.xpg_forward_kernels_c(
                ctypes.byref(self.desc), self._post,
                ctypes.byref(self._weights) if self._weights is not None else None,
                ctypes.byref(self._feats) if self._feats is not None else None,
                ctypes.byref(self._cls) if self._cls is not None else None, rows, buf, len(buf)))
        return buf.value.decode()

    def forward(self, bits: torch.Tensor, max_ws_bytes=8 << 30, out: torch.Tensor = None,
                workspace: torch.Tensor = None) -> torch.Tensor:
        """y [rows, n_out] fp32: model output at each target of the last conv layer, per mask
        row (wlm.py:349-436 for one batch, all batches at once).  `out`: a contiguous fp32
        [rows, n_out] tensor to write y into (no allocation once the workspace exists).
        `workspace`: a uint8 device tensor of at least workspace_bytes(rows) to use instead of the
        plan's own — forwards running at the same time on different streams need one each (the
        workspace holds the launch's block-scheduling counters).  Without it, forwards on
        different streams through one plan are ordered: each waits for the stream that used the
        plan's workspace last."""
        _lib.require_device(bits, "bits")
        rows = bits.shape[0]
        if out is None:
            y = torch.empty((rows, self.n_out), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (rows, self.n_out) or \
                not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [rows, n_out] tensor")
        else:
            y = out
        if rows == 0:
            return y
        st = _lib.stream_of(self.device)
        fwd, lead = self._entry("xpg_masked_forward")
        if workspace is not None:
            if workspace.dtype != torch.uint8 or workspace.device != self.device or \
                    workspace.numel() < self.workspace_bytes(rows):
                raise ValueError("workspace must be a uint8 device tensor of workspace_bytes(rows)")
            call(fwd, *lead, ptr(bits), rows, ptr(y), ptr(workspace), workspace.numel(), st)
            return y
        w1, w2 = self.workspace_bytes(1), self.workspace_bytes(2)
        per_row = max(0, w2 - w1)  # 0: a rows-independent workspace (the wide 32-row passes)
        fixed = max(0, w1 - per_row)
        chunk = rows if per_row == 0 else \
            max(1, min(rows, max(0, max_ws_bytes - fixed) // per_row))
        need = self.workspace_bytes(chunk)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        # the plan's own workspace (and the block counters in it) is reused in stream order: a
        # forward on another stream than the last user's first waits for what that stream has
        # queued (two streams forwarding through one plan then take turns instead of racing)
        cur = st.value or 0  # 0: the null stream
        if self._ws_stream is not None and self._ws_stream != cur and \
                not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(self.device).wait_stream(
                torch.cuda.ExternalStream(self._ws_stream, device=self.device))
        self._ws_stream = cur
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            call(fwd, *lead, ptr(bits[r0:r0 + n]), n, ptr(y[r0:r0 + n]), ptr(self._ws),
                 self._ws.numel(), st)
        return y


# ----------------------------------------------------------------------------- surrogate
_WS = {}


def _workspace(dev, nbytes):
    """Reusable per-device scratch (stream-ordered reuse: every user is on the current stream)."""
    key = (dev.type, dev.index)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        # grown with 25 % headroom, in whole MiB (>= 4 MiB): queries of somewhat larger sizes
        # reuse it instead of each first call on a larger one paying a device allocation; an
        # allocation the headroom does not fit falls back to the exact size
        _WS.pop(key, None)
        del t
        grow = max(4 << 20, (nbytes + nbytes // 4 + (1 << 20) - 1) >> 20 << 20)
        try:
            t = torch.empty(grow, dtype=torch.uint8, device=dev)
        except torch.OutOfMemoryError:
            t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _WS[key] = t
    return t


def check_fit_status(status):
    """Raise FitExchangeError when a fit's device status word (see wlm_fit) is nonzero.  Reads
    the word, i.e. waits for the stream to reach the end of that fit."""
    if int(status.max().item()) != 0:
        raise _lib.FitExchangeError(
            "surrogate fit: the multi-workgroup exchange timed out (workgroups not co-resident, "
            "e.g. another kernel or process held the GPU's CUs); the fitted weights are invalid. "
            "XPG_WLM=single selects the single-workgroup fit.")


_STATUS_HOST = {}


def status_to_host(status):
    """Queue a copy of a fit's device status word into pinned host memory (no host wait) and
    return the host tensor: once a later synchronising read on the stream (e.g. the results'
    .cpu()) has returned, check_status_host(...) reads it without a second synchronisation."""
    key = status.device.index
    h = _STATUS_HOST.get(key)
    if h is None:
        h = _STATUS_HOST[key] = torch.zeros(1, dtype=torch.int32, pin_memory=True)
    h.copy_(status.reshape(-1)[:1], non_blocking=True)
    return h


def check_status_host(h):
    """check_fit_status on a word copied by status_to_host (after the stream reached the copy)."""
    if int(h[0]) != 0:
        check_fit_status(torch.ones(1, dtype=torch.int32))


WLM_KINDS = {0: "single", 1: "multi", 2: "grid", 3: "grid_fused"}


def wlm_plan(n_fits, rows, cols, batch):
    """(kind, parts) of the fit kernel a shape takes on the current device (xpg_wlm_plan):
    kind "single" (one workgroup per fit), "multi" (`parts` co-resident workgroups per fit),
    "grid" (the many-column streaming fit, three launches per step) or "grid_fused" (the
    many-column fit as one persistent launch per fit over `parts` workgroups); the grid kinds
    have no prepared form."""
    kind, parts = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().xpg_wlm_plan(int(n_fits), int(rows), int(cols), int(batch),
                                        ctypes.byref(kind), ctypes.byref(parts)))
    return WLM_KINDS[kind.value], parts.value


# every variant name wlm_describe can report (the library's own list: xpg_wlm_variants, checked
# against this tuple by tests/test_fit_cpu.py): k_wlm_fit<CPT, STAGE>, k_wlm_fit_mc<C, G>, the
# three-launch grid fit and k_gw_fused
WLM_VARIANTS = tuple(
    [f"single<CPT={c},{s}>" for s in ("stage", "nostage") for c in (1, 2, 4, 8, 16)] +
    [f"multi<C={c},G={g}>" for c in (1, 2, 4) for g in (1, 2, 4)] + ["grid3", "grid_fused"])


def wlm_describe(n_fits, rows, cols, batch):
    """The fit kernel wlm_fit launches for a shape on the current device under the current
    XPG_WLM setting, as text (xpg_wlm_describe): the variant (one of WLM_VARIANTS) and the
    planner's split, e.g. "single<CPT=2,stage> n_bs=3 n_ds=1", "multi<C=1,G=1> P=13 wpp=3 ds=1",
    "grid3 n_wg=9", "grid_fused ch=1 nwg=9 nrbp=8".  A host query of the launcher's own decision
    (nothing is launched)."""
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().xpg_wlm_describe(int(n_fits), int(rows), int(cols), int(batch), buf, len(buf)))
    return buf.value.decode()


def wlm_variants():
    """The library's list of variant names (xpg_wlm_variants); equals WLM_VARIANTS."""
    buf = ctypes.create_string_buffer(2048)
    _lib.check(_lib.load().xpg_wlm_variants(buf, len(buf)))
    return tuple(buf.value.decode().split())


class PreparedFit:
    """A fresh surrogate fit (`wlm_fit` from w0) split in its two launches on static buffers of
    one shape (xpg_wlm_prepare / xpg_wlm_fit_prepared, ABI v12): `prepare` runs the prologue
    (per-step constants, column bit vectors, w = w0, zero Adam moments), `fit` the Adam steps and
    returns w [F, cols].  Nothing is allocated after construction, so both can be captured on
    any stream; with two instances the next fit is prepared while the current one runs.
    `status` is the device status word (check_fit_status; sticky over every fit of the
    instance).  Shapes that take the many-column grid fit have no prepared form: ValueError at
    construction (use wlm_fit)."""

    def __init__(self, n_fits, rows, cols, batch, params, device):
        self.kind, self.parts = wlm_plan(n_fits, rows, cols, batch)
        if self.kind.startswith("grid"):
            raise ValueError(f"PreparedFit: {cols} columns take the many-column grid fit, which "
                             "has no prologue / prepared form; use wlm_fit")
        self.shape = (int(n_fits), int(rows), int(cols), int(batch))
        n = ctypes.c_size_t(0)
        _lib.check(_lib.load().xpg_wlm_workspace(n_fits, rows, cols, batch, ctypes.byref(n)))
        self.ws = torch.empty(max(n.value, 1), dtype=torch.uint8, device=device)
        self.w = torch.empty((n_fits, cols), dtype=torch.float32, device=device)
        self.m = torch.empty_like(self.w)
        self.v = torch.empty_like(self.w)
        self.losses = torch.empty((n_fits, math.ceil(rows / batch)), dtype=torch.float64, device=device)
        self.best = torch.empty(n_fits, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.p = WlmParams(lr=abs(float(params["lr"])), l1_lambda=float(params["l1_lambda"]), beta1=0.9,
                           beta2=0.999, eps=1e-8, weight_decay=1e-2)

    def _check(self, name, t, dtype, numel):
        if t.dtype != dtype or t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of {numel} elements")

    def prepare(self, bits, y, kernel, w0):
        F, R, S, B = self.shape
        self._check("bits", bits, torch.int32, F * R * words_of(S))
        self._check("y", y, torch.float32, F * R)
        self._check("kernel", kernel, torch.float64, F * R)
        self._check("w0", w0, torch.float32, F * S)
        call("xpg_wlm_prepare", F, ptr(bits), R, S, B, ptr(y), ptr(kernel), ctypes.byref(self.p),
             ptr(w0), ptr(self.w), ptr(self.m), ptr(self.v), ptr(self.ws), self.ws.numel(),
             _lib.stream_of(bits.device))

    def fit(self, bits, kernel):
        F, R, S, B = self.shape
        self._check("bits", bits, torch.int32, F * R * words_of(S))
        self._check("kernel", kernel, torch.float64, F * R)
        call("xpg_wlm_fit_prepared", F, ptr(bits), R, S, B, ptr(kernel), ctypes.byref(self.p),
             ptr(self.w), ptr(self.m), ptr(self.v), ptr(self.losses), ptr(self.best), ptr(self.status),
             ptr(self.ws), self.ws.numel(), _lib.stream_of(bits.device))
        return self.w

    def fit_steps(self, bits, kernel):
        """`fit` without its losses / best epoch / status launch (xpg_wlm_fit_steps, ABI v17):
        only the Adam steps on the current stream; call `losses` afterwards (any stream ordered
        after this one) before the workspace is prepared again."""
        F, R, S, B = self.shape
        self._check("bits", bits, torch.int32, F * R * words_of(S))
        self._check("kernel", kernel, torch.float64, F * R)
        call("xpg_wlm_fit_steps", F, ptr(bits), R, S, B, ptr(kernel), ctypes.byref(self.p),
             ptr(self.w), ptr(self.m), ptr(self.v), ptr(self.ws), self.ws.numel(),
             _lib.stream_of(bits.device))
        return self.w

    def finish(self, kernel):
        """The losses, first best epoch and status word of the last `fit_steps`
        (xpg_wlm_fit_losses) on the current stream."""
        F, R, S, B = self.shape
        self._check("kernel", kernel, torch.float64, F * R)
        call("xpg_wlm_fit_losses", F, R, S, B, ptr(kernel), ctypes.byref(self.p), ptr(self.losses),
             ptr(self.best), ptr(self.status), ptr(self.ws), self.ws.numel(),
             _lib.stream_of(kernel.device))
        return self.losses, self.best


def wlm_fit(bits, cols, batch, y, kernel, w0, params, m0=None, v0=None, step0=0, check=True,
            status=None):
    """train_model (wlm.py:132-278) epoch loop on device for one or many independent fits.

    bits [R, W] or [F, R, W]; y / kernel [R] or [F, R]; w0 [S] or [F, S].  Returns
    (w, losses, best_epoch, adam_m, adam_v) with the same leading fit dimension (if any).

    check=True reads the fit's status word and raises FitExchangeError if the multi-workgroup
    exchange failed (one stream sync).  check=False leaves that to the caller: pass `status`
    (device int32 [1], zeroed once) and call check_fit_status(status) later (e.g. after a timed
    region); the word is sticky (ABI v13), so it reports a failure of any fit that used it."""
    dev = bits.device
    batched = bits.dim() == 3
    F = bits.shape[0] if batched else 1
    rows = bits.shape[-2]
    if batch <= 0:
        raise ValueError("batch_size should be a positive integer value, but got "
                         f"batch_size={batch}")
    nsteps = math.ceil(rows / batch)
    # a fresh fit (no Adam state handed in) starts from w0 inside the fit's prologue kernel
    # (xpg_wlm_fit_from): no copy / fill launches on the latency-bound chain
    fresh = m0 is None and v0 is None and int(step0) == 0
    w0f = w0.detach().to(device=dev, dtype=torch.float32).reshape(F, cols).contiguous()
    if fresh:
        w = torch.empty((F, cols), dtype=torch.float32, device=dev)
        m = torch.empty((F, cols), dtype=torch.float32, device=dev)
        v = torch.empty((F, cols), dtype=torch.float32, device=dev)
    else:
        w = w0f.clone()
        m = torch.zeros((F, cols), dtype=torch.float32, device=dev) if m0 is None else \
            m0.reshape(F, cols).clone()
        v = torch.zeros((F, cols), dtype=torch.float32, device=dev) if v0 is None else \
            v0.reshape(F, cols).clone()
    losses = torch.empty((F, nsteps), dtype=torch.float64, device=dev)
    best = torch.empty(F, dtype=torch.int32, device=dev)
    p = WlmParams(lr=abs(float(params["lr"])), l1_lambda=float(params["l1_lambda"]), beta1=0.9,
                  beta2=0.999, eps=1e-8, weight_decay=1e-2)
    yy = y.to(device=dev, dtype=torch.float32).reshape(F, rows).contiguous()
    kk = kernel.to(device=dev, dtype=torch.float64).reshape(F, rows).contiguous()
    bb = bits.contiguous()
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().xpg_wlm_workspace(F, rows, cols, batch, ctypes.byref(n)))
    ws = _workspace(dev, n.value)
    if status is None:  # sticky word (the fit ORs its error into it): starts at 0
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if fresh:
        call("xpg_wlm_fit_from", F, ptr(bb), rows, cols, batch, ptr(yy), ptr(kk), ctypes.byref(p),
             ptr(w0f), ptr(w), ptr(m), ptr(v), ptr(losses), ptr(best), ptr(status), ptr(ws),
             ws.numel(), _lib.stream_of(dev))
    else:
        call("xpg_wlm_fit", F, ptr(bb), rows, cols, batch, ptr(yy), ptr(kk), ctypes.byref(p),
             int(step0), ptr(w), ptr(m), ptr(v), ptr(losses), ptr(best), ptr(status), ptr(ws),
             ws.numel(), _lib.stream_of(dev))
    if check:
        check_fit_status(status)
    if not batched:
        return w[0], losses[0], best[0:1], m[0], v[0]
    return w, losses, best, m, v
