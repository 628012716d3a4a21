"""Shared inputs and case list of the rows / fused / multi-kernel forward variant tests
(tests/test_forward_variants_cpu.py, tests/test_gpu_forward_variants.py).

One graph family, 300 nodes:
* region A = nodes 0..259 with 600 random edges whose targets are 3..259;
* node 0: a hub target of in-degree 70, node 1: a hub target of in-degree 130 (the rows kernel's
  degree pass hands a node's in-edges out in 64-edge windows and its layer-1 loop batches 64
  in-edges, 4 at a time: one and two windows crossed, neither a multiple of 4);
* node 2: out-edges only (a target without in-edges);
* cluster C = nodes 260..299 with 70 random edges inside it: queries there have receptive fields
  of ~20 nodes, the frontier size at which the rows kernel's LDS arithmetic leaves room for one
  weight matrix and not for the next (its run-time forms);
* 10 explicit self-loops and 10 duplicated edges (7 + 3 over A and C, none at the hubs; the random
  draw repeats 2 more edges of its own).
130 mask rows = two 64-row blocks + a tail of 2: row 0 all-on, row 1 all-off, row 2 at 3 %
density, the rest with per-row keep probabilities in (0.2, 0.9).

A case = a ConvStack, a query set, an environment and the exact text ForwardPlan.kernels() must
report for it.  The fp64 reference is oracle.masked_all_outputs (gcn, sage) or
aggr_ref.union_outputs (the sum / max families) on the reference's union graph, cut to the case's
query columns.  Everything here runs on the host: descriptor() builds the case's plan descriptor
from the host-built receptive-field arrays and the compiled program, with the sizes and term
kinds the device plan has and device pointers that are only ever tested for NULL."""
import collections
import functools

import numpy as np
import torch

import oracle
from golden_utils import oracle_spec

S, ROWS = 300, 130
HUB70, HUB130, NO_IN = 0, 1, 2
ATOL = 1e-5
PTR = 256  # a non-NULL "device pointer": never dereferenced by a host query
ENV = ("XPG_FORWARD", "XPG_FORWARD_STRICT", "XPG_DIAGNOSTICS", "XPG_AGG_GENERIC", "XPG_L1_DBG")


@functools.lru_cache(maxsize=None)
def graph():
    """edge_index int64 [2, E] (read-only)."""
    rng = np.random.default_rng(77)
    a = np.stack([rng.integers(0, 260, 600), rng.integers(3, 260, 600)])
    c = np.stack([rng.integers(260, S, 70), rng.integers(260, S, 70)])
    a, c = a[:, a[0] != a[1]], c[:, c[0] != c[1]]
    loops = np.concatenate([rng.choice(np.arange(3, 260), 7, replace=False),
                            rng.choice(np.arange(260, S), 3, replace=False)])
    dup = np.concatenate([a[:, rng.choice(a.shape[1], 7, replace=False)],
                          c[:, rng.choice(c.shape[1], 3, replace=False)]], 1)
    hubs = [np.stack([rng.choice(np.arange(3, 260), deg, replace=False), np.full(deg, node)])
            for node, deg in ((HUB70, 70), (HUB130, 130))]
    ei = np.concatenate([a, c, np.stack([loops, loops]), dup] + hubs, 1)
    # the hubs' last in-edges stay last (hub_edge_dropped removes them); the rest is shuffled
    n_free = ei.shape[1] - 200
    ei = np.concatenate([ei[:, rng.permutation(n_free)], ei[:, n_free:]], 1).astype(np.int64)
    indeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=S)
    assert indeg[HUB70] == 70 and indeg[HUB130] == 130 and indeg[NO_IN] == 0
    assert (ei[0] == NO_IN).any() and int((ei[0] == ei[1]).sum()) == 10
    ei.setflags(write=False)
    return ei


def hub_edge_dropped(hub):
    """The graph without the last in-edge of `hub`."""
    ei = graph()
    last = np.flatnonzero(ei[1] == hub)[-1]
    return np.delete(ei, last, axis=1)


@functools.lru_cache(maxsize=None)
def features(f_in):
    x = torch.randn((S, f_in), generator=torch.Generator().manual_seed(5))
    return x


@functools.lru_cache(maxsize=None)
def masks():
    rng = np.random.default_rng(3)
    m = rng.random((ROWS, S)) < rng.uniform(0.2, 0.9, (ROWS, 1))
    m[0] = True
    m[1] = False
    m[2] = rng.random(S) < 0.03
    m.setflags(write=False)
    return m


# query sets (every one holds the target without in-edges)
QUERIES = {
    "hubs": (HUB70, HUB130, NO_IN, 17),         # both hubs
    "hub70": (HUB70, NO_IN, 17),
    "hub130": (HUB130, NO_IN),
    "quiet": (NO_IN, 265, 281),                 # cluster C: a receptive field of ~20 nodes
    # sage 64, one layer: the rows kernel's tables leave fewer than the 704 floats of the staged
    # mask rows ("fill"); one more target and they no longer fit at all ("overfill")
    "fill": (HUB70, HUB130, NO_IN, 3, 4, 5, 6),
    "overfill": (HUB70, HUB130, NO_IN, 3, 4, 5, 6, 7),
}

# kind, dims (dims[0] = input features), fc (head widths, fc[0] = dims[-1]), query set, relations,
# output column, environment, mask rows, weights seed (11, or the first seed from 12 at which the
# fp64 reference alone meets test_forward_variants_cpu's range and hub-edge conditions with a 1.5x
# margin), the text kernels() must report
Case = collections.namedtuple("Case", "kind dims fc queries n_rel out_col env rows seed want")


def _c(kind, dims, fc, queries, want, env=None, n_rel=1, out_col=0, rows=ROWS, seed=11):
    return Case(kind, tuple(dims), tuple(fc), queries, n_rel, out_col, dict(env or {}), rows, seed, want)


ROWS_ENV = {"XPG_FORWARD": "rows", "XPG_FORWARD_STRICT": "1"}
FUSED_ENV = {"XPG_FORWARD": "fused", "XPG_FORWARD_STRICT": "1"}
UNFUSED_ENV = {"XPG_FORWARD": "unfused", "XPG_FORWARD_STRICT": "1"}
GENERIC_ENV = dict(UNFUSED_ENV, XPG_DIAGNOSTICS="1", XPG_AGG_GENERIC="1")

CASES = {}
# a plan the fused kernel declines (its two 166 x 256 layer-1 tables alone pass the LDS limit): an
# error under XPG_FORWARD_STRICT=1, the multi-kernel path without it
FUSED_DECLINED = _c("sage", (16, 256), (256, 1), "hubs",
                    "unfused l1=k_agg_l1_rows<64,1>x4 head=k_dense<1,0>g1 tail=k_take_col")
# rows kernel, XPG_FORWARD unset (the default path of small frontiers): the six instantiations,
# 1 and 2 layers, GCN / mean+root / sum+root, two relations, 1 / 2 / 4 head layers, an output column
CASES['rows-gcn32-l1-hubs'] = _c('gcn', (16, 32), (32, 1), 'hubs',
    'rows k_rows_forward<2,0> layers=1 bits=lds w2=- head=lds')
CASES['rows-gcn32-l2-hub130'] = _c('gcn', (16, 32, 32), (32, 1), 'hub130',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=lds')
CASES['rows-sage64-l1-hub130'] = _c('sage', (16, 64), (64, 1), 'hub130',
    'rows k_rows_forward<4,0> layers=1 bits=lds w2=- head=lds')
CASES['rows-sage64-l2-quiet'] = _c('sage', (16, 64, 32), (32, 1), 'quiet',
    'rows k_rows_forward<4,0> layers=2 bits=lds w2=lds head=lds')
CASES['rows-sage128-l1-hub70'] = _c('sage', (16, 128), (128, 1), 'hub70',
    'rows k_rows_forward<8,0> layers=1 bits=lds w2=- head=lds')
CASES['rows-gcn128-l2-quiet'] = _c('gcn', (16, 128, 64), (64, 1), 'quiet',
    'rows k_rows_forward<8,0> layers=2 bits=lds w2=lds head=lds')
CASES['rows-add32-l1-hubs'] = _c('sage-add', (16, 32), (32, 1), 'hubs',
    'rows k_rows_forward<2,1> layers=1 bits=lds w2=- head=lds')
CASES['rows-add32-l2-hub70'] = _c('sage-add', (16, 32, 32), (32, 1), 'hub70',
    'rows k_rows_forward<2,1> layers=2 bits=lds w2=lds head=lds')
CASES['rows-add64-l1-hub130'] = _c('sage-add', (16, 64), (64, 1), 'hub130',
    'rows k_rows_forward<4,1> layers=1 bits=lds w2=- head=lds')
CASES['rows-add128-l1-hub70'] = _c('sage-add', (16, 128), (128, 1), 'hub70',
    'rows k_rows_forward<8,1> layers=1 bits=lds w2=- head=lds')
CASES['rows-sage32-rel2-l1-hub130'] = _c('sage', (16, 32), (32, 1), 'hub130',
    'rows k_rows_forward<2,0> layers=1 bits=lds w2=- head=lds', n_rel=2)
CASES['rows-gcn32-rel2-l2-quiet'] = _c('gcn', (16, 32, 32), (32, 1), 'quiet',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=lds', n_rel=2)
CASES['rows-gcn48-head2-hub130'] = _c('gcn', (16, 48), (48, 16, 1), 'hub130',
    'rows k_rows_forward<4,0> layers=1 bits=lds w2=- head=lds,lds')
CASES['rows-add32-head4-hubs'] = _c('sage-add', (16, 32), (32, 32, 16, 8, 1), 'hubs',
    'rows k_rows_forward<2,1> layers=1 bits=lds w2=- head=lds,lds,lds,lds', seed=22)
CASES['rows-gcn32-col2-hubs'] = _c('gcn', (16, 32), (32, 4), 'hubs',
    'rows k_rows_forward<2,0> layers=1 bits=lds w2=- head=lds', out_col=2)
CASES['rows-sage32-head2-col3-hub70'] = _c('sage', (16, 32, 32), (32, 16, 5), 'hub70',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=lds,lds', out_col=3, seed=13)
CASES['rows-gcn32-l2-rows1'] = _c('gcn', (16, 32, 32), (32, 1), 'hub130',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=lds', rows=1)
# its run-time forms, each reached by LDS arithmetic alone (try_rows_forward: 40,704 floats), and the
# plan one target too big, which the default path hands to the multi-kernel path
CASES['rows-form-bits-global'] = _c('sage', (16, 64), (64, 1), 'fill',
    'rows k_rows_forward<4,0> layers=1 bits=global w2=- head=global')
CASES['rows-form-w2-global'] = _c('sage', (16, 128, 128), (128, 1), 'quiet',
    'rows k_rows_forward<8,0> layers=2 bits=lds w2=global head=lds')
CASES['rows-form-head-global'] = _c('sage', (16, 64), (64, 1), 'hubs',
    'rows k_rows_forward<4,0> layers=1 bits=lds w2=- head=global')
CASES['rows-form-heads-global'] = _c('sage', (16, 32, 128), (128, 128, 128, 1), 'quiet',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=global,global,lds')
CASES['rows-form-head-global-lds'] = _c('sage', (16, 32, 128), (128, 128, 1), 'quiet',
    'rows k_rows_forward<2,0> layers=2 bits=lds w2=lds head=global,lds')
CASES['rows-too-big'] = _c('sage', (16, 64), (64, 1), 'overfill',
    'unfused l1=k_agg_l1_rows<64,1>x1 head=k_dense<1,0>g1 tail=k_take_col')
# fused kernel (XPG_FORWARD=fused): waves per block 8 / 4 / 2 by how many waves' scratch fits, 1-4
# layers, layer input widths 32 / 64 / 128 / 256 (8 / 4 / 2 / 1 targets per pass)
CASES['fused-gcn32-l1-hubs'] = _c('gcn', (16, 32), (32, 1), 'hubs',
    'fused k_fused_forward<8> layers=1 tpp=-', env=FUSED_ENV)
CASES['fused-sage128-l1-hub130'] = _c('sage', (16, 128), (128, 1), 'hub130',
    'fused k_fused_forward<8> layers=1 tpp=-', env=FUSED_ENV)
CASES['fused-sage256-l1-hub70'] = _c('sage', (16, 256), (256, 1), 'hub70',
    'fused k_fused_forward<2> layers=1 tpp=-', env=FUSED_ENV)
CASES['fused-gcn32-l2-hubs'] = _c('gcn', (16, 32, 32), (32, 1), 'hubs',
    'fused k_fused_forward<2> layers=2 tpp=8', env=FUSED_ENV)
CASES['fused-gcn64-l2-hub70'] = _c('gcn', (16, 64, 32), (32, 1), 'hub70',
    'fused k_fused_forward<2> layers=2 tpp=4', env=FUSED_ENV)
CASES['fused-gcn128-l2-quiet-col1'] = _c('gcn', (16, 128, 64), (64, 4), 'quiet',
    'fused k_fused_forward<8> layers=2 tpp=2', env=FUSED_ENV, out_col=1)
CASES['fused-gcn256-l2-quiet'] = _c('gcn', (16, 256, 32), (32, 1), 'quiet',
    'fused k_fused_forward<4> layers=2 tpp=1', env=FUSED_ENV)
CASES['fused-sage64-rel2-l2-quiet'] = _c('sage', (16, 64, 32), (32, 1), 'quiet',
    'fused k_fused_forward<8> layers=2 tpp=4', env=FUSED_ENV, n_rel=2)
CASES['fused-sage32-l3-quiet'] = _c('sage', (16, 32, 32, 32), (32, 16, 1), 'quiet',
    'fused k_fused_forward<8> layers=3 tpp=8,8', env=FUSED_ENV)
CASES['fused-sage32-l3-hub70'] = _c('sage', (16, 32, 32, 32), (32, 16, 1), 'hub70',
    'fused k_fused_forward<2> layers=3 tpp=8,8', env=FUSED_ENV, seed=21)
CASES['fused-gcn-l4-quiet'] = _c('gcn', (16, 32, 64, 128, 32), (32, 1), 'quiet',
    'fused k_fused_forward<8> layers=4 tpp=8,4,2', env=FUSED_ENV)
# multi-kernel path (XPG_FORWARD=unfused), layer 1 on k_agg_l1_rows<features per wave, ONE> x slices
# (ONE = 0: two aggregating terms) and the raw form of a MAX layer 1
CASES['unfused-l1rows-gcn32'] = _c('gcn', (16, 32), (32, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<32,1>x1 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1rows-sage64'] = _c('sage', (16, 64), (64, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x1 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1rows-gcn128'] = _c('gcn', (16, 128), (128, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x2 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1rows-sage256'] = _c('sage', (16, 256), (256, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x4 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1rows-gcn32-rel2'] = _c('gcn', (16, 32), (32, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<32,0>x1 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV, n_rel=2)
CASES['unfused-l1rows-sage64-rel2'] = _c('sage', (16, 64), (64, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,0>x1 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV, n_rel=2)
CASES['unfused-l1rows-gcn128-rel2'] = _c('gcn', (16, 128), (128, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,0>x2 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV, n_rel=2)
CASES['unfused-l1rows-add256-rel2'] = _c('sage-add', (16, 256), (256, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,0>x4 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV, n_rel=2)
CASES['unfused-raw-max'] = _c('sage-max', (16, 32, 32), (32, 1), 'hubs',
    'unfused l1=k_agg<0,8,1>+k_dense<1,0>g1 l2=k_agg<0,8,1>+k_dense<1,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-raw-max-f96'] = _c('sage-max', (96, 64), (64, 1), 'hubs',
    'unfused l1=k_agg<0,24,1>+k_dense<2,0>g1 head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
# layer 1 on the generic k_agg<1, LPS, 1>: by the diagnostics switch at the widths of k_agg_l1_rows,
# by width alone at 96 / 160 / 192 / 224
CASES['unfused-l1gen-32'] = _c('gcn', (16, 32), (32, 1), 'hubs',
    'unfused l1=k_agg<1,8,1> head=k_dense<1,0>g1 tail=k_take_col', env=GENERIC_ENV)
CASES['unfused-l1gen-64'] = _c('sage', (16, 64), (64, 1), 'hubs',
    'unfused l1=k_agg<1,16,1> head=k_dense<1,0>g1 tail=k_take_col', env=GENERIC_ENV)
CASES['unfused-l1gen-96'] = _c('gcn', (16, 96), (96, 1), 'hubs',
    'unfused l1=k_agg<1,24,1> head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1gen-128'] = _c('sage', (16, 128), (128, 1), 'hubs',
    'unfused l1=k_agg<1,32,1> head=k_dense<1,0>g1 tail=k_take_col', env=GENERIC_ENV)
CASES['unfused-l1gen-160'] = _c('gcn', (16, 160), (160, 1), 'hubs',
    'unfused l1=k_agg<1,40,1> head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1gen-192'] = _c('sage', (16, 192), (192, 1), 'hubs',
    'unfused l1=k_agg<1,48,1> head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1gen-224'] = _c('gcn', (16, 224), (224, 1), 'hubs',
    'unfused l1=k_agg<1,56,1> head=k_dense<1,0>g1 tail=k_take_col', env=UNFUSED_ENV)
CASES['unfused-l1gen-256'] = _c('sage', (16, 256), (256, 1), 'hubs',
    'unfused l1=k_agg<1,64,1> head=k_dense<1,0>g1 tail=k_take_col', env=GENERIC_ENV)
# layer-2 input width w1 -> k_agg<0, w1 / 4, 1>; layer-2 output width w2 -> k_dense<w2 / 32, 1> with
# the output column in its epilogue (1 column group, or 4 at 128 / 256)
CASES['unfused-l2-32-96-epi'] = _c('gcn', (16, 32, 96), (96, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<32,1>x1 l2=k_agg<0,8,1>+k_dense<3,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-64-160-epi'] = _c('sage', (16, 64, 160), (160, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x1 l2=k_agg<0,16,1>+k_dense<5,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-96-32-epi'] = _c('gcn', (16, 96, 32), (32, 1), 'hubs',
    'unfused l1=k_agg<1,24,1> l2=k_agg<0,24,1>+k_dense<1,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-128-64-epi'] = _c('sage', (16, 128, 64), (64, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x2 l2=k_agg<0,32,1>+k_dense<2,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-160-192-epi'] = _c('gcn', (16, 160, 192), (192, 1), 'hubs',
    'unfused l1=k_agg<1,40,1> l2=k_agg<0,40,1>+k_dense<6,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-192-224-epi'] = _c('sage', (16, 192, 224), (224, 1), 'hubs',
    'unfused l1=k_agg<1,48,1> l2=k_agg<0,48,1>+k_dense<7,1>g1 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-224-128-epi'] = _c('gcn', (16, 224, 128), (128, 1), 'hubs',
    'unfused l1=k_agg<1,56,1> l2=k_agg<0,56,1>+k_dense<1,1>g4 head=- tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-256-256-epi'] = _c('sage', (16, 256, 256), (256, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x4 l2=k_agg<0,64,1>+k_dense<2,1>g4 head=- tail=epilogue', env=UNFUSED_ENV)
# the same with a head layer of width v: k_dense<w2 / 32, 0> on the conv layer, k_dense<v / 32, 1> on
# the head layer
CASES['unfused-l2-32-32-head96'] = _c('sage', (16, 32, 32), (32, 96, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<32,1>x1 l2=k_agg<0,8,1>+k_dense<1,0>g1 head=k_dense<3,1>g1 tail=epilogue', env=UNFUSED_ENV, seed=198)
CASES['unfused-l2-64-64-head160'] = _c('gcn', (16, 64, 64), (64, 160, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x1 l2=k_agg<0,16,1>+k_dense<2,0>g1 head=k_dense<5,1>g1 tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-96-96-head32'] = _c('sage', (16, 96, 96), (96, 32, 1), 'hubs',
    'unfused l1=k_agg<1,24,1> l2=k_agg<0,24,1>+k_dense<3,0>g1 head=k_dense<1,1>g1 tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-128-160-head64'] = _c('gcn', (16, 128, 160), (160, 64, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x2 l2=k_agg<0,32,1>+k_dense<5,0>g1 head=k_dense<2,1>g1 tail=epilogue', env=UNFUSED_ENV)
CASES['unfused-l2-160-192-head192'] = _c('sage', (16, 160, 192), (192, 192, 1), 'hubs',
    'unfused l1=k_agg<1,40,1> l2=k_agg<0,40,1>+k_dense<6,0>g1 head=k_dense<6,1>g1 tail=epilogue', env=UNFUSED_ENV, seed=66)
CASES['unfused-l2-192-224-head224'] = _c('gcn', (16, 192, 224), (224, 224, 1), 'hubs',
    'unfused l1=k_agg<1,48,1> l2=k_agg<0,48,1>+k_dense<7,0>g1 head=k_dense<7,1>g1 tail=epilogue', env=UNFUSED_ENV, seed=13)
CASES['unfused-l2-224-128-head128'] = _c('sage', (16, 224, 128), (128, 128, 1), 'hubs',
    'unfused l1=k_agg<1,56,1> l2=k_agg<0,56,1>+k_dense<1,0>g4 head=k_dense<1,1>g4 tail=epilogue', env=UNFUSED_ENV, seed=64)
CASES['unfused-l2-256-256-head256'] = _c('gcn', (16, 256, 256), (256, 256, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x4 l2=k_agg<0,64,1>+k_dense<2,0>g4 head=k_dense<2,1>g4 tail=epilogue', env=UNFUSED_ENV)
# three layers with an output column, two relations, one mask row, and a headless plan (k_take_col
# after a conv layer's dense launch)
CASES['unfused-l3-col2'] = _c('sage', (16, 32, 64, 96), (96, 40, 4), 'hub130',
    'unfused l1=k_agg_l1_rows<32,1>x1 l2=k_agg<0,8,1>+k_dense<2,0>g1 l3=k_agg<0,16,1>+k_dense<3,0>g1 head=k_dense<2,1>g1 tail=epilogue', env=UNFUSED_ENV, out_col=2, seed=69)
CASES['unfused-rel2-l2'] = _c('sage', (16, 64, 64), (64, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,0>x1 l2=k_agg<0,16,1>+k_dense<2,1>g1 head=- tail=epilogue', env=UNFUSED_ENV, n_rel=2)
CASES['unfused-rows1'] = _c('gcn', (16, 64, 96), (96, 1), 'hubs',
    'unfused l1=k_agg_l1_rows<64,1>x1 l2=k_agg<0,16,1>+k_dense<3,1>g1 head=- tail=epilogue', env=UNFUSED_ENV, rows=1)
CASES['unfused-headless-take-col'] = _c('gcn', (16, 32, 3), (3,), 'hubs',
    'unfused l1=k_agg_l1_rows<32,1>x1 l2=k_agg<0,8,1>+k_dense<1,0>g1 head=- tail=k_take_col', env=UNFUSED_ENV, seed=12)


def relation_edges(n_rel, ei=None):
    """The graph's edges split over n_rel relations (edge i belongs to relation i % n_rel)."""
    ei = graph() if ei is None else ei
    et = np.arange(ei.shape[1]) % n_rel
    return et, [ei[:, et == r] for r in range(n_rel)]


def relation_names(n_rel):
    return [("n", "r%d" % r, "n") for r in range(n_rel)] if n_rel > 1 else None


def case(x):
    """A case by name, or the Case itself (a plan outside the table, e.g. FUSED_DECLINED)."""
    return CASES[x] if isinstance(x, str) else x


def model_key(name):
    """Cases that differ in query set, environment or row count share one model and one reference."""
    c = case(name)
    return (c.kind, c.dims, c.fc, c.n_rel, c.out_col, c.seed)


@functools.lru_cache(maxsize=None)
def _arch(key):
    from bikg_graph_explainability_public_amd.nn import ConvStack
    kind, dims, fc, n_rel, _, seed = key
    torch.manual_seed(seed)
    return ConvStack(kind, list(dims), list(fc), hetero_rels=relation_names(n_rel)).eval()


def arch(name):
    return _arch(model_key(name))


@functools.lru_cache(maxsize=None)
def _program(key):
    from bikg_graph_explainability_public_amd.program import compile_arch
    return compile_arch(_arch(key), relation_names(key[3]))


def program(name):
    return _program(model_key(name))


@functools.lru_cache(maxsize=None)
def _plan_arrays(queries, n_rel, n_layers):
    from bikg_graph_explainability_public_amd import engine
    _, parts = relation_edges(n_rel)
    return engine.plan_arrays(S, [np.ascontiguousarray(p) for p in parts], list(QUERIES[queries]), n_layers)


def plan_arrays(name):
    c = case(name)
    return _plan_arrays(c.queries, c.n_rel, len(c.dims) - 1)


@functools.lru_cache(maxsize=None)
def _all_outputs(key, dropped=None):
    """fp64 [ROWS, S]: the model at every node under every mask row (`dropped`: without the last
    in-edge of that hub)."""
    kind, dims, fc, n_rel, out_col, _ = key
    a = _arch(key)
    ei = graph() if dropped is None else hub_edge_dropped(dropped)
    x = features(dims[0]).numpy()
    rels = relation_names(n_rel)
    _, parts = relation_edges(n_rel, ei)
    if kind in ("gcn", "sage"):
        spec_a = {"kind": kind, "dims": list(dims), "fc": list(fc)}
        if rels:
            spec_a["hetero_rels"] = rels
        spec = oracle_spec({"arch_spec": spec_a},
                           {k: v.detach().cpu().numpy().copy() for k, v in a.state_dict().items()})
        if out_col:  # the oracle reads output column 0: hand it the picked row of the last head layer
            spec["fc"][-1]["W"] = spec["fc"][-1]["W"][out_col:out_col + 1]
            spec["fc"][-1]["b"] = spec["fc"][-1]["b"][out_col:out_col + 1]
        out = oracle.masked_all_outputs(spec, x, dict(zip(rels, parts)) if rels else {None: ei}, masks())
    else:
        import aggr_ref
        assert out_col == 0
        out = aggr_ref.union_outputs(a, x, parts, masks())
    out.setflags(write=False)
    return out


def reference(name):
    """fp64 [ROWS, n queries] in the plan's output order (the query set's order)."""
    return _all_outputs(model_key(name))[:, list(QUERIES[case(name).queries])]


def reference_hub_edge_dropped(name, hub):
    return _all_outputs(model_key(name), hub)[:, list(QUERIES[case(name).queries])]


def descriptor(name):
    """The case's plan descriptor, host only: sizes from the host-built receptive-field arrays,
    term kinds and widths from the compiled program (as engine.ForwardPlan fills them), every
    device pointer PTR or NULL as the plan has it set or unset."""
    from bikg_graph_explainability_public_amd import _lib
    c, prog, arr = case(name), program(name), plan_arrays(name)
    fr = arr["frontiers"]
    L = (_lib.LayerDesc * len(prog.convs))()
    prev = None
    for li, (ld, conv) in enumerate(zip(L, prog.convs)):
        raw = li == 0 and any(t.kind == "max" for t in conv.terms)
        if raw:
            prev = (conv.f_in + 31) // 32 * 32
        ld.n_terms, ld.act = len(conv.terms), 1
        ld.f_in_pad = prev if (li > 0 or raw) else 0
        ld.f_out, ld.f_out_pad = conv.f_out, (conv.f_out + 31) // 32 * 32
        ld.n_tgt, ld.n_edges = fr[li + 1].size, int(arr["layers"][li]["agg_src"].size)
        for f in ("tgt_prev", "tgt_f0", "agg_ptr", "agg_src", "agg_f0", "self_mult", "bias"):
            setattr(ld, f, PTR)
        ld.n_types = 1
        ld.weight = PTR if (li > 0 or raw) else None
        for k, t in enumerate(conv.terms):
            ld.terms[k].kind, ld.terms[k].rel, ld.terms[k].dst_type = _lib.TERM[t.kind], t.rel, t.dst_type
            ld.terms[k].table = PTR if li == 0 else None
        prev = ld.f_out_pad
    H = (_lib.HeadDesc * max(1, len(prog.head)))()
    for hd, h in zip(H, prog.head):
        n_real = h.weight.shape[0]
        hd.k_pad, hd.n_real, hd.n_pad, hd.act = prev, n_real, (n_real + 31) // 32 * 32, 2
        hd.weight, hd.bias = PTR, PTR
        prev = hd.n_pad
    desc = _lib.ForwardPlanDesc(cols=S, n_rel=c.n_rel, n0=fr[0].size, f0_node=PTR, deg_ptr=PTR, deg_src=PTR,
                                n_deg_edges=int(arr["deg_src"].size), n_layers=len(prog.convs), layers=L,
                                n_head=len(prog.head), head=H, out_col=c.out_col)
    desc._keep = (L, H)
    return desc


# ------------------------------------------------------------------ two plans outside the table
# An edge-mask plan (mask columns = the graph's edges, a link decoder on the query edge): its
# 32-wide layer 1 cannot take k_agg_l1_rows (lanes = mask rows of NODES) and runs the generic
# k_agg<1, 8, 1>.  The query edge is the 70-in-edge hub's last in-edge.
EDGE_MODEL = ("gcn", (16, 32, 32), (32, 8), 11)
EDGE_WANT = "unfused l1=k_agg<1,8,1> l2=k_agg<0,8,1>+k_dense<1,0>g1 head=k_dense<1,0>g1 tail=k_edge_dot"


@functools.lru_cache(maxsize=None)
def edge_model():
    from bikg_graph_explainability_public_amd.nn import ConvStack, LinkModel
    kind, dims, fc, seed = EDGE_MODEL
    torch.manual_seed(seed)
    return LinkModel(ConvStack(kind, list(dims), list(fc), final_act="identity").eval(), act="sigmoid").eval()


def edge_query():
    ei = graph()
    e = np.flatnonzero(ei[1] == HUB70)[-1]
    return int(ei[0, e]), int(ei[1, e])


@functools.lru_cache(maxsize=None)
def edge_masks():
    E = graph().shape[1]
    rng = np.random.default_rng(4)
    m = rng.random((ROWS, E)) < rng.uniform(0.2, 0.9, (ROWS, 1))
    m[0] = True
    m[1] = False
    m[2] = rng.random(E) < 0.03
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def edge_reference():
    """fp64 [ROWS]: the decoder's score of the query edge under every edge-mask row."""
    kind, dims, fc, _ = EDGE_MODEL
    sd = {k[len("encoder."):]: v.detach().cpu().numpy() for k, v in edge_model().state_dict().items()}
    spec = oracle_spec({"arch_spec": {"kind": kind, "dims": list(dims), "fc": list(fc)}}, sd)
    spec["fc"][-1]["act"] = None  # the encoder ends in Identity; the decoder applies the sigmoid
    u, v = edge_query()
    ref = oracle.masked_edge_outputs(spec, features(dims[0]).numpy(), graph(), edge_masks(), u, v)
    ref.setflags(write=False)
    return ref


def _layer_common(ld, n_tgt, n_edges):
    ld.n_tgt, ld.n_edges, ld.act = n_tgt, n_edges, 1
    for f in ("tgt_prev", "tgt_f0", "agg_ptr", "agg_src", "agg_f0", "self_mult", "bias"):
        setattr(ld, f, PTR)


def edge_descriptor():
    """The edge-mask plan's descriptor, host only (as pipeline.build_edge_plan / ForwardPlan fill it)."""
    from bikg_graph_explainability_public_amd import _lib, engine
    from bikg_graph_explainability_public_amd.program import compile_arch
    prog = compile_arch(edge_model())
    ei = np.ascontiguousarray(graph())
    E = ei.shape[1]
    arr = engine.plan_arrays(S, [ei], list(edge_query()), len(prog.convs), [np.arange(E, dtype=np.int64)])
    fr = arr["frontiers"]
    L = (_lib.LayerDesc * len(prog.convs))()
    prev = 0
    for li, (ld, conv) in enumerate(zip(L, prog.convs)):
        _layer_common(ld, fr[li + 1].size, int(arr["layers"][li]["agg_src"].size))
        ld.n_terms, ld.f_in_pad, ld.n_types = len(conv.terms), prev, 1
        ld.f_out, ld.f_out_pad = conv.f_out, (conv.f_out + 31) // 32 * 32
        ld.agg_eid = ld.self_ptr = ld.self_eid = PTR
        ld.weight = PTR if li else None
        for k, t in enumerate(conv.terms):
            ld.terms[k].kind, ld.terms[k].rel, ld.terms[k].dst_type = _lib.TERM[t.kind], t.rel, t.dst_type
            ld.terms[k].table = None if li else PTR
        prev = ld.f_out_pad
    H = (_lib.HeadDesc * max(1, len(prog.head)))()
    for hd, h in zip(H, prog.head):
        n_real = h.weight.shape[0]
        hd.k_pad, hd.n_real, hd.n_pad, hd.act = prev, n_real, (n_real + 31) // 32 * 32, 0
        hd.weight, hd.bias = PTR, PTR
        prev = hd.n_pad
    desc = _lib.ForwardPlanDesc(cols=E, n_rel=1, n0=fr[0].size, f0_node=PTR, deg_ptr=PTR, deg_src=PTR,
                                n_deg_edges=int(arr["deg_src"].size), n_layers=len(prog.convs), layers=L,
                                n_head=len(prog.head), head=H, out_col=0)
    desc.edge_masks, desc.deg_eid = 1, PTR
    desc.edge_dot, desc.dot_a, desc.dot_b, desc.dot_act = 1, 0, 1, 2
    desc._keep = (L, H)
    return desc


# A two-node-type plan (HeteroConv of SAGE relations between types A and B, the query a B node):
# every dense launch adds the bias row of its target's node type (the `t` mark of k_dense).
MT_RELS = [("A", "ab", "B"), ("B", "ba", "A"), ("A", "aa", "A")]
MT_SIZES, MT_DIMS, MT_HIDDEN, MT_LAYERS, MT_FC = {"A": 200, "B": 100}, {"A": 24, "B": 16}, 64, 2, [64, 16, 1]
MT_WANT = "unfused l1=k_agg_l1_rows<64,0>x1 l2=k_agg<0,16,1>+k_dense<2,0>g1t head=k_dense<1,1>g1 tail=epilogue"


@functools.lru_cache(maxsize=None)
def mt_setup():
    """(arch, golden_utils.multi_type_setup's dict): the 2-hop subgraph of B node 7."""
    from bikg_graph_explainability_public_amd.nn import HeteroSageStack
    from golden_utils import multi_type_setup
    g = torch.Generator().manual_seed(21)
    feat = {t: torch.randn(n, MT_DIMS[t], generator=g).numpy() for t, n in MT_SIZES.items()}
    ei = {r: torch.stack([torch.randint(0, MT_SIZES[r[0]], (m,), generator=g),
                          torch.randint(0, MT_SIZES[r[-1]], (m,), generator=g)]).numpy()
          for r, m in zip(MT_RELS, (500, 400, 500))}
    torch.manual_seed(3)
    arch = HeteroSageStack(MT_RELS, MT_DIMS, MT_HIDDEN, MT_LAYERS, MT_FC).eval()
    names = {t: [f"{t.lower()}{i}" for i in range(n)] for t, n in MT_SIZES.items()}
    c = multi_type_setup(feat, ei, names, "b7", "B", MT_LAYERS,
                         {k: v.numpy() for k, v in arch.state_dict().items()}, MT_FC)
    return arch, c


@functools.lru_cache(maxsize=None)
def mt_masks():
    n = mt_setup()[1]["x"].shape[0]
    rng = np.random.default_rng(6)
    m = rng.random((ROWS, n)) < rng.uniform(0.2, 0.9, (ROWS, 1))
    m[0] = True
    m[1] = False
    m[2] = rng.random(n) < 0.03
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def mt_reference():
    """fp64 [ROWS]: Model.predict_hetero_output per mask row (a copy that keeps no edge gives 0)."""
    c = mt_setup()[1]
    ref = oracle.hetero_multi_copy_outputs(c["spec"], c["x"], c["nt"], c["ei"], c["et"], c["ntypes"],
                                           c["rels"], c["pads"], mt_masks(), c["sub_ind"])
    ref.setflags(write=False)
    return ref


def mt_descriptor():
    """The two-node-type plan's descriptor, host only (as pipeline.build_plan / ForwardPlan fill it:
    the query mapped into its type's rows, other types' relation terms dropped from a layer whose
    targets share one type, tgt_type set on every layer)."""
    from bikg_graph_explainability_public_amd import _lib, engine
    from bikg_graph_explainability_public_amd.program import compile_arch
    arch, c = mt_setup()
    prog = compile_arch(arch, c["rels"], c["ntypes"])
    nt, et, ei = np.asarray(c["nt"]), np.asarray(c["et"]), np.asarray(c["ei"])
    q = int(np.flatnonzero(nt == prog.out_type)[c["sub_ind"]])
    rel_np = [np.ascontiguousarray(ei[:, et == r]) for r in range(len(c["rels"]))]
    arr = engine.plan_arrays(nt.size, rel_np, [q], len(prog.convs))
    fr = arr["frontiers"]
    L = (_lib.LayerDesc * len(prog.convs))()
    prev = 0
    for li, (ld, conv) in enumerate(zip(L, prog.convs)):
        terms = list(conv.terms)
        tt = np.unique(nt[fr[li + 1]])
        if tt.size == 1 and engine.PLAN_DROP_OTHER_TYPES:
            terms = [t for t in terms if t.dst_type < 0 or t.dst_type == int(tt[0])] or terms
        _layer_common(ld, fr[li + 1].size, int(arr["layers"][li]["agg_src"].size))
        ld.n_terms, ld.f_in_pad, ld.n_types = len(terms), prev, prog.n_types
        ld.f_out, ld.f_out_pad = conv.f_out, (conv.f_out + 31) // 32 * 32
        ld.tgt_type = PTR
        ld.weight = PTR if li else None
        for k, t in enumerate(terms):
            ld.terms[k].kind, ld.terms[k].rel, ld.terms[k].dst_type = _lib.TERM[t.kind], t.rel, t.dst_type
            ld.terms[k].table = None if li else PTR
        prev = ld.f_out_pad
    H = (_lib.HeadDesc * max(1, len(prog.head)))()
    for hd, h in zip(H, prog.head):
        n_real = h.weight.shape[0]
        hd.k_pad, hd.n_real, hd.n_pad, hd.act = prev, n_real, (n_real + 31) // 32 * 32, 2
        hd.weight, hd.bias = PTR, PTR
        prev = hd.n_pad
    desc = _lib.ForwardPlanDesc(cols=nt.size, n_rel=len(rel_np), n0=fr[0].size, f0_node=PTR, deg_ptr=PTR,
                                deg_src=PTR, n_deg_edges=int(arr["deg_src"].size), n_layers=len(prog.convs),
                                layers=L, n_head=len(prog.head), head=H, out_col=0)
    desc._keep = (L, H)
    return desc
