/*
 * xpgnn.h — C-ABI of the MI355X-native XP-GNN perturbation-scoring engine (libxpgnn.so).
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes + a HIP stream
 * (`xpg_stream_t`, NULL = legacy default stream) and returns an int status (XPG_OK = 0);
 * `xpg_last_error()` returns a thread-local message for the last failure.  No entry point
 * allocates device memory, frees or synchronises (the xpg_profile_* measurement hooks aside):
 * device memory (inputs, outputs, workspaces) is owned by the caller (PyTorch tensors in the
 * Python host), so every call can be captured in a hipGraph.  The one handle an entry point
 * creates: xpg_masked_forward's wide path (more than one 32-row pass, stream not capturing)
 * creates, once per device, a side stream and five events for its pass overlap.
 *
 * Mask bit layout ("row bits"): uint32 [rows][words], words = ceil(cols / 32); element c of
 * row r is bit (c & 31) of word r*words + (c >> 5).  Bits past `cols` in the last word are 0.
 *
 * Reference interfaces replaced (paths relative to /root/reference/src/pathway_explanations):
 *   xpg_pack_masks / xpg_unpack_masks  — bool mask batches handed between masks.py and
 *                                        wlm.py (DataLoader batches, masks.py:197-229)
 *   xpg_sample_shapley                 — Mask.shapley_mask           masks.py:231-260
 *   xpg_sample_shapley_dev             — same, device-resident seed (graph replays)
 *   xpg_sample_shapley_sets            — same, one draw per repeat in one call
 *   xpg_plan_arrays_build / _take      — ForwardPlan receptive-field arrays (host)
 *   xpg_sample_communities             — Mask.get_internal_mask / get_external_indices +
 *                                        Pathways.mask_generator (masks.py:81-194,
 *                                        pathways.py:234-385)
 *   xpg_edge_keep                      — Data.build_edge_mask        data.py:390-451
 *   xpg_rows_no_edge                   — the empty-copy test of the multi-node-type loop
 *                                        (a copy keeping no edge outputs 0)  model.py:213-215
 *   xpg_popcount_rows + xpg_shap_kernel— Kernel.compute             kernels.py:115-174
 *   xpg_masked_forward                 — Data.perturbator + Model.infer + extract_node_edge_output
 *                                        (wlm.py:349-436 -> data.py:591-648, model.py:62-116,
 *                                        model.py:295-328) for GCNConv / SAGEConv (mean, add, max) /
 *                                        GraphConv / GINConv / GATConv / HeteroConv-sum conv
 *                                        stacks and RGCNConv / FastRGCNConv stacks on typed
 *                                        edges (the 4-argument call of model.py:102-112) with a
 *                                        dense head; with edge_masks set, the
 *                                        edge problem's Data.perturb_edge (data.py:500-554: mask
 *                                        columns are edges) and a dot-product or DistMult link
 *                                        decoder (GCN / SAGE-mean terms, or RGCN REL terms, v27)
 *                                        (v27 addendum, no version change: xpg_layer_desc.pool
 *                                        appended; a conv stack followed by a global mean / add /
 *                                        max readout and a dense head, one output per mask row;
 *                                        XPG_TERM_ATT2 = 7: GATv2Conv layers, XPG_TERM_QKV = 8:
 *                                        TransformerConv layers, enum xpg_term below;
 *                                        xpg_masked_forward_w: the same with PyG's edge_weight of
 *                                        GCNConv / GraphConv, struct xpg_edge_weights below;
 *                                        xpg_masked_forward_e: the same with PyG's edge_attr of
 *                                        GINEConv, struct xpg_edge_feats below)
 *   xpg_pool_rows / _workspace / _describe — the readout alone (PyG global_mean_pool /
 *                                        global_add_pool / global_max_pool over one graph per row)
 *   xpg_forward_describe / xpg_wide_variants — none: host queries of xpg_masked_forward's own
 *                                        dispatch (path and wide-path kernels), for tests and logs
 *   xpg_forward_kernels / xpg_forward_variants — none: the same for the rows, fused and multi-kernel
 *                                        paths (instantiation and run-time form of every launch)
 *   xpg_sampler_describe               — none: host query of the device samplers' own dispatch (which
 *                                        k_shapley / k_shapley_flat / k_communities instantiation
 *                                        a shape launches, and its grid), for tests and logs
 *   xpg_wlm_describe / xpg_wlm_variants — none: host queries of xpg_wlm_fit's own dispatch (which
 *                                        k_wlm_fit / k_wlm_fit_mc instantiation or grid fit a
 *                                        shape launches, and the planner's split), for tests and logs
 *   xpg_dense                          — the dense feature x weight contraction inside each layer
 *                                        (PyG Linear / GCNConv.lin / SAGEConv.lin_l|lin_r)
 *   xpg_wlm_fit                        — train_model's epoch loop     wlm.py:132-278 with
 *                                        LinearRegression, regularizer, weighted_mse_loss and
 *                                        torch.optim.Adam(weight_decay=1e-2) (wlm.py:17-129,441-520)
 */
#ifndef XPGNN_H
#define XPGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XPG_ABI_VERSION 28
#define XPG_MAX_TERMS 8

typedef void* xpg_stream_t; /* hipStream_t */

enum xpg_status { XPG_OK = 0, XPG_EINVAL = 1, XPG_EHIP = 2, XPG_ENOSPC = 3 };

enum xpg_act { XPG_ACT_NONE = 0, XPG_ACT_RELU = 1, XPG_ACT_SIGMOID = 2, XPG_ACT_TANH = 3,
               XPG_ACT_LEAKY_RELU = 4, XPG_ACT_ELU = 5 };

/* aggregation term kinds of one conv layer (one term per relation, plus ROOT for SAGE) */
enum xpg_term { XPG_TERM_GCN = 0,   /* D^-1/2 (A_r + I) D^-1/2 over relation r               */
                XPG_TERM_MEAN = 1,  /* mean over kept in-edges of relation r (SAGE aggr)      */
                XPG_TERM_ROOT = 2,  /* the target's own row (SAGE lin_r)                     */
                XPG_TERM_ATT = 3,   /* graph attention over relation r (GATConv, v22; below)  */
                XPG_TERM_SUM = 4,   /* sum over kept in-edges of relation r (v25; below)      */
                XPG_TERM_MAX = 5,   /* element-wise max over kept in-edges (v25; below)       */
                XPG_TERM_REL = 6,   /* every relation's mean / sum, one term (RGCN, v26; below) */
                XPG_TERM_ATT2 = 7,  /* dynamic attention over relation r (GATv2Conv; v27 addendum, below) */
                XPG_TERM_QKV = 8    /* dot-product attention over relation r (TransformerConv; v27 addendum, below) */ };
/* ATT2 (v27 addendum: an enum value only; the version, every struct layout and the meaning of
 * every existing plan are unchanged).  One term = one GATv2Conv relation (PyG 2.0.4) and reuses
 * xpg_term_desc's fields: rel, heads, head_ch, neg_slope and self_loops mean what they mean for
 * ATT, and the edge set of target t in mask row b is exactly ATT's (xpg_term_desc below; the
 * loop's source row is XL[t]).  dst_type must be -1 and the layer's tgt_type NULL; node masks only.
 * With XL = lin_l(x), XR = lin_r(x) viewed as [.][heads][head_ch], edge e = (u -> t), head h:
 *   z_e^h = sum_c att[h][c] * leaky_relu(XL[u][h][c] + XR[t][h][c], neg_slope),
 *   m = max z, p_e = exp(z_e - m), alpha_e = p_e / (sum p + 1e-16), an empty edge set gives 0,
 * and the term adds sum_e alpha_e^h XL[u][h * head_ch + c] to column h * head_ch + c (the lin_l
 * bias travels inside the messages).  A layer's terms are all ATT2 or none and are summed; then
 * the layer's bias and act apply; columns past f_out are 0.  The layer is transform-then-aggregate
 * at every depth, so its `weight` is NULL and no dense launch follows it.
 * att_src, at every depth: device [f_out_pad], att[h][c] at h * head_ch + c, 0 past heads * head_ch.
 * Layer 1: table = XL [n0][f_out_pad] = X[F_0] W_l^T + b_l, att_dst = XR [n0][f_out_pad] (may alias
 * table: share_weights); padded columns 0; built once per plan (features are never masked).
 * Layer >= 2: table = device [2][f_out_pad][f_in_pad], W_l then W_r, zero-padded; coef = device
 * [2][f_out_pad], b_l then b_r (zeros without a bias); att_dst = NULL.  n_slices == 1 marks shared
 * weights: table / coef then hold the one block [1][f_out_pad][f_in_pad] / [1][f_out_pad] and XR is
 * XL (any other n_slices: the two blocks).  The forward transforms every previous-frontier row
 * of the call with xpg_dense's kernel into its workspace, then aggregates.
 * Refused before any launch (XPG_EINVAL, from xpg_masked_forward, xpg_forward_workspace and
 * xpg_forward_describe alike, without reading a device pointer): ATT2 mixed with another kind in a
 * layer, edge_masks, tgt_type or dst_type != -1, heads * head_ch > f_out_pad, a missing att_src /
 * table (att_dst at layer 1, coef at deeper layers), a non-NULL layer weight (at layer 1: the raw
 * form).  ATT2 plans run on the multi-kernel path only (xpg_forward_describe: `unfused`), launch no
 * degree pass unless another layer needs one, and need no score region. */
/* QKV (v27 addendum: an enum value only; the version, every struct layout and the meaning of every
 * existing plan are unchanged).  One term = one TransformerConv relation (PyG 2.0.4) and reuses
 * xpg_term_desc's fields.  heads and head_ch mean what they mean for ATT; dst_type must be -1 and
 * the layer's tgt_type NULL; node masks only.  self_loops = 0 and att_dst = NULL are unused.
 * Edge set of target t in mask row b: every CSR in-edge (u -> t) with bit(b, u) & bit(b, t),
 * duplicate edges as separate entries, plus the self_mult[r][t] copies of (t -> t) iff bit(b, t);
 * nothing is added or removed (a masked target has no edges).
 * n_slices = nb = 3 or 4 names the term's blocks, in the order K = lin_key(x), V = lin_value(x),
 * Q = lin_query(x) and, with root_weight (nb = 4), S = lin_skip(x), each viewed as
 * [.][heads][head_ch].  Edge e = (u -> t), head h:
 *   z_e^h = scale * sum_c Q[t][h][c] * K[u][h][c],
 *   m = max z, p_e = exp(z_e - m), alpha_e = p_e / (sum p + 1e-16), an empty edge set gives 0,
 *   out[h * head_ch + c] = sum_e alpha_e^h V[u][h][c].
 * scale = 1 / sqrt(head_ch), rounded once from fp64, travels in the term's neg_slope field (the
 * query row is multiplied by it before the products).
 * The term's epilogue, before the layer's terms are summed: nb = 3: out; nb = 4, att_src NULL:
 * out + S[t]; nb = 4 with att_src = device [2][f_out_pad] (g_out then g_r, zero-padded; with
 * lin_beta.weight = [w1 | w2 | w3] over [out, x_r, out - x_r], g_out = w1 + w3 and g_r = w2 - w3):
 * g = sigmoid(<g_out, out> + <g_r, S[t]>), g * S[t] + (1 - g) * out.  A layer's terms are all QKV
 * or none and are summed; then the layer's bias (a zero row for TransformerConv, which has no
 * bias of its own) and act apply; columns past f_out are 0.  The layer is transform-then-aggregate
 * at every depth, so its `weight` is NULL and no dense launch follows it.
 * Layer 1: table = device [n0][nb * f_out_pad], per F_0 node the nb blocks, block i =
 * X[F_0] W_i^T + b_i with padded columns 0; built once per plan (features are never masked).
 * Layer >= 2: table = device [nb][f_out_pad][f_in_pad], coef = device [nb][f_out_pad] (zeros
 * without a bias), both zero-padded.  The forward transforms every previous-frontier row of the
 * call with xpg_dense's kernel into its workspace ([rows * |F_{l-1}|][nb * f_out_pad] per term),
 * then aggregates.
 * Refused before any launch (XPG_EINVAL, from xpg_masked_forward, xpg_forward_workspace and
 * xpg_forward_describe alike, without reading a device pointer): QKV mixed with another kind in a
 * layer, edge_masks, tgt_type or dst_type != -1, heads <= 0 or heads * head_ch > f_out_pad,
 * n_slices not 3 or 4, a gate with n_slices == 3, a missing table (coef at deeper layers), a
 * non-NULL layer weight (at layer 1: the raw form), f_in_pad != the previous layer's f_out_pad.
 * xpg_masked_forward_w and xpg_masked_forward_e refuse QKV terms as they refuse ATT2.  QKV plans
 * run on the multi-kernel path only (xpg_forward_describe: `unfused`), launch no degree pass unless
 * another layer needs one, and need no score region. */
/* SUM and MAX (v25; node masks only: a plan with edge_masks set and one of them is refused).  The
 * edge set of target t in mask row b for relation r is MEAN's: every CSR in-edge (u -> t) with
 * bit(b, u) & bit(b, t), duplicate edges as separate entries, plus self_mult[r][t] copies of
 * (t -> t) iff bit(b, t).
 * SUM: the sum of the source rows over that edge set (MEAN's numerator: a self-loop of
 * multiplicity 2 adds the own row twice); an empty set gives 0.
 * MAX: the element-wise maximum over that edge set: duplicates are irrelevant, the own row takes
 * part iff self_mult > 0 and the target is kept; an empty set gives 0, not -inf (torch_scatter's
 * fill for empty segments), while a non-empty set of all-negative rows gives its negative maximum.
 * MAX is not linear, so a layer that holds a MAX term is aggregate-then-transform at every depth:
 * at layer 1 it needs the raw form (xpg_layer_desc.weight below).  SUM runs on the multi-kernel
 * and rows paths, MAX and raw layers on the multi-kernel path only; the fused and wide paths
 * take neither kind. */
/* REL (v26; RGCNConv / FastRGCNConv of PyG 2.0.4; no tgt_type; the node-mask rules first, the
 * edge-mask rules of v27 at the end): ONE term for all
 * n_rel relations (edge types) of the plan; its `rel` is ignored.  The edge set of target t in
 * mask row b for relation r is MEAN's (above): CSR in-edges (u -> t) with bit(b, u) & bit(b, t),
 * duplicates as separate entries, plus self_mult[r][t] copies of the own row iff bit(b, t): a
 * (t -> t) edge is an ordinary edge of its relation.  A_r = the sum of the source rows over that
 * set, divided by its size (norm = XPG_REL_MEAN; an empty set gives 0) or as it is (XPG_REL_SUM).
 * A masked-out target aggregates 0 and keeps its ROOT term (features are never masked).
 * A layer with a REL term holds exactly one, first, and at most one ROOT term after it; a plan
 * with a REL layer has one in every conv layer.  The kernel reads the mask bits itself (f0_node), so such a
 * plan launches no degree pass and its workspace has no degree region.  Per layer the plan
 * lists, for every target, the relations that have an in-edge or a self-loop, ascending
 * (xpg_layer_desc.seg_ptr / seg_rel): only those are visited.
 * Layer 1 (table form): `table` = [n_rel][n0][f_out_pad], relation r's pre-transformed F_0 rows
 * X[F_0] W_r (bases folded into W_r by the caller); n_slices = n_rel, coef = NULL; the term adds
 * sum_r A_r over the rows of table r.
 * Layer >= 2 (aggregate-then-transform): the term fills n_slices <= 32 slices of the layer's
 * dense input, slice s = A_s (coef = NULL, and then n_slices = n_rel) or sum_r coef[r][s] A_r
 * (coef = device [n_rel][n_slices], the basis coefficients: any n_rel); the ROOT term's slice
 * follows, and `weight` is [f_out_pad][(n_slices + ROOT terms) * f_in_pad].
 * REL plans run on the multi-kernel path only: the rows, fused and wide paths decline them.
 * REL under edge masks (v27; plan.edge_masks = 1, mask columns are the subgraph's edges): taken
 * when every conv layer carries agg_eid, self_ptr and self_eid (a plan that lacks one is refused
 * before any launch).  Nodes are never masked, so every target is "on".  In row b, relation r's
 * edge set at target t is: the CSR in-edges e of relation r with bit(b, agg_eid[e]) set,
 * duplicates as separate entries, plus one copy of the target's own row per kept self-loop edge of
 * type r, i.e. per column of self_eid[self_ptr[r][t] .. self_ptr[r][t + 1]) whose bit is set
 * (self_mult is not read).  XPG_REL_MEAN divides by the relation's kept count, by 1 when that is
 * 0; XPG_REL_SUM does not divide.  ROOT and bias are unchanged.  seg_ptr / seg_rel list the
 * relations with an in-edge or a self-loop in the unmasked subgraph.  Still no degree pass and no
 * degree region in the workspace; still the multi-kernel path only. */
enum xpg_rel_norm { XPG_REL_MEAN = 0, XPG_REL_SUM = 1 };
/* Graph-level readout (v27 addendum: xpg_layer_desc.pool, appended after seg_rel; the version and
 * every other layout are unchanged, and a zero-filled field means what every plan meant before).
 * `pool` may be non-zero on the LAST conv layer only.  After that layer's bias and activation the
 * n_tgt rows of each mask row reduce column-wise to one row of f_out_pad floats (padded columns
 * stay 0): a global mean / add / max pooling over the plan's last frontier (build it with every
 * node of the graph as a query for a graph-level model).  Node masks never remove a node: a
 * masked node loses its edges and keeps its own row (features are never masked), so every one of
 * the n_tgt targets takes part in every mask row.  MEAN is the SUM divided by (float)n_tgt (one
 * fp32 quotient); MAX has no empty case (n_tgt >= 1).  The reduction order is fixed and depends
 * on (n_tgt, f_out_pad) only, never on rows, a row's position in the launch or timing (no float
 * atomics): row shards and repeated calls agree bit for bit.  The head layers then run on `rows`
 * rows and y has `rows` values, y[r] = column out_col of row r.
 * xpg_masked_forward / xpg_forward_workspace / xpg_forward_describe fail with XPG_EINVAL before any
 * launch for: pool on a non-last layer, pool with edge_masks, pool with edge_dot, pool with
 * tgt_type, pool outside this enum.  The workspace of a pooled plan is that of the same plan
 * without pool plus, at its end, the pooled rows (rows * f_out_pad floats, rounded up to 256
 * bytes) and, when a row is split over several workgroups, the partial rows (xpg_pool_workspace
 * bytes, rounded up to 256).  Pooled plans run on the multi-kernel path only: the rows, fused and
 * wide paths decline them. */
enum xpg_pool { XPG_POOL_NONE = 0, XPG_POOL_MEAN = 1, XPG_POOL_SUM = 2, XPG_POOL_MAX = 3 };

int xpg_abi_version(void);
const char* xpg_last_error(void);

/* ---------------------------------------------------------------- masks */
int xpg_pack_masks(const uint8_t* mask, int64_t rows, int64_t cols, uint32_t* bits,
                   xpg_stream_t stream);
int xpg_unpack_masks(const uint32_t* bits, int64_t rows, int64_t cols, uint8_t* mask,
                     xpg_stream_t stream);
/* Shapley masks, P(bit) = 1/2, counter-based Philox4x32-10 keyed by (seed, global row). */
int xpg_sample_shapley(uint64_t seed, int64_t row_offset, int64_t rows, int64_t cols,
                       uint32_t* bits, xpg_stream_t stream);
/* Same rows with the seed read from device memory (*seed, uint64) when the kernel runs: a captured
 * HIP graph of the hot path draws new masks on every replay once the caller advances *seed on
 * the stream (v11). */
int xpg_sample_shapley_dev(const uint64_t* seed, int64_t row_offset, int64_t rows, int64_t cols,
                           uint32_t* bits, xpg_stream_t stream);
/* n_sets independent Shapley draws in one call: set k = xpg_sample_shapley(seeds[k], 0, rows, cols)
 * written at bits + k * rows * ceil(cols/32) (bits = [n_sets][rows][words]); seeds is a HOST array.
 * Explainer.run(times = n_sets) draws every repeat's masks this way (one host call, v18). */
int xpg_sample_shapley_sets(const uint64_t* seeds, int32_t n_sets, int64_t rows, int64_t cols,
                            uint32_t* bits, xpg_stream_t stream);
/* HOST function (no GPU work): the reference's compat Shapley draw torch.randint(0, 2, (rows, cols),
 * dtype=torch.bool) on torch's CPU generator (masks.py:231-260), replayed from the generator's
 * at::mt19937 state (state[624] words, left, next as torch.get_rng_state() stores them) and
 * written as bit-packed rows bits[rows][ceil(cols/32)] (host memory); the state is advanced past
 * the rows * cols outputs exactly as torch would (the caller writes it back with
 * torch.set_rng_state).  Bit-identical to the torch draw (v15). */
int xpg_mt19937_mask_bits(uint32_t* state, int32_t* left, int32_t* next, int64_t rows, int64_t cols,
                          uint32_t* bits);
/* HOST function (no GPU work): the per-repeat draws Explainer.run makes on torch's CPU generator
 * with the device Shapley sampler, in the reference's order (explainer.py:490-519): per repeat
 * the sampler seed torch.randint(0, 2**62, (1,)) -> seeds[t], the surrogate's initial weights
 * LinearRegression(S) = uniform_(from, to) on S floats (wlm.py:40-45) -> w0[t][S], and the
 * DataLoader iterator's base seed draw (value discarded).  State as in xpg_mt19937_mask_bits;
 * `fma` selects the fused x * (to - from) + from form of ATen's uniform_real (v20). */
int xpg_mt19937_repeat_draws(uint32_t* state, int32_t* left, int32_t* next, int32_t times, int64_t S,
                             float from, float to, int32_t fma, int64_t* seeds, float* w0);
/* HOST function (no GPU work): the reference's compat COMMUNITY draws (Mask.mask_generator with
 * communities, masks.py:299-348: per community in length-descending order get_internal_mask's
 * randint masks.py:130, Pathways.mask_generator's antithetic randint rows pathways.py:260-281,
 * activate_dead_mask's randperm pathways.py:318, pathway_mask2node_mask pathways.py:336-385 and
 * the member assignment masks.py:338) replayed from the at::mt19937 state as above, written
 * UNSHUFFLED as bit-packed rows bits[rows][ceil(cols/32)] (host memory); the caller applies the
 * row shuffle (torch.randperm, masks.py:385, on the returned state) or the S > 4000 truncation.
 * comm_ptr / comm_cols: CSR [n_comm + 1] / [nnz] of every community's member columns, ascending
 * (the reference sorts each community in place, masks.py:323); blocks: int32 [n_blocks][5] =
 * {row_start, size, size_internal, own community, b} back to back (Mask.community_plan), rows =
 * their total.  Bit-identical to the torch path, state advanced exactly as torch would (v16). */
int xpg_mt19937_community_bits(uint32_t* state, int32_t* left, int32_t* next, int64_t cols,
                               int32_t n_comm, const int32_t* comm_ptr, const int32_t* comm_cols,
                               const int32_t* blocks, int32_t n_blocks, int64_t rows, uint32_t* bits);
/* HOST functions (no GPU work): the receptive-field plan arrays of a forward plan
 * (engine.plan_arrays; the frontier walk of Model's L message-passing layers over the
 * computational subgraph, explainer.py:345-480 / model.py:62-116).  Edges relation by relation
 * (rel_ptr [n_rel + 1] offsets into src / dst [E]), optional per-edge mask columns eid [E]
 * (edge-mask plans; NULL = 0), the query positions [nq] (distinct, < S), L layers.  build
 * computes and keeps the arrays behind *handle and writes their sizes: the L + 1 frontier sizes,
 * then per CSR (the F_0 degree CSR, then layers 1..L) the sizes of {ptr, src, eid, smul, sptr,
 * seid}; take copies them back to back into out (int64, the sum of the sizes) and releases the
 * handle (free releases it without copying).  Frontier L = the queries, frontier l - 1 = frontier
 * l + its sorted new in-neighbours; CSRs group each target's in-edges (self-loops apart, counted
 * in smul with their columns in sptr / seid) in edge order, offsets absolute across relations;
 * the degree CSR holds source node ids, the layer CSRs source positions in F_0 (v19). */
int xpg_plan_arrays_build(int64_t S, int32_t n_rel, const int64_t* rel_ptr, const int64_t* src,
                          const int64_t* dst, const int64_t* eid, const int64_t* queries, int64_t nq,
                          int32_t L, void** handle, int64_t* sizes);
int xpg_plan_arrays_take(void* handle, int64_t* out);
int xpg_plan_arrays_free(void* handle);
/* Same bits, plus counts[r] = popcount of row r (the KernelSHAP coalition sizes, kernels.py:144),
 * accumulated while sampling so KernelSHAP needs no second pass over the bits. */
int xpg_sample_shapley_counts(uint64_t seed, int64_t row_offset, int64_t rows, int64_t cols,
                              uint32_t* bits, int32_t* counts, xpg_stream_t stream);
/* Community-aware masks — replaces Mask.get_internal_mask / get_external_indices and
 * Pathways.mask_generator / activate_dead_mask / pathway_mask2node_mask (masks.py:81-194,
 * pathways.py:234-385) plus the row shuffle (masks.py:375-380), generated in HBM.
 * blocks (device, int32 [n_blocks][5]) = {row_start, size, size_internal, own, off} per
 * community in length-descending order (the host plan, masks.py:309-340); col_ptr / col_comm
 * (device, int32 [cols+1] / [nnz]) = the communities each column belongs to.  Output row r is
 * source row perm(r) (shuffle != 0; a seeded bijection of [0, src_rows)) or r (shuffle == 0,
 * the S > 4000 truncation branch); prow (nullable) gets the row's community (pathway_rows). */
int xpg_sample_communities(uint64_t seed, int64_t rows, int64_t cols, int32_t n_comm,
                           const int32_t* blocks, int32_t n_blocks, int64_t src_rows,
                           int32_t shuffle, const int32_t* col_ptr, const int32_t* col_comm,
                           uint32_t* bits, int32_t* prow, xpg_stream_t stream);
/* the same rows' global range [row_offset, row_offset + rows) only, written to bits / prow from row 0
 * (row r of the full call == row r - row_offset here): a rank generates its own shard (ABI v14) */
int xpg_sample_communities_rows(uint64_t seed, int64_t row_offset, int64_t rows, int64_t cols,
                                int32_t n_comm, const int32_t* blocks, int32_t n_blocks,
                                int64_t src_rows, int32_t shuffle, const int32_t* col_ptr,
                                const int32_t* col_comm, uint32_t* bits, int32_t* prow,
                                xpg_stream_t stream);

/* The dispatch decision of the device samplers under the current environment, as text (v24).  A
 * HOST function: it launches nothing (the launchers and the query share one selection).
 * kind = XPG_SAMPLER_SHAPLEY: the kernel xpg_sample_shapley* (rows, cols) launches and its grid,
 * `k_shapley_flat<ALIGN> grid=NBx1` for rows of fewer than 64 quads (a quad = 4 mask words; cols
 * <= 8064) or `k_shapley<ALIGN> grid=GXxGY` (GX = ceil(quads / 256) blocks along a row, GY blocks
 * striding over the rows: 64 blocks per CU of the current device, 1 CU where none is visible, or
 * XPG_SHAPLEY_BLOCKS); ALIGN = 4 / 2 / 1 by words % 4 == 0 / words % 2 == 0 / else; n_comm and
 * n_blocks are ignored.  kind = XPG_SAMPLER_COMMUNITIES: the kernel xpg_sample_communities_rows
 * (rows, cols, n_comm, n_blocks) launches, `k_communities<SMALL,STAGED,CM> grid=NB lds=BYTES`
 * with SMALL = n_comm <= 64 (flags in a register, else an LDS bitset), STAGED = the columns'
 * communities staged in LDS (cols <= 16384 and they fit), CM = one column bitmask per community
 * in LDS (SMALL, cols <= 16384, masks + plan <= 48 KB, no XPG_COMM_PERCOL).  rows = 0: `none`.
 * XPG_SHAPLEY_BLOCKS / XPG_COMM_PERCOL count only with XPG_DIAGNOSTICS=1, as in the launchers
 * (XPG_EINVAL without it); XPG_ENOSPC when `n` bytes do not hold the text and its terminator. */
enum xpg_sampler { XPG_SAMPLER_SHAPLEY = 0, XPG_SAMPLER_COMMUNITIES = 1 };
int xpg_sampler_describe(int32_t kind, int64_t rows, int64_t cols, int32_t n_comm, int32_t n_blocks,
                         char* buf, size_t n);

/* ---------------------------------------------------------------- perturbation */
/* keep[b*n_edges + e] = bit(b, src[e]) & bit(b, dst[e])   (data.py:420-449) */
int xpg_edge_keep(const uint32_t* bits, int64_t rows, int64_t cols, const int32_t* src,
                  const int32_t* dst, int64_t n_edges, uint8_t* keep, xpg_stream_t stream);

/* empty[r] = 1 iff mask row r keeps no edge (src[e] and dst[e] both set), else 0: the multi-node-type
 * loop's copies without edges (model.py:213-215), one byte per row; stops at a row's first kept
 * edge.  (ABI v14) */
int xpg_rows_no_edge(const uint32_t* bits, int64_t rows, int64_t cols, const int32_t* src,
                     const int32_t* dst, int64_t n_edges, uint8_t* empty, xpg_stream_t stream);

/* ---------------------------------------------------------------- KernelSHAP */
int xpg_popcount_rows(const uint32_t* bits, int64_t rows, int64_t cols, int32_t* counts,
                      xpg_stream_t stream);
/* kernel_out[r] from counts[r] with M = cols-1: exact formula for M <= 1000, the reference's
 * ref-1000 approximation with its 0.9 back-off otherwise, then +-inf/NaN -> 0. */
int xpg_shap_kernel(const int32_t* counts, int64_t rows, int64_t cols, double* kernel_out,
                    xpg_stream_t stream);

/* ---------------------------------------------------------------- dense (MFMA fp32) */
/* C[m, n] = act(sum_k A[m, k] * W[n, k] + bias[n]) for n < n_real, 0 for n_real <= n < n_pad.
 * k_pad % 8 == 0 (A and W zero-padded in k), n_pad % 32 == 0 (<= 256), W has n_pad rows,
 * lda/ldw/ldc multiples of 4, pointers 16-byte aligned. */
int xpg_dense(const float* A, int64_t M, int64_t lda, const float* W, int64_t ldw,
              int64_t k_pad, const float* bias, int64_t n_real, int64_t n_pad, int act,
              float* C, int64_t ldc, xpg_stream_t stream);

/* ---------------------------------------------------------------- masked forward */
/* Frontier formulation: F_L ⊆ ... ⊆ F_1 ⊆ F_0 are the subgraph nodes whose layer outputs are
 * needed (the query's receptive field; or every node for a full-graph pass).  All CSR arrays
 * are device pointers; per-relation CSRs are concatenated (ptr arrays hold absolute offsets,
 * relation r's segment of a ptr array starts at r * (n + 1)). */
typedef struct xpg_term_desc {
  int32_t kind;            /* enum xpg_term                                             */
  int32_t rel;             /* relation index (degree slot); ignored for ROOT           */
  const float* table;      /* layer 1 only: pre-transformed F_0 rows [n0][f_out_pad]; a */
                           /* raw layer 1: the raw feature rows X[F_0] [n0][f_in_pad]   */
  int32_t dst_type;        /* multi-node-type plans: the term only reaches targets of   */
                           /* this node type (HeteroConv relation destination); -1 = all */
  /* XPG_TERM_ATT only (v22): one term = one GATConv relation (PyG 2.0.4 semantics) with `heads`
   * heads of `head_ch` channels, heads * head_ch = the conv's output width.
   * Edge set of target t in mask row b (node masks only): a non-self in-edge (u -> t) takes part
   * iff bit(b, u) & bit(b, t), duplicate edges as separate entries; self_loops = 0: the
   * self_mult copies of (t -> t) take part as ordinary edges iff bit(b, t); self_loops = 1
   * (add_self_loops): existing self-loops are dropped and exactly one (t -> t) edge takes part
   * whatever the mask.
   * Logit of edge e = (u -> t), head h: z = leaky_relu(a_s[u, h] + a_d[t, h], neg_slope);
   * softmax over the edge set: m = max z, p_e = exp(z_e - m), alpha_e = p_e / (sum p + 1e-16);
   * an empty edge set gives 0.
   * Layer 1: att_src / att_dst = [n0][heads] score tables a_s / a_d of the F_0 nodes (shared by
   * every mask row) and the term adds sum_e alpha_e table[u][h * head_ch + c] to column
   * h * head_ch + c.  Layer >= 2: att_src / att_dst = [heads][f_in_pad] vectors v_s / v_d with
   * a_s[u, h] = <v_s[h], row u of the layer input> (a_d likewise on the target's row), and the
   * term fills `heads` slices of the layer's dense input, slice h = sum_e alpha_e^h (row u);
   * the layer's `weight` then has one f_in_pad-wide column block per slice, in term order.
   * A layer's terms are all ATT or none; ATT plans run on the multi-kernel path only.       */
  int32_t heads, head_ch;
  float neg_slope;         /* leaky_relu slope of the logits (GATConv negative_slope)      */
  int32_t self_loops;      /* GATConv add_self_loops                                      */
  const float* att_src;
  const float* att_dst;
  /* XPG_TERM_REL only (v26; the rules are above) */
  int32_t n_slices;        /* slices of the dense input (layer >= 2); layer 1: n_rel        */
  int32_t norm;            /* enum xpg_rel_norm                                            */
  const float* coef;       /* device [n_rel][n_slices]; NULL = identity (n_slices == n_rel) */
} xpg_term_desc;

typedef struct xpg_layer_desc {
  int32_t n_terms;
  int32_t act;             /* activation after the conv (enum xpg_act)                 */
  int32_t f_in_pad;        /* width of this layer's input rows (layer >= 2), % 8 == 0;  */
                           /* layer 1: 0, or the raw form's feature width (below)       */
  int32_t f_out;           /* real output width                                        */
  int32_t f_out_pad;       /* padded output width, % 32 == 0, <= 256                   */
  int32_t n_tgt;           /* |F_l|                                                    */
  int32_t n_edges;         /* agg_src / agg_f0 length (all relations)                  */
  const int32_t* tgt_prev; /* [n_tgt] position of each target inside F_{l-1}          */
  const int32_t* tgt_f0;   /* [n_tgt] position of each target inside F_0; frontiers are */
                           /* prefix-ordered (F_l = the first |F_l| nodes of F_{l-1}),  */
                           /* so every target of every layer sits in F_0[0, |F_1|)      */
  const int32_t* agg_ptr;  /* [n_rel * (n_tgt + 1)] in-edges per target, self-loops out */
  const int32_t* agg_src;  /* source positions inside F_{l-1}                          */
  const int32_t* agg_f0;   /* source positions inside F_0                              */
  const int32_t* self_mult;/* [n_rel * n_tgt] multiplicity of (t, t) edges             */
  xpg_term_desc terms[XPG_MAX_TERMS];
  const float* weight;     /* layer >= 2: [f_out_pad][n_terms * f_in_pad] (ATT layers:   */
                           /* [f_out_pad][(sum of the terms' heads) * f_in_pad]; REL     */
                           /* layers: [f_out_pad][(n_slices + ROOT terms) * f_in_pad])   */
  /* Raw layer 1 (v25): layers[0].weight != NULL and layers[0].f_in_pad > 0 (the first conv's
   * input width rounded up to 32, at most 256) make layer 1 aggregate-then-transform like the
   * deeper layers: every term's `table` is the one pointer to the zero-padded raw feature rows
   * X[F_0] [n0][f_in_pad], shared by the terms and by all mask rows; the layer fills one f_in_pad-wide slice of a dense
   * input per term (ROOT: the own row; MEAN / SUM / MAX / GCN: the usual aggregate of raw rows)
   * and `weight` [f_out_pad][n_terms * f_in_pad] is applied with bias and activation.  Required
   * by a MAX term at layer 1; no ATT terms.  weight == NULL: the table form, unchanged.       */
  const float* bias;       /* [n_types][f_out_pad], summed over relations, zero-padded */
  const int32_t* tgt_type; /* multi-node-type plans: [n_tgt] node type of each target;   */
                           /* NULL for homogeneous / single-node-type graphs             */
  int32_t n_types;         /* rows of bias (1 when tgt_type is NULL)                   */
  /* edge-mask plans only (plan.edge_masks = 1; NULL otherwise):                          */
  const int32_t* agg_eid;  /* [n_edges] mask column (subgraph edge id) of each in-edge   */
  const int32_t* self_ptr; /* [n_rel * (n_tgt + 1)] self-loop edges of each target       */
  const int32_t* self_eid; /* their mask columns (MEAN terms count the kept ones)        */
  /* layers with a REL term only (v26; NULL otherwise):                                     */
  const int32_t* seg_ptr;  /* [n_tgt + 1] each target's range of seg_rel                 */
  const int32_t* seg_rel;  /* relations with an in-edge or self-loop at the target, ascending */
  /* graph-level readout (v27 addendum; the rules are at enum xpg_pool): 0 on every layer but the last */
  int32_t pool;            /* enum xpg_pool                                              */
} xpg_layer_desc;

typedef struct xpg_head_desc {
  int32_t k_pad, n_real, n_pad, act;
  const float* weight;     /* [n_pad][k_pad], zero-padded                              */
  const float* bias;       /* [n_pad], zero-padded                                     */
} xpg_head_desc;

typedef struct xpg_forward_plan {
  int64_t cols;            /* mask columns S                                           */
  int32_t n_rel;           /* relations (1 for homogeneous graphs)                     */
  int32_t n0;              /* |F_0|                                                    */
  const int32_t* f0_node;  /* [n0] subgraph node id of each F_0 position              */
  const int32_t* deg_ptr;  /* [n_rel * (n0 + 1)] in-edges of F_0 nodes, self-loops out */
  const int32_t* deg_src;  /* subgraph node ids                                        */
  int64_t n_deg_edges;     /* deg_src length (all relations)                           */
  int32_t n_layers;
  const xpg_layer_desc* layers;   /* host array [n_layers]                             */
  int32_t n_head;
  const xpg_head_desc* head;      /* host array [n_head]                               */
  int32_t out_col;         /* output column extracted (0)                              */
  /* Edge masks (Data.perturb_edge, data.py:500-554): mask columns are the subgraph's edges
   * (cols = edge count) and edge e is kept in row r iff its bit is set; every node stays
   * active.  Degrees and aggregations test the edge's own bit (deg_eid / agg_eid / self_eid);
   * GCN keeps one weight-1 self-loop per node whatever the mask (add_remaining_self_loops),
   * MEAN counts the kept self-loop edges.  Only the multi-kernel path takes these plans. */
  int32_t edge_masks;      /* 0: node masks (default), 1: edge masks                   */
  const int32_t* deg_eid;  /* [n_deg_edges] mask column of each deg_src entry          */
  /* Link decoder (edge problems): y[r] = act(<h_a, h_b>) over the n_real columns of the
   * last layer (head output, else last conv) of last-frontier targets a and b, instead of
   * one output column per target (then y has 1 column). */
  int32_t edge_dot;        /* 0: per-target outputs (default), 1: dot-product decoder   */
  int32_t dot_a, dot_b;    /* target positions in the last frontier                   */
  int32_t dot_act;         /* enum xpg_act applied to the dot product                  */
  /* v27, edge_dot only: NULL = the plain dot product above, unchanged.  Non-NULL: device [n_real]
   * per-column scale d (a DistMult decoder's relation embedding of the plan's query edge type,
   * fixed per plan): y[r] = act(sum_f (h_a[f] * d[f]) * h_b[f]), s = fmaf(h_a[f] * d[f], h_b[f], s)
   * in column order. */
  const float* dot_scale;
} xpg_forward_plan;

/* Workspace needed by xpg_masked_forward for `rows` mask rows. */
int xpg_forward_workspace(const xpg_forward_plan* plan, int64_t rows, size_t* bytes);
/* y[r * n_last + i] = model output (column out_col) of target i of the last conv layer for
 * mask row r (n_last = layers[n_layers-1].n_tgt; 1 for a single query); with edge_dot set,
 * y[r] = the decoded score of the target pair (dot_a, dot_b).  The workspace also holds the
 * launch's block-scheduling counters (zeroed on the stream before the kernel); its prior
 * contents never matter (no kernel reads a workspace byte it did not write).  Calls that may
 * run at the same time (different streams) need workspaces of their own.  Concurrent calls from
 * several host threads are safe under that rule: the wide path's shared side stream and pass
 * events are held by one call's whole enqueue sequence at a time. */
int xpg_masked_forward(const xpg_forward_plan* plan, const uint32_t* bits, int64_t rows,
                       float* y, void* workspace, size_t workspace_bytes, xpg_stream_t stream);
/* The dispatch decision of xpg_masked_forward(plan, rows) under the current environment, as text
 * (v23): the path, `wide`, `rows`, `fused` or `unfused`; for `wide` also the layer-1 and layer-2
 * kernels with their template arguments, e.g.
 * `wide l1=k_wide_l1s<2,0> l2=k_wide_last_ws<8,32,8,1,pipe>`.  A HOST function: it launches
 * nothing and touches no device (the launch and the query share one selection).  The plan's
 * pointers are tested for NULL only.  Fails like xpg_masked_forward where the decision itself
 * fails (XPG_FORWARD_STRICT=1 with a forced path that does not take the plan: XPG_EINVAL);
 * XPG_ENOSPC when `n` bytes do not hold the text and its terminator. */
int xpg_forward_describe(const xpg_forward_plan* plan, int64_t rows, char* buf, size_t n);
/* Every `l1=<kernel>` / `l2=<kernel>` token xpg_forward_describe can write for the wide path, one
 * per line (v23; the table the selection itself picks from). */
int xpg_wide_variants(char* buf, size_t n);

/* The readout of a pooled plan on its own (v27 addendum; rules at enum xpg_pool): h [rows][n][ld]
 * fp32 -> out [rows][ld], out[r][c] = mean / sum / max over i of h[r][i][c] (kind = enum xpg_pool,
 * not NONE).  ld % 4 == 0, 4 <= ld <= 256, n >= 1, h / out / workspace 16-byte aligned.  A row of
 * more nodes than one workgroup reduces is split into `parts` contiguous node ranges (parts
 * depends on n only): k_pool writes one partial row per part into the workspace
 * ([rows][parts][ld] floats, xpg_pool_workspace bytes; 0 when parts == 1) and k_pool_finish
 * combines them in ascending part order.  The workspace's prior contents never matter. */
int xpg_pool_workspace(int64_t rows, int64_t n, int64_t ld, size_t* bytes);
int xpg_pool_rows(const float* h, int64_t rows, int64_t n, int64_t ld, int32_t kind, float* out,
                  void* workspace, size_t workspace_bytes, xpg_stream_t stream);
/* The kernels xpg_pool_rows (and a pooled plan's readout) launches for a shape, as text, e.g.
 * `k_pool<sum> parts=1 part_nodes=512` or `k_pool<mean>+k_pool_finish<mean> parts=3 part_nodes=512`
 * (part_nodes = the node rows one workgroup reduces; parts = ceil(n / part_nodes)).  A HOST
 * function sharing the launcher's selection; XPG_ENOSPC when `nbytes` do not hold the text. */
int xpg_pool_describe(int64_t rows, int64_t n, int64_t ld, int32_t kind, char* buf, size_t nbytes);

/* Post-ops of conv layers (v27 addendum: new symbols only; the version, every struct above and the
 * three entry points above are unchanged, and a library without these symbols fails to load).
 * One record per conv layer, a HOST array [n_layers] handed beside the plan; an all-zero record
 * means the layer has no post-op, and post == NULL means no layer has one (then each _post entry
 * point is its namesake above, same results).  A layer with a post-op carries act = XPG_ACT_NONE
 * in its xpg_layer_desc; after its bias the post-op works in place on each of the layer's output
 * rows (one f_out_pad-wide fp32 row per (mask row, target)), in this order:
 *   1. v = h * scale + shift              (device [f_out_pad] each; NULL = 1 / 0)
 *   2. norm LAYER: mean and biased variance of v over the f_out real columns, two passes in fp32;
 *      v = (v - mean) / sqrt(var + eps) * gamma + beta   (device [f_out_pad]; NULL = 1 / 0)
 *   3. v = act(v)
 *   4. residual: v += the same mask row's input row of that target, row
 *      (r * n_prev + tgt_prev[t]) of the previous layer's output (after ITS post-op)
 *   5. columns f_out .. f_out_pad - 1 are written as exact 0, whatever they held.
 * A BatchNorm in eval mode that cannot be folded into the layer's weights (attention layers) is
 * the affine of step 1; a LayerNorm over the last dimension is step 2.  The sums are reduced in a
 * fixed order that depends on (f_out, f_out_pad) alone: row shards and repeated calls agree bit
 * for bit.  Host checks, XPG_EINVAL before any launch: a post layer whose xpg_layer_desc.act is
 * not NONE; norm outside enum xpg_norm; LAYER with eps not finite or <= 0; gamma / beta without
 * LAYER; residual on layer 1, with f_out_pad unequal to the previous layer's, or without tgt_prev;
 * an edge_masks or edge_dot plan; n_types > 1 / tgt_type.  A plan with any post-op runs on the
 * multi-kernel path only (a forced rows / fused / wide path under XPG_FORWARD_STRICT=1 is
 * refused); when its last conv layer has a post-op, neither the out-column pick nor the first head
 * layer is fused into that layer's dense epilogue; a pooled plan's readout follows the post-op.
 * xpg_forward_describe_post writes `unfused` followed by ` post<l>=k_post<NORM,RES>` for each post
 * layer l (1-based), e.g. `unfused post2=k_post<layer,1>`.  The workspace is that of the same plan
 * without post-ops on the multi-kernel path. */
enum xpg_norm { XPG_NORM_NONE = 0, XPG_NORM_LAYER = 1 };
typedef struct xpg_post_desc {
  int32_t norm;            /* enum xpg_norm                                              */
  float eps;               /* LAYER: added to the variance                               */
  const float* scale;      /* before the norm                                            */
  const float* shift;
  const float* gamma;      /* after the norm (LAYER only)                                */
  const float* beta;
  int32_t act;             /* enum xpg_act                                               */
  int32_t residual;        /* 0 / 1                                                      */
} xpg_post_desc;
int xpg_forward_workspace_post(const xpg_forward_plan* plan, const xpg_post_desc* post, int64_t rows,
                               size_t* bytes);
int xpg_masked_forward_post(const xpg_forward_plan* plan, const xpg_post_desc* post, const uint32_t* bits,
                            int64_t rows, float* y, void* workspace, size_t workspace_bytes,
                            xpg_stream_t stream);
int xpg_forward_describe_post(const xpg_forward_plan* plan, const xpg_post_desc* post, int64_t rows,
                              char* buf, size_t n);
/* One post-op on its own: in place on h [M][ld] fp32 (ld % 4 == 0, 4 <= ld <= 256, 1 <= f_out <= ld,
 * h and the record's arrays ([ld] each) 16-byte aligned).  With post->residual: M = rows * n_tgt,
 * hprev [rows][n_prev][ld_prev] (ld_prev >= ld, % 4 == 0, 16-byte aligned), tgt_prev device
 * [n_tgt] with values < n_prev; otherwise hprev / ld_prev / n_tgt / n_prev / tgt_prev are not read.
 * An item is one row on a power-of-two group of >= ld / 4 lanes of one wave (one float4 chunk per
 * lane), so a wave works on 64 / group rows at once. */
int xpg_post_rows(float* h, int64_t M, int64_t ld, int64_t f_out, const xpg_post_desc* post,
                  const float* hprev, int64_t ld_prev, int64_t n_tgt, int64_t n_prev,
                  const int32_t* tgt_prev, xpg_stream_t stream);
/* The kernel xpg_post_rows launches for a shape, as text: `k_post<layer,1> group=8 rows_per_wave=8`.
 * A HOST function sharing the launcher's selection; XPG_ENOSPC when `nbytes` do not hold the text. */
int xpg_post_describe(int64_t M, int64_t ld, int64_t f_out, const xpg_post_desc* post, char* buf,
                      size_t nbytes);

/* Edge weights (v27 addendum: new symbols only; the version, every struct above and every entry
 * point above are unchanged).  One finite float per edge of the graph (PyG 2.0.4's `edge_weight` of
 * GCNConv and GraphConv), handed beside the plan already gathered into the plan's CSR orders, all
 * device arrays.  weights == NULL: each _w entry point is its _post namesake, same results (the
 * _post entry points are that case of the same code).  Node masks as ever: in mask row b an edge
 * (u -> t) of weight w_e survives iff bit(b, u) & bit(b, t); a self-loop is an edge like any other.
 *   GCN term (gcn_norm with add_remaining_self_loops(fill_value = 1); weights >= 0):
 *     lw[v]  = loop_w[v] when v is kept, else 1   (loop_w: the weight of v's LAST self-loop in edge
 *              order, 1 for a node without one)
 *     deg[v] = lw[v] + sum of w_e over v's kept non-loop in-edges, fp32, in CSR order
 *     dis[v] = deg[v] > 0 ? 1 / sqrt(deg[v]) : 0
 *     out[t] = dis[t]^2 lw[t] x[t] + sum over kept (u -> t) of dis[u] w_e dis[t] x[u]
 *   SUM term: self_sum[t] x[t] + sum over kept in-edges of w_e x[u] (nothing for a masked-out t).
 *   MEAN term: that sum divided by the COUNT of kept in-edges, self_mult[t] included, at least 1.
 *   MAX term: the element-wise maximum of w_e x[u] over the kept in-edges and, with self_mult[t] > 0,
 *     of the self-loops, folded per element as x[t] >= 0 ? self_wmax[t] x[t] : self_wmin[t] x[t];
 *     an empty set gives 0.  Any finite weight, negative ones included, for SUM / MEAN / MAX.
 *   ROOT terms, the table / raw forms of layer 1, post-ops, the pooled readout and the head are
 *   unchanged (they run around the aggregation).
 * k_degree_w writes the in-edge counts as k_degree does (-1 for a masked-out node) and, for plans
 * with a GCN term, the weighted degrees (1 for a masked-out node); k_agg_w<L1, LPS, NV> is k_agg's
 * item / lane mapping with the per-edge weight loaded beside each in-edge.
 * Host checks, XPG_EINVAL before any launch: edge_masks or edge_dot; n_rel > 1; tgt_type
 * (multi-node-type plans); a term kind other than GCN / MEAN / ROOT / SUM / MAX; a missing array
 * (layers, agg_w, self_sum, self_wmax, self_wmin; deg_w and loop_w with a GCN term).  A weighted
 * plan runs on the multi-kernel path only (a forced rows / fused / wide path under
 * XPG_FORWARD_STRICT=1 is refused).  xpg_forward_describe_w writes
 * `unfused weights=k_degree_w+k_agg_w`, then the ` post<l>=...` tokens.  The workspace is that of
 * the same plan without weights on the multi-kernel path plus, at its end and only with a GCN
 * term, the weighted degrees (rows * n0 floats, rounded up to 256 bytes). */
typedef struct xpg_layer_weights {
  const float* agg_w;      /* [n_edges] weight of in-edge e (the index of agg_src / agg_f0)   */
  const float* self_sum;   /* [n_rel * n_tgt] sum of the weights of the target's self-loops  */
  const float* self_wmax;  /* [n_rel * n_tgt] their maximum (unread where self_mult == 0)    */
  const float* self_wmin;  /* [n_rel * n_tgt] their minimum                                  */
} xpg_layer_weights;
typedef struct xpg_edge_weights {
  const float* deg_w;      /* [n_deg_edges] weight of each deg_src entry (GCN terms)         */
  const float* loop_w;     /* [n_rel * n0] last self-loop weight of each F_0 node, else 1    */
  const xpg_layer_weights* layers; /* host array [n_layers]                                  */
} xpg_edge_weights;
int xpg_forward_workspace_w(const xpg_forward_plan* plan, const xpg_post_desc* post,
                            const xpg_edge_weights* weights, int64_t rows, size_t* bytes);
int xpg_masked_forward_w(const xpg_forward_plan* plan, const xpg_post_desc* post,
                         const xpg_edge_weights* weights, const uint32_t* bits, int64_t rows, float* y,
                         void* workspace, size_t workspace_bytes, xpg_stream_t stream);
int xpg_forward_describe_w(const xpg_forward_plan* plan, const xpg_post_desc* post,
                           const xpg_edge_weights* weights, int64_t rows, char* buf, size_t n);

/* Edge features (v27 addendum: new symbols only; the version, every struct above and every entry
 * point above are unchanged).  One finite float row per edge of the graph (PyG 2.0.4's `edge_attr`
 * of GINEConv), already mapped to each conv layer's input width (E_l = lin_l(edge_attr), or the
 * rows themselves) and gathered into the plan's CSR orders, all device arrays of f_in_pad floats
 * per row with zero padded columns.  feats == NULL: each _e entry point is its _w namesake, same
 * results (the _w entry points are that case of the same code).  Node masks as ever: in mask row b
 * an edge (j -> t) survives iff bit(b, j) & bit(b, t); no self-loop is added, and a self-loop or a
 * duplicate edge is a message of its own with its own row.
 *   SUM term:  out[t] = sum over t's self-loops k of relu(x[t] + self_e[k])
 *                     + sum over kept in-edges e = (j -> t), in CSR order, of relu(x[j] + agg_e[e])
 *              for a kept t, 0 for a masked-out one.  ROOT terms (which carry GINEConv's (1 + eps)
 *              fold), post-ops, the pooled readout and the head are unchanged.
 * Every layer runs in the aggregate-then-transform form (layer 1: the raw form, weight and
 * f_in_pad set, every term's table the one X[F_0] table).  A SUM layer's descriptor must set
 * self_ptr (agg_eid / self_eid are not read): self_e's row k belongs to entry k of the self-loop
 * CSR, agg_e's row e to entry e of agg_src / agg_f0.  Layer 1 may also give msg_rows
 * [n_edges + n_self][f_in_pad]: relu(x[j] + agg_e[e]) per in-edge, then relu(x[t] + self_e[k]) per
 * self-loop, formed in fp32 (its sources are feature rows shared by every mask row); the kernel
 * then loads that one row per edge and adds the same values (XPG_EFEAT_MSG=0: ignored, for
 * diagnostics).  k_agg_e<MSG, LPS, NV> is k_agg_w's item / lane mapping.
 * Host checks, XPG_EINVAL before any launch: weights given as well; edge_masks or edge_dot;
 * n_rel > 1; tgt_type; a term kind other than SUM / ROOT; a layer in the table form; a missing
 * array (layers; self_ptr, agg_e, self_e of a layer with a SUM term; a ROOT-only layer's record is
 * not read); msg_rows past layer 1.  An edge-featured plan runs on the multi-kernel path only (a
 * forced rows / fused / wide path under XPG_FORWARD_STRICT=1 is refused).
 * xpg_forward_describe_e writes `unfused efeat=k_agg_e`, then the ` post<l>=...` tokens.  The
 * workspace is that of the same plan without features on the multi-kernel path. */
typedef struct xpg_layer_efeat {
  const float* agg_e;     /* [n_edges][f_in_pad] edge row of in-edge e (the index of agg_f0)     */
  const float* self_e;    /* [n_self][f_in_pad] edge row of self-loop k (the index of self_eid)  */
  const float* msg_rows;  /* layer 1, optional: [n_edges + n_self][f_in_pad] whole messages      */
} xpg_layer_efeat;
typedef struct xpg_edge_feats {
  const xpg_layer_efeat* layers; /* host array [n_layers]                                       */
} xpg_edge_feats;
int xpg_forward_workspace_e(const xpg_forward_plan* plan, const xpg_post_desc* post,
                            const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                            int64_t rows, size_t* bytes);
int xpg_masked_forward_e(const xpg_forward_plan* plan, const xpg_post_desc* post,
                         const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                         const uint32_t* bits, int64_t rows, float* y, void* workspace,
                         size_t workspace_bytes, xpg_stream_t stream);
int xpg_forward_describe_e(const xpg_forward_plan* plan, const xpg_post_desc* post,
                           const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                           int64_t rows, char* buf, size_t n);

/* Class readout (v27 addendum: new symbols only; the version, every struct above and every entry
 * point above are unchanged).  z[m][0..C) is the network's last linear output of output row m =
 * (mask row, target), a query node or the one pooled row; C = the last head layer's n_real, or the
 * last conv layer's f_out of a headless plan.  Output column c of row m:
 *   NONE:        z[m][c]   (what out_col means; element-wise activations already applied)
 *   SOFTMAX:     exp(z_c - max_j z_j) / sum_j exp(z_j - max_j z_j)   over the C real columns only
 *   LOG_SOFTMAX: (z_c - max_j z_j) - log sum_j exp(z_j - max_j z_j)
 * Padded columns never take part, whatever they hold; C = 1 gives exactly 1.0f / 0.0f.
 * k_class_out<KIND, ALL>: one row on a power-of-two lane group of one wave (k_post's mapping, one
 * float4 chunk per lane); the maximum and the sum each cross the group by one xor butterfly, so a
 * row's result depends on its values and (C, ld) alone, never on M or on its position in the launch.
 * cls == NULL: each _c entry point is its _e namesake, same results (the _e entry points are that
 * case of the same code).  With cls, plan->out_col is ignored and y holds rows * n_last values
 * (col >= 0) or rows * n_last * C values (col == -1: [rows][n_last][C]); {NONE, c} gives bitwise
 * the output of the plain entry with out_col = c where that entry's tail is the column pick
 * (k_take_col: the same rows, the same element); where the plain entry computes the column in
 * k_dense's HEAD epilogue, or takes the rows / fused / wide path, the two differ by float32 rounding.
 * Host checks, XPG_EINVAL before any launch: kind outside the enum; col outside [-1, C);
 * edge_masks or edge_dot; tgt_type; SOFTMAX / LOG_SOFTMAX over a last head layer (or headless
 * last conv layer, its post-op included) that carries an element-wise activation.  A plan with cls
 * runs on the multi-kernel path only (a forced rows / fused / wide path under XPG_FORWARD_STRICT=1
 * is refused) with the unfused tail: neither the column pick nor the last head layer goes into a
 * k_dense epilogue, and k_class_out is launched where k_take_col was.  Post-ops, the pooled
 * readout, weights and edge features compose unchanged.  xpg_forward_describe_c appends
 * ` class=k_class_out<kind,one|all>`, e.g. `unfused class=k_class_out<softmax,all>`.  The
 * workspace is that of the same plan on the multi-kernel path. */
enum xpg_class_kind { XPG_CLASS_NONE = 0, XPG_CLASS_SOFTMAX = 1, XPG_CLASS_LOG_SOFTMAX = 2 };
typedef struct xpg_class_out {
  int32_t kind;            /* enum xpg_class_kind                                         */
  int32_t col;             /* >= 0: that class; -1: all C classes                         */
} xpg_class_out;
int xpg_forward_workspace_c(const xpg_forward_plan* plan, const xpg_post_desc* post,
                            const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                            const xpg_class_out* cls, int64_t rows, size_t* bytes);
int xpg_masked_forward_c(const xpg_forward_plan* plan, const xpg_post_desc* post,
                         const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                         const xpg_class_out* cls, const uint32_t* bits, int64_t rows, float* y,
                         void* workspace, size_t workspace_bytes, xpg_stream_t stream);
int xpg_forward_describe_c(const xpg_forward_plan* plan, const xpg_post_desc* post,
                           const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                           const xpg_class_out* cls, int64_t rows, char* buf, size_t n);
/* The readout on its own: in [M][ld] fp32 (ld % 4 == 0, 4 <= ld <= 256, 16-byte aligned,
 * 1 <= n_real <= ld) -> out [M] (col >= 0) or [M][n_real] (col == -1). */
int xpg_class_out_rows(const float* in, int64_t M, int64_t ld, int64_t n_real, int32_t kind,
                       int32_t col, float* out, xpg_stream_t stream);

/* The kernels behind xpg_forward_describe's `rows`, `fused` and `unfused` (v28 addendum: new symbols
 * only; the version, every struct above and every entry point above are unchanged).  HOST functions:
 * they launch nothing and touch no device; the launches dispatch on the same pick records
 * (rows_pick, fused_pick, layer_pick, agg_pick, dense_pick, tail_pick) these texts are printed from.
 * xpg_forward_kernels writes what xpg_masked_forward would launch for the plan, row count and
 * environment, one of
 *   `rows k_rows_forward<4,0> layers=2 bits=lds w2=global head=lds,global`
 *        k_rows_forward<FS, SUMK> (FS = f1_pad / 16 features per wave, SUMK = a SUM term) and its
 *        run-time forms: mask rows staged in LDS or read from global memory, layer 2's weights
 *        (`-`: one layer), each head layer's weights (`-`: no head layer)
 *   `fused k_fused_forward<4> layers=3 tpp=8,4`
 *        k_fused_forward<waves per block>; targets per pass of each layer past the first
 *   `unfused l1=k_agg_l1_rows<64,1>x2 l2=k_agg<0,24,1>+k_dense<3,0>g1 head=k_dense<1,1>g1 tail=epilogue`
 *        per conv layer its aggregation kernel, k_agg_l1_rows<features per wave, ONE> x feature
 *        slices or k_agg<L1, LPS, NV>, `+` its dense launch k_dense<NT, HEAD> g column groups (`t`:
 *        per-type bias rows); then the head layers' dense launches (`-`: none) and the tail:
 *        `epilogue` (the output column computed in the k_dense<NT,1> launch named before it),
 *        `k_take_col`, `k_edge_dot`, `k_edge_dot_scaled` or the class readout's kernel.  Weighted
 *        and edge-featured layers read `k_agg_w` / `k_agg_e`, attention and relation layers
 *        `att` / `att2` / `qkv` / `rel` (their own tests name those kernels), followed by `+` and
 *        the layer's dense launch where it has one (`att` / `rel` layers past the first).
 *   `wide l1=... l2=...`  as xpg_forward_describe.
 * Fails where xpg_forward_describe fails.  xpg_forward_variants lists every instantiation of
 * k_rows_forward, k_fused_forward, k_agg_l1_rows, k_agg and k_dense in the library, one per line. */
int xpg_forward_kernels(const xpg_forward_plan* plan, int64_t rows, char* buf, size_t n);
int xpg_forward_kernels_c(const xpg_forward_plan* plan, const xpg_post_desc* post,
                          const xpg_edge_weights* weights, const xpg_edge_feats* feats,
                          const xpg_class_out* cls, int64_t rows, char* buf, size_t n);
int xpg_forward_variants(char* buf, size_t n);

/* Optional per-kernel timing of xpg_masked_forward's wide (full-graph) path (v13): with profiling
 * on, every launch of a profiled kernel is bracketed by two hipEvents on its stream;
 * xpg_profile_read waits for them and returns, per slot, the summed device milliseconds and the
 * launch count, then releases them.  xpg_profile_enable (0 / 1) also drops unread records.  For
 * measurement only: never enable it around a graph capture.  Slots: */
enum xpg_prof_slot { XPG_PROF_WIDE_BITS = 0, XPG_PROF_WIDE_F0 = 1, XPG_PROF_WIDE_DEGREE = 2,
                     XPG_PROF_WIDE_L1 = 3, XPG_PROF_WIDE_L2 = 4, XPG_PROF_SLOTS = 5 };
int xpg_profile_enable(int on);
int xpg_profile_read(double* ms, int64_t* launches, int32_t n_slots);

/* ---------------------------------------------------------------- weighted linear surrogate */
typedef struct xpg_wlm_params {
  float lr, l1_lambda, beta1, beta2, eps, weight_decay;
} xpg_wlm_params;

/* Workspace needed by xpg_wlm_fit. */
int xpg_wlm_workspace(int64_t n_fits, int64_t rows, int64_t cols, int64_t batch, size_t* bytes);
/* Which fit kernel a shape takes (v13): *kind = XPG_WLM_SINGLE (one workgroup per fit),
 * XPG_WLM_MULTI (*parts co-resident workgroups per fit), XPG_WLM_GRID (the many-column
 * streaming fit, three launches per Adam step) or XPG_WLM_GRID_FUSED (v21: the many-column fit
 * as one persistent launch per fit, *parts co-resident workgroups, one per CU; the grid kinds
 * have no xpg_wlm_prepare / xpg_wlm_fit_prepared); *parts = 1 unless MULTI / GRID_FUSED.  The
 * choice depends on the current device's CU count and the XPG_WLM / XPG_MC_* overrides
 * (XPG_WLM=grid3: the three-launch grid fit). */
enum xpg_wlm_kind { XPG_WLM_SINGLE = 0, XPG_WLM_MULTI = 1, XPG_WLM_GRID = 2, XPG_WLM_GRID_FUSED = 3 };
int xpg_wlm_plan(int64_t n_fits, int64_t rows, int64_t cols, int64_t batch, int32_t* kind,
                 int32_t* parts);
/* The fit kernel xpg_wlm_fit / xpg_wlm_fit_from launch for a shape on the current device under
 * the current XPG_WLM setting, as text (v28): the variant and the planner's split, one of
 *   `single<CPT=2,stage> n_bs=3 n_ds=1`   k_wlm_fit<CPT, STAGE> (`stage` / `nostage`), batch and
 *                                         column slices per wave item
 *   `multi<C=1,G=1> P=13 wpp=3 ds=1`      k_wlm_fit_mc<C, G>, parts per fit, mask words per part,
 *                                         column-row slices per lane
 *   `grid3 n_wg=9`                        the three-launch grid fit, column chunks
 *   `grid_fused ch=1 nwg=9 nrbp=8`        k_gw_fused: chunks per workgroup, workgroups, padded
 *                                         32-row blocks
 * A HOST function: it launches nothing.  The launch dispatches on the same variant record this
 * text is printed from.  Fails where the fit's layout fails; XPG_ENOSPC when `n` bytes do not
 * hold the text and its terminator. */
int xpg_wlm_describe(int64_t n_fits, int64_t rows, int64_t cols, int64_t batch, char* buf, size_t n);
/* Every variant name (the text before the first space) xpg_wlm_describe can write, one per line
 * (v28): ten `single<...>`, nine `multi<...>`, `grid3`, `grid_fused`. */
int xpg_wlm_variants(char* buf, size_t n);
/* Runs ceil(rows / batch) Adam steps of train_model over consecutive row batches for n_fits
 * independent surrogates (e.g. the `times` repeats of Explainer.run), one workgroup each.
 * Arrays are fit-major and contiguous: bits [n_fits][rows][words], y / kernel [n_fits][rows],
 * w / adam_m / adam_v [n_fits][cols] (updated in place), losses [n_fits][steps] (fp64),
 * best_epoch [n_fits] (first argmin).  `step0` = Adam steps already taken with (m, v).
 * status (device int32 [1], nullable, zeroed by the caller): sticky — the call ORs a nonzero
 * error word into it when the multi-workgroup fit's cross-workgroup exchange timed out (a
 * partner workgroup was not co-resident) and never clears it (v13), so one word checked after
 * many fits (e.g. K replays of a captured chain) reports a failure in any of them; every
 * output of a failed call is invalid and the caller must not use it. */
int xpg_wlm_fit(int64_t n_fits, const uint32_t* bits, int64_t rows, int64_t cols,
                int64_t batch, const float* y, const double* kernel,
                const xpg_wlm_params* params, int64_t step0, float* w, float* adam_m,
                float* adam_v, double* losses, int32_t* best_epoch, int32_t* status,
                void* workspace, size_t workspace_bytes, xpg_stream_t stream);
/* Same fit started from initial weights w0 [n_fits][cols] with zero Adam moments (step0 = 0):
 * w = w0, adam_m = adam_v = 0 are written by the fit's own prologue kernel, so a fresh fit
 * needs no copy / fill launches of its own (v11). */
int xpg_wlm_fit_from(int64_t n_fits, const uint32_t* bits, int64_t rows, int64_t cols,
                     int64_t batch, const float* y, const double* kernel,
                     const xpg_wlm_params* params, const float* w0, float* w, float* adam_m,
                     float* adam_v, double* losses, int32_t* best_epoch, int32_t* status,
                     void* workspace, size_t workspace_bytes, xpg_stream_t stream);
/* xpg_wlm_fit_from in two launches on one workspace (v12): xpg_wlm_prepare runs the fit's
 * prologue (per-step constants from y / kernel, column bit vectors, w = w0, zero moments,
 * exchange-slot reset) and xpg_wlm_fit_prepared the Adam steps + losses / best epoch / status.
 * Same results bit for bit; a caller with two workspaces can prepare the next fit while the
 * current one runs.  Shapes that take the many-column grid fit have no prologue: EINVAL. */
int xpg_wlm_prepare(int64_t n_fits, const uint32_t* bits, int64_t rows, int64_t cols,
                    int64_t batch, const float* y, const double* kernel,
                    const xpg_wlm_params* params, const float* w0, float* w, float* adam_m,
                    float* adam_v, void* workspace, size_t workspace_bytes, xpg_stream_t stream);
int xpg_wlm_fit_prepared(int64_t n_fits, const uint32_t* bits, int64_t rows, int64_t cols,
                         int64_t batch, const double* kernel, const xpg_wlm_params* params,
                         float* w, float* adam_m, float* adam_v, double* losses,
                         int32_t* best_epoch, int32_t* status, void* workspace,
                         size_t workspace_bytes, xpg_stream_t stream);

/* xpg_wlm_fit_prepared in its two launches (v17): the Adam steps (the fit kernel: w, adam_m,
 * adam_v) and then, in stream order after them, the losses / first best epoch / status word
 * (k_wlm_loss_best).  A caller that needs the next fit to start right after this one's steps can
 * put the losses on another stream (after an event on the steps' stream). */
int xpg_wlm_fit_steps(int64_t n_fits, const uint32_t* bits, int64_t rows, int64_t cols, int64_t batch,
                      const double* kernel, const xpg_wlm_params* params, float* w, float* adam_m,
                      float* adam_v, void* workspace, size_t workspace_bytes, xpg_stream_t stream);
int xpg_wlm_fit_losses(int64_t n_fits, int64_t rows, int64_t cols, int64_t batch, const double* kernel,
                       const xpg_wlm_params* params, double* losses, int32_t* best_epoch,
                       int32_t* status, void* workspace, size_t workspace_bytes, xpg_stream_t stream);

/* ---------------------------------------------------------------- k-hop computational subgraph */
/* Replaces Data.comp_graph's PyG k_hop_subgraph(seed, hops, edge_index, relabel_nodes=True,
 * flow='source_to_target') call (reference data.py:331-333).  Workspace for a graph of
 * n_nodes nodes and n_edges edges. */
int xpg_khop_workspace(int64_t n_nodes, int64_t n_edges, size_t* bytes);
/* edge_index: int64 [2][n_edges] (row 0 = source, row 1 = target).  Outputs (device):
 * subset [n_nodes capacity] sorted node ids; sub_src / sub_dst [n_edges capacity] relabelled
 * kept edges in original order; edge_mask [n_edges] (0/1 bytes); counts [4] =
 * {|subset|, kept edges, position of seed in subset, 1 if any edge id was out of range}.
 * Asynchronous: the caller reads counts after synchronising the stream. */
int xpg_khop_subgraph(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int64_t seed,
                      int32_t hops, int64_t* subset, int64_t* sub_src, int64_t* sub_dst,
                      uint8_t* edge_mask, int64_t* counts, void* workspace,
                      size_t workspace_bytes, xpg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* XPGNN_H */
