"""The device mask samplers and the row popcount, bit for bit against NumPy.

Reference: oracle/sampler_oracle.py, a per-row / per-column restatement of the samplers' Philox
counter layout (validated on its own in tests/test_samplers_cpu.py: Random123 known answers and
the community rule's structure).  Every comparison here is exact; the one tolerance is the
suite's KernelSHAP rtol 1e-10 (device lgamma binomial vs scipy).  Every case first asserts,
through xpg_sampler_describe, the kernel instantiation it was chosen to run: the column counts
come from the launchers' own conditions (fewer than 64 quads of 4 words -> k_shapley_flat, ALIGN
by words % 4 / % 2, a second blockIdx.x past 1024 words; n_comm <= 64, 16384 staged columns, 48
KB of column masks for k_communities)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from bikg_graph_explainability_public_amd import _lib
from sampler_checks import check_dead_rows, community_case, unpack

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SH, CO = 0, 1
ROWS = 37
SEEDS = (7, 2 ** 64 - 5)
OFFSETS = (0, 2 ** 33 + 7)
# cols -> the kernel xpg_sample_shapley* must launch (words, quads; tail = cols % 32)
SHAPLEY = {1: "k_shapley_flat<1>",       # 1 word, tail 1
           33: "k_shapley_flat<2>",      # 2 words, tail 1
           96: "k_shapley_flat<1>",      # 3 words, no tail
           100: "k_shapley_flat<4>",     # 4 words, tail 4
           128: "k_shapley_flat<4>",     # 4 words, no tail
           1193: "k_shapley_flat<2>",    # 38 words, tail 9
           8064: "k_shapley_flat<4>",    # 252 words = 63 quads: the last flat size
           8065: "k_shapley<1>",         # 253 words = 64 quads, tail 1
           8100: "k_shapley<2>",         # 254 words, tail 4
           8190: "k_shapley<4>",         # 256 words, tail 30
           8192: "k_shapley<4>",         # 256 words, no tail
           32790: "k_shapley<1>",        # 1025 words = 257 quads: gridDim.x = 2, tail 22
           32800: "k_shapley<1>"}        # 1025 words, no tail (32800 = 1025 x 32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.load()


def _eng():
    from bikg_graph_explainability_public_amd import engine
    return engine


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(seed, row_offset, rows, cols):
    """(bits, popcounts) of the oracle, computed once per case and read-only."""
    bits = oracle.shapley_bits(seed, row_offset, rows, cols)
    cnt = oracle.popcount_rows(bits)
    bits.setflags(write=False)
    cnt.setflags(write=False)
    return bits, cnt


def _shapley_grid(rows, cols):
    """The launch grid the launcher documents: flat = one lane per (row, quad); else
    ceil(quads / 256) blocks along a row x blocks striding over rows, 64 per CU in all."""
    quads = ((cols + 31) // 32 + 3) // 4
    if quads < 64:
        return f"{-(-rows * quads // 256)}x1"
    gx = -(-quads // 256)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return f"{gx}x{max(1, min(rows, 64 * cus // gx))}"


def _assert_shapley_variant(rows, cols, grid=None):
    assert _eng().sampler_describe(SH, rows, cols) == f"{SHAPLEY[cols]} grid={grid or _shapley_grid(rows, cols)}"


def _dev_seed(seed):
    return torch.full((1,), seed - 2 ** 64 if seed >= 2 ** 63 else seed, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------ Shapley sampler
@pytest.mark.parametrize("row_offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cols", list(SHAPLEY))
def test_shapley_bits_and_counts_equal_oracle(cols, seed, row_offset):
    """Host seed, device seed and the fused-popcount entry point write the oracle's rows; the
    fused counts are the oracle's row popcounts (global rows past 2^33, a seed with its high
    half set)."""
    e = _eng()
    _assert_shapley_variant(ROWS, cols)
    ref, ref_cnt = _ref(seed, row_offset, ROWS, cols)
    got = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=row_offset)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(_u32(got), ref)
    dev = e.sample_shapley_dev(_dev_seed(seed), ROWS, cols, row_offset=row_offset)
    np.testing.assert_array_equal(_u32(dev), ref)
    bits, cnt = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=row_offset, with_counts=True)
    assert torch.equal(bits, got)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref_cnt)


@pytest.mark.parametrize("cols", [1193, 8100, 32800])
def test_shapley_sets_equal_oracle(cols):
    e = _eng()
    _assert_shapley_variant(ROWS, cols)
    sets = e.sample_shapley_sets(list(SEEDS), ROWS, cols, DEV)
    np.testing.assert_array_equal(_u32(sets), np.stack([_ref(s, 0, ROWS, cols)[0] for s in SEEDS]))


@pytest.mark.parametrize("blocks_y", [3, -1])
@pytest.mark.parametrize("cols", [8100, 32800])
def test_shapley_row_stride_loop(cols, blocks_y, monkeypatch):
    """k_shapley's blocks stride over the rows: 3 row-blocks walk 37 rows in 13 uneven trips (the
    last one short), -1 = one row per block; bits and counts equal the default launch's and the
    oracle's either way."""
    e = _eng()
    seed, off = SEEDS[1], OFFSETS[1]
    base_bits, base_cnt = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=off, with_counts=True)
    gx = 2 if cols > 32768 else 1
    monkeypatch.setenv("XPG_DIAGNOSTICS", "1")
    monkeypatch.setenv("XPG_SHAPLEY_BLOCKS", str(blocks_y * gx if blocks_y > 0 else -1))
    _assert_shapley_variant(ROWS, cols, grid=f"{gx}x{blocks_y if blocks_y > 0 else ROWS}")
    bits, cnt = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=off, with_counts=True)
    plain = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=off)
    ref, ref_cnt = _ref(seed, off, ROWS, cols)
    np.testing.assert_array_equal(_u32(bits), ref)
    np.testing.assert_array_equal(_u32(plain), ref)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref_cnt)
    assert torch.equal(bits, base_bits) and torch.equal(cnt, base_cnt)


@pytest.mark.parametrize("cols", [1193, 8100])
def test_shapley_counts_do_not_depend_on_the_buffer(cols):
    """The counts are accumulated with atomics, so the call zeroes them first: drawn right after
    tensors of the counts' size were filled with a pattern and freed (the caching allocator hands
    such a block back), and through the C entry point onto a caller's filled tensor."""
    e = _eng()
    _assert_shapley_variant(ROWS, cols)
    ref, ref_cnt = _ref(SEEDS[0], 0, ROWS, cols)
    dirty = [torch.full((ROWS,), 0x7f7f7f7f, dtype=torch.int32, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    del dirty
    bits, cnt = e.sample_shapley(SEEDS[0], ROWS, cols, DEV, with_counts=True)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref_cnt)
    np.testing.assert_array_equal(_u32(bits), ref)
    filled = torch.full((ROWS,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    _lib.call("xpg_sample_shapley_counts", ctypes.c_uint64(SEEDS[0]), 0, ROWS, cols, _lib.ptr(bits),
              _lib.ptr(filled), _lib.stream_of(DEV))
    np.testing.assert_array_equal(filled.cpu().numpy(), ref_cnt)


@pytest.mark.parametrize("cols", [1193, 8100])
def test_shapley_shards_concatenate_to_the_single_draw(cols):
    """Rows [0, a), [a, b), [b, R) drawn with row_offset, bits and counts concatenated, are the
    single draw's (the multi-rank benchmark step draws its masks this way)."""
    e = _eng()
    seed, base = SEEDS[1], OFFSETS[1]
    full_bits, full_cnt = e.sample_shapley(seed, ROWS, cols, DEV, row_offset=base, with_counts=True)
    parts = [e.sample_shapley(seed, b - a, cols, DEV, row_offset=base + a, with_counts=True)
             for a, b in ((0, 5), (5, 23), (23, ROWS))]
    assert torch.equal(torch.cat([p[0] for p in parts]), full_bits)
    assert torch.equal(torch.cat([p[1] for p in parts]), full_cnt)
    ref, ref_cnt = _ref(seed, base, ROWS, cols)
    np.testing.assert_array_equal(_u32(full_bits), ref)
    np.testing.assert_array_equal(full_cnt.cpu().numpy(), ref_cnt)


# ------------------------------------------------------------------ k_popcount
@pytest.mark.parametrize("words", [1, 63, 64, 65, 255, 256, 257, 449, 625, 1025])
def test_popcount_rows_at_loop_boundaries(words):
    """k_popcount (one wave per row, 4 rows per block; lanes stride the words with 4 loads in
    flight while w + 192 < words, then one by one) against NumPy at the loop boundaries: rows of
    mixed density, a row set only in its last word, one set only in word 192."""
    e = _eng()
    cols = words * 32 - 3
    rng = np.random.default_rng(words)
    for rows in (1, 4, 5, 259):   # 259: 64 full blocks and one of 3 rows
        dens = rng.choice([0.0, 0.03, 0.5, 0.97, 1.0], size=(rows, 1))
        m = rng.random((rows, cols)) < dens
        m[0] = False
        m[0, (words - 1) * 32:] = True
        if rows > 1 and words > 192:
            m[1] = False
            m[1, 192 * 32:193 * 32] = True
        bits = torch.from_numpy(oracle.pack_bits(m).view(np.int32)).to(DEV)
        assert bits.shape == (rows, words)
        scratch = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
        e.shap_kernel(bits, cols, scratch=scratch)
        np.testing.assert_array_equal(scratch.cpu().numpy(), m.sum(1))


# ------------------------------------------------------------------ KernelSHAP from counts
@pytest.mark.parametrize("cols", [200, 1001, 1002, 8100])
def test_shap_kernel_from_fused_counts(cols):
    """shap_kernel(counts=) on the sampler's fused counts (the timed benchmark step) is bitwise
    shap_kernel's own popcount pass, and both are the oracle's KernelSHAP of the unpacked rows."""
    e = _eng()
    rows = 64
    bits, cnt = e.sample_shapley(11, rows, cols, DEV, with_counts=True)
    m = unpack(_ref(11, 0, rows, cols)[0], cols)
    np.testing.assert_array_equal(_u32(bits), _ref(11, 0, rows, cols)[0])
    k_cnt = e.shap_kernel(bits, cols, counts=cnt)
    k_own = e.shap_kernel(bits, cols)
    assert torch.equal(k_cnt, k_own)
    ref = oracle.shap_kernel(m)
    np.testing.assert_allclose(k_cnt.cpu().numpy(), ref, rtol=1e-10, atol=0)
    np.testing.assert_array_equal(k_cnt.cpu().numpy() == 0, ref == 0)
    if cols == 1001:
        # Why the exact branch (M = cols - 1 <= 1000) is the one that shows a wrong count: its
        # value M / (C(M + 1, k) (M + 1 - k) k) moves by the factor (M - k) / k when k grows by
        # one — a relative step of at least 1 / k unless 2 k = M — far above rtol 1e-10.
        k = m.sum(1)
        m1 = m.copy()
        for r in range(rows):
            m1[r, np.flatnonzero(~m[r])[0]] = True   # one more bit per row
        step = np.abs(oracle.shap_kernel(m1) / ref - 1)
        assert (step[k != 500] >= 1.0 / k[k != 500] - 1e-12).all() and (k != 500).sum() > rows // 2


# ------------------------------------------------------------------ community sampler
# name -> (S, community lengths, interpret_samples, members shared by two communities, the
# k_communities<SMALL,STAGED,CM> the case must launch)
COMMUNITY = {
    "cm": (300, [40, 7, 2, 1, 25, 60, 3], 100, 12, "k_communities<1,1,1>"),
    "cm_94_words": (3000, [1000, 700, 33, 300, 5], 100, 12, "k_communities<1,1,1>"),
    # 64 communities x 250 words x 4 B > 48 KB: no column masks
    "small_staged": (8000, [900, 700] + [100] * 20 + [20] * 42, 60, 30, "k_communities<1,1,0>"),
    "small_unstaged": (16400, [5000, 3000, 40, 7], 60, 9, "k_communities<1,0,0>"),
    "lds_staged": (4000, [300, 200] + [20] * 40 + [7] * 23, 100, 20, "k_communities<0,1,0>"),
    "lds_unstaged": (16400, [3000, 2000] + [20] * 40 + [7] * 23, 60, 20, "k_communities<0,0,0>"),
}


@pytest.mark.parametrize("name", list(COMMUNITY))
def test_community_bits_equal_oracle(name):
    """Bits and pathway rows of every k_communities variant against the per-row oracle:
    unshuffled and shuffled, two seeds (one with its high half set), the whole repeat and a
    row_offset / rows shard; overlapping members; community counts 4, 5, 7, 65 (no multiple of
    32) and 64."""
    e = _eng()
    S, lens, samples, overlap, variant = COMMUNITY[name]
    pathways, (blocks, src_rows, _, _) = community_case(S, lens, samples, overlap=overlap)
    assert e.sampler_describe(CO, src_rows, S, len(pathways), blocks.shape[0]).split()[0] == variant
    for seed in (5, 2 ** 63 + 11):
        for shuffle in (False, True):
            plan = (blocks, src_rows, src_rows, shuffle)
            bits, prow = e.sample_communities(seed, plan, pathways, S, DEV)
            rb, rp = oracle.community_bits(seed, blocks.numpy(), src_rows, shuffle, pathways, S)
            np.testing.assert_array_equal(_u32(bits), rb)
            np.testing.assert_array_equal(prow.cpu().numpy(), rp)
    # a shard of the last draw (shuffled, the second seed): the same rows of the oracle's repeat
    a, n = src_rows // 3, src_rows // 2
    assert e.sampler_describe(CO, n, S, len(pathways), blocks.shape[0]).split()[0] == variant
    sb, sp = e.sample_communities(seed, plan, pathways, S, DEV, row_offset=a, rows=n)
    np.testing.assert_array_equal(_u32(sb), rb[a:a + n])
    np.testing.assert_array_equal(sp.cpu().numpy(), rp[a:a + n])


def test_community_flags_past_2048_communities():
    """2100 communities of one or two columns (and one big one, for antithetic pairs): the flag
    words of communities 2048.. come from the flag loop's second 64-word trip."""
    e = _eng()
    S, lens = 4000, [1200] + [2] * 700 + [1] * 1399
    pathways, (blocks, src_rows, _, _) = community_case(S, lens, 100)
    assert len(pathways) == 2100 and blocks.shape[0] == 2100
    assert e.sampler_describe(CO, src_rows, S, 2100, 2100).split()[0] == "k_communities<0,1,0>"
    bits, prow = e.sample_communities(5, (blocks, src_rows, src_rows, False), pathways, S, DEV)
    rb, rp = oracle.community_bits(5, blocks.numpy(), src_rows, False, pathways, S)
    np.testing.assert_array_equal(_u32(bits), rb)
    np.testing.assert_array_equal(prow.cpu().numpy(), rp)
    hi = np.concatenate([pathways[c] for c in range(2048, 2100)])
    assert unpack(rb, S)[:, hi].any(0).all()        # the last flag words are exercised
    a, n = src_rows - 500, 400                       # shuffled shard, the other seed
    sb, sp = e.sample_communities(2 ** 63 + 11, (blocks, src_rows, src_rows, True), pathways, S, DEV,
                                  row_offset=a, rows=n)
    rb, rp = oracle.community_bits(2 ** 63 + 11, blocks.numpy(), src_rows, True, pathways, S,
                                   row_offset=a, rows=n)
    np.testing.assert_array_equal(_u32(sb), rb)
    np.testing.assert_array_equal(sp.cpu().numpy(), rp)


@pytest.mark.parametrize("percol", ["0", "1"])
def test_community_dead_rows_equal_oracle(percol, monkeypatch):
    """The 3-community / 5-column case over 64 seeds: every lone external row with no flag on
    switches the oracle's pick on (both the column-mask and the per-column kernel)."""
    e = _eng()
    from bikg_graph_explainability_public_amd.masks import Mask
    pathways = [[0, 1, 2], [2, 3], [4]]
    m = Mask(torch.zeros((5, 1)), torch.zeros((2, 0), dtype=torch.long), pathways,
             {"interpret_samples": 2, "epochs": 1}, "node_prediction")
    blocks, src_rows, rows, _ = m.community_plan()
    monkeypatch.setenv("XPG_DIAGNOSTICS", "1")
    monkeypatch.setenv("XPG_COMM_PERCOL", percol)
    want = "k_communities<1,1,1>" if percol == "0" else "k_communities<1,1,0>"
    assert e.sampler_describe(CO, src_rows, 5, 3, 3).split()[0] == want
    picked = set()

    def rows_of_seed(seed):
        bits, prow = e.sample_communities(seed, (blocks, src_rows, src_rows, False), pathways, 5, DEV)
        rb, rp = oracle.community_bits(seed, blocks.numpy(), src_rows, False, pathways, 5)
        np.testing.assert_array_equal(_u32(bits), rb)
        np.testing.assert_array_equal(prow.cpu().numpy(), rp)
        picked.add(rb.tobytes())
        return unpack(rb, 5)

    check_dead_rows(rows_of_seed, pathways, blocks)
    assert len(picked) > 32
