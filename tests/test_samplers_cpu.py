"""The device samplers' NumPy oracle (oracle/sampler_oracle.py) and their dispatch query
(xpg_sampler_describe) on a machine without a GPU.  The oracle is checked on its own here — the
Philox known-answer vectors, the properties a counter-based draw must have, and the community
rule's structure on the oracle's own rows — so that tests/test_gpu_samplers.py compares the
kernels with something validated independently of them.  The dispatch strings are the ones that
file asserts before it compares bits."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import sampler_oracle as so
from sampler_checks import (check_community_shuffle, check_community_structure, check_dead_rows,
                            community_case, unpack)

ENV = ("XPG_DIAGNOSTICS", "XPG_SHAPLEY_BLOCKS", "XPG_COMM_PERCOL")
SH, CO = 0, 1


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _describe(*a, **k):
    from bikg_graph_explainability_public_amd import engine
    return engine.sampler_describe(*a, **k)


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, want):
    """Random123's published philox4x32-10 vectors (kat_vectors), scalar and vectorised."""
    got = oracle.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(v) for v in got) == want
    vec = oracle.philox4x32_10([np.array([c, 5, c]) for c in ctr], key)
    assert all(v.dtype == np.uint32 and v.shape == (3,) for v in vec)
    assert " ".join("%08x" % int(v[2]) for v in vec) == want


# ------------------------------------------------------------------ Shapley rows
def test_shapley_bits_properties():
    S, R = 1193, 64
    a = oracle.shapley_bits(7, 0, R, S)
    assert a.dtype == np.uint32 and a.shape == (R, 38)
    np.testing.assert_array_equal(oracle.shapley_bits(7, 40, 9, S), a[40:49])  # row_offset
    big = 2 ** 33 + 7
    np.testing.assert_array_equal(oracle.shapley_bits(7, big + 3, 5, S),
                                  oracle.shapley_bits(7, big, 8, S)[3:])
    assert not (a[:, -1] >> np.uint32(S % 32)).any()                          # clean tail word
    for cols in (1, 31, 33, 95):
        b = oracle.shapley_bits(7, 0, 4, cols)
        assert b.shape == (4, (cols + 31) // 32) and not (b[:, -1] >> np.uint32(cols % 32)).any()
    # the first words of a row do not depend on its length (quad q -> words 4q .. 4q + 3)
    np.testing.assert_array_equal(oracle.shapley_bits(7, 0, 4, 96), oracle.shapley_bits(7, 0, 4, 4096)[:, :3])
    # the counter holds all 64 bits of the global row, the key all 64 bits of the seed
    hi = oracle.shapley_bits(7, 2 ** 32, R, S)
    assert not (hi == a).all(1).any()
    assert not (oracle.shapley_bits(7 + 2 ** 32, 0, R, S) == a).all(1).any()
    assert not (oracle.shapley_bits(8, 0, R, S) == a).all(1).any()
    # fair bits (64 x 1193 draws: 0.5 +- 5 sigma = 0.0091)
    assert abs(unpack(a, S).mean() - 0.5) < 0.0091
    np.testing.assert_array_equal(oracle.popcount_rows(a), unpack(a, S).sum(1))


# ------------------------------------------------------------------ community rows
@pytest.mark.parametrize("S, lens, samples", [(300, [40, 7, 2, 1, 25, 60, 3], 100),
                                              (4000, [20] * 100 + [7] * 50, 500)])
def test_community_bits_structure(S, lens, samples):
    """The oracle's own rows pass the structural assertions test_community_sampler_structure
    makes of the kernel's (one case with a single flag word, one with five)."""
    pathways, (blocks, src_rows, rows, _) = community_case(S, lens, samples)
    bits, prow = oracle.community_bits(5, blocks, src_rows, False, pathways, S)
    assert bits.dtype == np.uint32 and bits.shape == (src_rows, (S + 31) // 32)
    check_community_structure(bits, prow, S, pathways, blocks)
    sb, sp = oracle.community_bits(5, blocks, src_rows, True, pathways, S)
    check_community_shuffle(sb, sp, bits, prow)
    sb3, _ = oracle.community_bits(6, blocks, src_rows, True, pathways, S)
    assert not np.array_equal(sb, sb3)
    a_, b_ = rows // 3, rows // 3 + 5                                         # a shard
    pb, pp = oracle.community_bits(5, blocks, src_rows, True, pathways, S, row_offset=a_, rows=b_ - a_)
    np.testing.assert_array_equal(pb, sb[a_:b_])
    np.testing.assert_array_equal(pp, sp[a_:b_])


def test_community_permute_is_a_seeded_bijection():
    for n in (1, 2, 3, 190, 257, 4096, 4097):
        p = [oracle.community_permute(g, n, 5) for g in range(n)]
        assert sorted(p) == list(range(n))
    n = 190
    p = [oracle.community_permute(g, n, 5) for g in range(n)]
    assert p != [oracle.community_permute(g, n, 5 + 2 ** 32) for g in range(n)]  # high seed half
    assert p != [oracle.community_permute(g, n, 6) for g in range(n)]            # low seed half


def test_community_rows_are_independent_draws():
    """Internal bits depend on the row; external flags on the pair; the dead-row pick on the seed."""
    pathways, (blocks, src_rows, _, _) = community_case(300, [40, 7, 2, 1, 25, 60, 3], 100)
    bits, _ = oracle.community_bits(5, blocks, src_rows, False, pathways, 300)
    m = unpack(bits, 300)
    start, size, size_int, own, off = blocks.tolist()[0]
    assert size_int >= 2
    inner = m[start:start + size][:, pathways[own]]
    assert len({r.tobytes() for r in inner}) == size                        # every row its own draw
    assert not np.array_equal(so.internal_row(5, 0, 300), so.internal_row(5 + 2 ** 32, 0, 300))
    picks = set()
    for seed in range(64):
        flags, extra = so.community_flags(seed, 1, 0, 0, 3, 1)
        assert (extra >= 0) == (not flags.any()) and extra != 1
        picks.add(extra)
    assert {0, 2} <= picks                                                    # both other communities


def test_community_dead_rows_in_the_oracle():
    from bikg_graph_explainability_public_amd.masks import Mask
    import torch
    pathways = [[0, 1, 2], [2, 3], [4]]
    m = Mask(torch.zeros((5, 1)), torch.zeros((2, 0), dtype=torch.long), pathways,
             {"interpret_samples": 2, "epochs": 1}, "node_prediction")
    blocks, src_rows, rows, _ = m.community_plan()
    check_dead_rows(lambda s: unpack(oracle.community_bits(s, blocks, src_rows, False, pathways, 5)[0], 5),
                    pathways, blocks)


# ------------------------------------------------------------------ dispatch query
@pytest.mark.parametrize("cols, want", [
    (1, "k_shapley_flat<1> grid=1x1"), (33, "k_shapley_flat<2> grid=1x1"),
    (96, "k_shapley_flat<1> grid=1x1"), (100, "k_shapley_flat<4> grid=1x1"),
    (128, "k_shapley_flat<4> grid=1x1"),
    (1193, "k_shapley_flat<2> grid=2x1"),       # 37 rows x 10 quads = 370 lanes
    (8064, "k_shapley_flat<4> grid=10x1"),      # 63 quads: the last flat size
    (8065, "k_shapley<1>"), (8100, "k_shapley<2>"), (8190, "k_shapley<4>"), (8192, "k_shapley<4>"),
    (32768, "k_shapley<4>"), (32800, "k_shapley<1>")])
def test_shapley_dispatch_boundaries(cols, want, monkeypatch):
    got = _describe(SH, 37, cols)
    if " " in want:
        assert got == want
        return
    # the 2-D grid: its height follows the device's CU count by default, so only its width here
    gx = 2 if cols > 32768 else 1
    assert got.split()[0] == want and got.split()[1].startswith(f"grid={gx}x")
    monkeypatch.setenv("XPG_DIAGNOSTICS", "1")
    monkeypatch.setenv("XPG_SHAPLEY_BLOCKS", str(3 * gx))   # total blocks -> 3 row-striding ones
    assert _describe(SH, 37, cols) == f"{want} grid={gx}x3"
    monkeypatch.setenv("XPG_SHAPLEY_BLOCKS", "1")            # never fewer than one row of blocks
    assert _describe(SH, 37, cols) == f"{want} grid={gx}x1"
    monkeypatch.setenv("XPG_SHAPLEY_BLOCKS", "-1")           # one row per block
    assert _describe(SH, 37, cols) == f"{want} grid={gx}x37"
    assert _describe(SH, 70000, cols) == f"{want} grid={gx}x65535"


@pytest.mark.parametrize("cols, n_comm, n_blocks, want", [
    (300, 7, 7, "k_communities<1,1,1> grid=25 lds=420"),
    (5984, 64, 64, "k_communities<1,1,1> grid=25 lds=49152"),     # masks + plan = 48 KB exactly
    (5985, 64, 64, "k_communities<1,1,0> grid=25 lds=13250"),
    (8000, 64, 64, "k_communities<1,1,0> grid=25 lds=17280"),
    (8000, 65, 65, "k_communities<0,1,0> grid=25 lds=17348"),     # 65 communities: LDS flags
    (16384, 64, 4, "k_communities<1,1,0> grid=25 lds=32848"),     # the last staged width
    (16385, 64, 4, "k_communities<1,0,0> grid=25 lds=0"),
    (16384, 65, 65, "k_communities<0,1,0> grid=25 lds=34116"),
    (16385, 65, 65, "k_communities<0,0,0> grid=25 lds=48"),
    (3000, 2100, 2100, "k_communities<0,1,0> grid=25 lds=49056"),
    (3000, 3200, 3200, "k_communities<0,0,0> grid=25 lds=1600")])  # plan + columns past 64 KB
def test_community_dispatch_boundaries(cols, n_comm, n_blocks, want):
    assert _describe(CO, 100, cols, n_comm, n_blocks) == want


def test_sampler_dispatch_switches_and_errors(monkeypatch):
    assert _describe(CO, 10000, 300, 7, 7).split()[1] == "grid=2048"          # staged: capped
    assert _describe(CO, 10000, 16385, 7, 7).split()[1] == "grid=2500"
    assert _describe(SH, 0, 300) == "none" and _describe(CO, 0, 300, 7, 7) == "none"
    from bikg_graph_explainability_public_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8)
    assert lib.xpg_sampler_describe(SH, 37, 300, 0, 0, buf, 8) == 3            # XPG_ENOSPC
    assert buf.value == b""
    for bad in [(2, 37, 300, 0, 0), (SH, 37, 0, 0, 0), (SH, -1, 300, 0, 0), (CO, 37, 300, 0, 1),
                (CO, 37, 300, 3, 4), (CO, 37, 300, 32769, 1)]:
        with pytest.raises(RuntimeError):
            _describe(*bad)
    # the diagnostics switches count only with XPG_DIAGNOSTICS=1, as in the launchers
    monkeypatch.setenv("XPG_COMM_PERCOL", "1")
    with pytest.raises(RuntimeError, match="XPG_DIAGNOSTICS"):
        _describe(CO, 100, 300, 7, 7)
    monkeypatch.setenv("XPG_SHAPLEY_BLOCKS", "3")
    with pytest.raises(RuntimeError, match="XPG_DIAGNOSTICS"):
        _describe(SH, 37, 8100)
    assert _describe(SH, 37, 8064) == "k_shapley_flat<4> grid=10x1"            # flat: not read
    monkeypatch.setenv("XPG_DIAGNOSTICS", "1")
    assert _describe(CO, 100, 300, 7, 7) == "k_communities<1,1,0> grid=25 lds=740"
    assert _describe(SH, 37, 8100) == "k_shapley<2> grid=1x3"
