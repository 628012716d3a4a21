"""Structural checks of community-sampler output, shared by the
GPU tests (the kernels' rows) and the CPU tests (the NumPy oracle's rows, which validates the
oracle's restatement of the rule independently of the kernels)."""
import numpy as np
import torch


def community_case(S, lens, samples, seed=0, overlap=0):
    """Disjoint random communities of the given lengths over S columns (+ `overlap` members
    shared by two communities) and their Mask.community_plan()."""
    from bikg_graph_explainability_public_amd.masks import Mask
    rng = np.random.default_rng(seed)
    perm = rng.permutation(S)
    pathways, o = [], 0
    for n in lens:
        pathways.append(sorted(perm[o:o + n].tolist()))
        o += n
    rng = np.random.default_rng(3)
    for _ in range(overlap):  # members shared by two communities
        a, b = rng.choice(len(pathways), 2, replace=False)
        pathways[b] = sorted(set(pathways[b]) | {int(rng.choice(pathways[a]))})
    m = Mask(torch.zeros((S, 1)), torch.zeros((2, 0), dtype=torch.long), pathways,
             {"interpret_samples": samples, "epochs": 2}, "node_prediction")
    return pathways, m.community_plan()


def unpack(bits_u32, cols):
    b = np.ascontiguousarray(bits_u32).view(np.uint8).reshape(bits_u32.shape[0], -1)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :cols].astype(bool)


def check_community_structure(bits_u32, prow, S, pathways, blocks):
    """Unshuffled community rows (uint32 [src_rows, words], pathway_rows) have the reference's
    structure (masks.py:81-194, pathways.py:234-385): uncovered columns off; a clean tail word;
    internal rows touch only the own community; external rows switch whole communities, the
    sorted-position column off, and the first 2h rows are antithetic pairs; pathway_rows = the own
    community; own-community bits have density 0.5 +- 0.05."""
    m = unpack(bits_u32, S)
    covered = np.zeros(S, bool)
    for p in pathways:
        covered[p] = True
    assert not m[:, ~covered].any()
    tail = bits_u32[:, -1] >> np.uint32(S % 32) if S % 32 else 0
    assert np.all(tail == 0)
    P = len(pathways)
    own_bits = []
    for start, size, size_int, own, off in np.asarray(blocks).tolist():
        blk = m[start:start + size]
        assert (prow[start:start + size] == own).all()
        own_bits.append(blk[:, pathways[own]])
        others = [c for c in range(P) if c != own]
        if not others:
            continue
        flags = np.stack([blk[:, pathways[c]].all(1) for c in others], 1)
        anyon = np.stack([blk[:, pathways[c]].any(1) for c in others], 1)
        assert np.array_equal(flags, anyon)                # whole communities switch together
        assert not anyon[:size_int].any()                  # internal rows: own community only
        if off != own:
            assert not flags[size_int:, others.index(off)].any()
        h = (size - size_int) // 2
        keep = [i for i, c in enumerate(others) if c != off]
        a, b = flags[size_int:size_int + h][:, keep], flags[size_int + h:size_int + 2 * h][:, keep]
        assert np.array_equal(a, ~b)                       # antithetic pairs
    ob = np.concatenate([x.ravel() for x in own_bits])
    assert abs(ob.mean() - 0.5) < 0.05


def check_community_shuffle(sb, sp, bits_u32, prow):
    """Shuffled rows are a permutation of the unshuffled ones (and not the identity), the
    pathway rows with them."""
    key = lambda x: sorted(map(bytes, np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1)))
    assert key(sb) == key(bits_u32) and not np.array_equal(sb, bits_u32)
    assert np.array_equal(np.sort(sp), np.sort(prow))


def check_dead_rows(rows_of_seed, pathways, blocks):
    """The 3-community / 5-column case: rows_of_seed(seed) -> bool [src_rows, 5]; every lone
    external row has another community switched on, members it shares with the own community
    aside (those take the internal bits)."""
    for seed in range(64):
        mm = rows_of_seed(seed)
        for start, size, size_int, own, off in np.asarray(blocks).tolist():
            row = mm[start + 1]                            # the lone external row
            outside = [s for s in range(5) if s not in pathways[own]]
            on = [c for c in range(3) if c != own
                  and all(row[s] for s in pathways[c] if s not in pathways[own])]
            assert on, f"seed {seed}: dead external row in block {own}"
            want = np.zeros(5, bool)
            for c in on:
                want[pathways[c]] = True
            assert np.array_equal(row[outside], want[outside])
