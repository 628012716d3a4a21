"""ORACLE — test infrastructure only: the device mask samplers' draws, restated in NumPy.

The device samplers are counter-based: every word they write is one output of Philox4x32-10
(Salmon et al., SC'11; checked here against the Random123 known-answer vectors) under the key
(lo32(seed), hi32(seed)) and a counter that names what the word is.  This module restates the
counter layout documented beside the kernels and in include/xpgnn.h, per row and per column, so
the kernels' lane / ballot / LDS mechanics have an independent check:

  Shapley          (quad q, lo32(g), hi32(g), 0x58504721)  -> words 4q .. 4q+3 of global row g
  community flags  (word w, block b, pair index kk, 0x434F4D31).x
  dead-row pick    (0, block b, external row k, 0x44454144).x
  internal bits    (word w, source row, 0, 0x494E5431).x

`shapley_bits` is the iid-fair-bits draw of Mask.shapley_mask; `community_bits` the rule of
Mask.get_internal_mask / get_external_indices + Pathways.mask_generator / activate_dead_mask /
pathway_mask2node_mask and the row shuffle (masks.py:81-194, 375-380; pathways.py:234-385) as the
comment above k_communities states it.
"""
import numpy as np

__all__ = ["philox4x32_10", "shapley_bits", "comm_mix", "community_permute", "community_bits",
           "popcount_rows"]

_M32 = 0xFFFFFFFF
TAG_SHAPLEY, TAG_FLAGS, TAG_DEAD, TAG_INTERNAL = 0x58504721, 0x434F4D31, 0x44454144, 0x494E5431


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(counter4, key2):
    """Philox4x32 with 10 rounds.  counter4 = four arrays (or scalars) of 32-bit values that
    broadcast against each other, key2 = two; returns the four output words as uint32 arrays of
    the broadcast shape."""
    m32 = np.uint64(_M32)
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & m32 for c in counter4])
    k0, k1 = (_u64(k) & m32 for k in key2)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0   # < 2^64: both factors are < 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32)
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & _M32, seed >> 32


def shapley_bits(seed, row_offset, rows, cols):
    """uint32 [rows, ceil(cols / 32)]: the Shapley rows [row_offset, row_offset + rows) of `seed`.
    Bit c of a row is bit (c & 31) of word c >> 5; bits past `cols` are 0."""
    words = (cols + 31) // 32
    quads = (words + 3) // 4
    g = [int(row_offset) + r for r in range(rows)]
    lo = np.array([x & _M32 for x in g], dtype=np.uint64).reshape(rows, 1)
    hi = np.array([(x >> 32) & _M32 for x in g], dtype=np.uint64).reshape(rows, 1)
    q = np.arange(quads, dtype=np.uint64).reshape(1, quads)
    out = philox4x32_10((q, lo, hi, TAG_SHAPLEY), _key(seed))
    bits = np.stack(out, axis=-1).reshape(rows, quads * 4)[:, :words].copy()
    if cols % 32:
        bits[:, -1] &= np.uint32((1 << (cols % 32)) - 1)
    return bits


def popcount_rows(bits):
    """int32 [rows]: set bits per row of a uint32 [rows, words] array."""
    b = np.ascontiguousarray(bits).view(np.uint8).reshape(bits.shape[0], -1)
    return np.unpackbits(b, axis=1).sum(axis=1).astype(np.int32)


def comm_mix(x, k):
    """Round function of the row shuffle (32-bit multiply-xorshift finaliser)."""
    x = (x ^ k) & _M32
    x = (x * 0x9E3779B1) & _M32
    x ^= x >> 16
    x = (x * 0x85EBCA77) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def community_permute(g, src_rows, seed):
    """Source row of output row g: a 4-round balanced Feistel network on 2 * hb bits, hb =
    ceil(bitlen(src_rows - 1) / 2) (at least 1), walked along its cycle until it lands in
    [0, src_rows) — a bijection of that range."""
    k0, k1 = _key(seed)
    k0 ^= 0x5EED1234
    k1 ^= 0x0F00D321
    hb = (max(1, int(src_rows - 1).bit_length()) + 1) // 2
    m = (1 << hb) - 1
    x = int(g)
    while True:
        left, right = x >> hb, x & m
        for i in range(4):
            rk = ((k1 if i & 1 else k0) + 0x632BE5AB * i) & _M32
            left, right = right, left ^ (comm_mix(right, rk) & m)
        x = (left << hb) | right
        if x < src_rows:
            return x


def _word_bits(words_u32, n):
    """bool [n]: the first n bits of a uint32 word array, bit i = bit (i & 31) of word i >> 5."""
    return np.unpackbits(np.ascontiguousarray(words_u32).view(np.uint8), bitorder="little")[:n].astype(bool)


def community_flags(seed, b, k, h, n_comm, off):
    """(bool [n_comm] flags, extra) of external row k >= 0 of block b, h = its antithetic pairs.
    Rows k < h draw one flag word per 32 communities; rows h <= k < 2h are the complements of
    rows k - h; the odd row k = 2h draws its own.  Community `off` is cleared.  extra: the
    community a lone external row (h = 0) with no flag on switches on instead, else -1."""
    kk = k if k < h else (k - h if k < 2 * h else 2 * h)
    w = np.arange((n_comm + 31) // 32, dtype=np.uint64)
    v = philox4x32_10((w, b, kk, TAG_FLAGS), _key(seed))[0]
    if h <= k < 2 * h:
        v = ~v
    flags = _word_bits(v, n_comm)
    flags[off] = False
    extra = -1
    if h == 0 and n_comm > 1 and not flags.any():
        extra = int(philox4x32_10((0, b, k, TAG_DEAD), _key(seed))[0]) % (n_comm - 1)
        if extra >= off:
            extra += 1
    return flags, extra


def internal_row(seed, src, cols):
    """bool [cols]: the internal random bits of source row `src` (used on its own community)."""
    w = np.arange((cols + 31) // 32, dtype=np.uint64)
    return _word_bits(philox4x32_10((w, src, 0, TAG_INTERNAL), _key(seed))[0], cols)


def community_bits(seed, blocks, src_rows, shuffle, communities, cols, row_offset=0, rows=None):
    """(bits uint32 [rows, words], pathway_rows int32 [rows]) of the community sampler's global
    rows [row_offset, row_offset + rows) (rows = None: up to src_rows).  blocks = [n_blocks, 5]
    {row_start, size, size_internal, own, off} as Mask.community_plan lays them out."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 5)
    rows = int(src_rows) - row_offset if rows is None else rows
    n_comm = len(communities)
    member = [np.asarray(c, dtype=np.int64) for c in communities]
    col_of = np.concatenate(member) if n_comm else np.zeros(0, np.int64)
    comm_of = np.repeat(np.arange(n_comm), [len(c) for c in member])
    mask = np.zeros((rows, cols), dtype=bool)
    prow = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        g = row_offset + r
        src = community_permute(g, src_rows, seed) if shuffle else g
        b = int(np.searchsorted(blocks[:, 0], src, side="right")) - 1
        start, size, size_int, own, off = (int(x) for x in blocks[b])
        k = src - start - size_int
        on = np.zeros(n_comm, dtype=bool)
        if k >= 0:  # an external coalition row
            on, extra = community_flags(seed, b, k, (size - size_int) // 2, n_comm, off)
            if extra >= 0:
                on[extra] = True
        row = mask[r]
        row[col_of[on[comm_of]]] = True            # every member of a switched-on community
        mine = np.zeros(cols, dtype=bool)
        mine[member[own]] = True
        row[mine] = internal_row(seed, src, cols)[mine]  # own members: the internal bits instead
        prow[r] = own
    packed = np.packbits(mask, axis=1, bitorder="little")
    words = (cols + 31) // 32
    out = np.zeros((rows, words * 4), dtype=np.uint8)
    out[:, :packed.shape[1]] = packed
    return out.view(np.uint32), prow
