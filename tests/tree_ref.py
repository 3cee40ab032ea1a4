"""Float64 reference of the tree-masked draft forwards (include/fa_api.h, "Tree-masked draft attention"): Q slice bi
attends K/V slice bi // g of L live keys, L = lens[bi // g] clamped to [0, capacity].  With base = L - nq, draft slot
j is key base + j, and query i sees key k iff 0 <= k < L and (k < base or bit j = k - base of its mask row is set).
Written directly from that rule, one boolean mask per slice; tests/test_tree_ref.py checks it against
ragged_ref.forward_f64.  Test infrastructure only."""

import math

import numpy as np


def mask_words(nq):
    return (nq + 31) // 32


def pack_mask(bits):
    """bool [..., nq, nq] (row i, slot j) -> uint32 [..., nq, W]: bit j & 31 of word j >> 5."""
    bits = np.asarray(bits, dtype=bool)
    nq = bits.shape[-1]
    W = mask_words(nq)
    padded = np.zeros(bits.shape[:-1] + (32 * W,), dtype=np.uint64)
    padded[..., :nq] = bits
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(bits.shape[:-1] + (W, 32)) * weights).sum(axis=-1).astype(np.uint32)


def unpack_mask(words, nq):
    """uint32 [..., nq, W] -> bool [..., nq, nq]; bits at or past nq are dropped, whatever they hold."""
    words = np.asarray(words).astype(np.uint32)
    j = np.arange(nq)
    return ((words[..., j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def set_unused_bits(words, nq):
    """A copy of uint32 [..., nq, W] with the bits at or past nq of the last word set to ones."""
    out = np.array(words, dtype=np.uint32, order="C")
    if nq % 32:
        out[..., -1] |= np.uint32((0xFFFFFFFF << (nq % 32)) & 0xFFFFFFFF)
    return out


def lower_triangle(nq):
    """The chain: bit j of row i set iff j <= i (the tail-causal rule)."""
    return pack_mask(np.tril(np.ones((nq, nq), dtype=bool)))


def ancestors(parents):
    """int [..., nq] with parents[i] < i or -1 -> bool [..., nq, nq]: node i sees itself and its ancestors."""
    parents = np.asarray(parents)
    nq = parents.shape[-1]
    flat = parents.reshape(-1, nq)
    out = np.zeros((flat.shape[0], nq, nq), dtype=bool)
    for s, par in enumerate(flat):
        for i in range(nq):
            k = i
            while k >= 0:
                out[s, i, k] = True
                assert par[k] < k
                k = int(par[k])
    return out.reshape(parents.shape + (nq,))


def tree_mask(nq, cap, length, words):
    """bool [nq, cap]: the keys each query sees in a slice of ``length`` live keys under mask rows uint32 [nq, W]."""
    L = min(max(int(length), 0), cap)
    base = L - nq
    bits = unpack_mask(words, nq)
    k = np.arange(cap)
    mask = np.zeros((nq, cap), dtype=bool)
    mask[:, (k < L) & (k < base)] = True
    for j in range(nq):
        if 0 <= base + j < L:
            mask[:, base + j] = bits[:, j]
    return mask


def forward_f64(Q, K, V, lens, masks, g=1, kv_per_len=1):
    """Q [b, d, nq], K [b // g, d, cap], V [b // g, vd, cap] (dtype-rounded inputs), ``lens`` one length per K/V
    slice, ``masks`` uint32 [sequences, nq, W] with sequence = K/V slice // kv_per_len.  Returns tests/ragged_ref.
    forward_f64's (O [b, vd, nq], L [b, nq], M [b, nq], has_any [b, nq]): M the row max of the scaled scores,
    L = sum exp(s - M), float64 and unrounded; rows without a key have O = L = M = 0 and has_any False."""
    b, d, nq = Q.shape
    bkv, vd, cap = V.shape
    assert b == bkv * g and K.shape == (bkv, d, cap) and len(lens) == bkv
    masks = np.asarray(masks)
    assert masks.shape == (bkv // kv_per_len, nq, mask_words(nq))
    scale = 1.0 / math.sqrt(d)
    O = np.zeros((b, vd, nq))
    Ls = np.zeros((b, nq))
    M = np.zeros((b, nq))
    has_any = np.zeros((b, nq), dtype=bool)
    for bi in range(b):
        s_kv = bi // g
        L = min(max(int(lens[s_kv]), 0), cap)
        mask = tree_mask(nq, cap, L, masks[s_kv // kv_per_len])[:, :L]
        ha = mask.any(axis=1)
        has_any[bi] = ha
        if not ha.any():
            continue
        k = K[s_kv, :, :L].astype(np.float64)
        v = V[s_kv, :, :L].astype(np.float64)
        s = np.where(mask, (Q[bi].astype(np.float64).T @ k) * scale, -np.inf)
        m = np.where(ha, s.max(axis=1, initial=-np.inf), 0.0)
        p = np.exp(s - m[:, None])
        l = p.sum(axis=1)
        o = v @ (p / np.where(ha, l, 1.0)[:, None]).T
        o[:, ~ha] = 0.0
        O[bi], Ls[bi], M[bi] = o, np.where(ha, l, 0.0), m
    return O, Ls, M, has_any
