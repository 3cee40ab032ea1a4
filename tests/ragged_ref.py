"""Float64 reference of the ragged few-query forward (include/fa_api.h, "Ragged few-query forward"): Q slice bi
attends the first L keys of K/V slice bi // g, L = lens[bi // g] clamped to [0, capacity]; with ``tail_causal``
query i sees keys j <= L - nq + i.  Written directly from that definition (one mask per slice); tests/
test_ragged_ref.py checks it against oracle.forward_f64 on truncated K / V and against the merge of two oracle
calls.  Test infrastructure only."""

import math

import numpy as np


def ragged_mask(nq, cap, length, tail_causal):
    """bool [nq, cap]: the keys each query sees in a slice of ``length`` live keys."""
    L = min(max(int(length), 0), cap)
    j = np.arange(cap)[None, :]
    mask = np.broadcast_to(j < L, (nq, cap)).copy()
    if tail_causal:
        mask &= j <= (L - nq + np.arange(nq))[:, None]
    return mask


def forward_f64(Q, K, V, lens, g=1, tail_causal=False):
    """Q [b, d, nq], K [b // g, d, cap], V [b // g, vd, cap] (dtype-rounded inputs), ``lens`` one length per K/V
    slice.  Returns (O [b, vd, nq], L [b, nq], M [b, nq], has_any [b, nq]): M the row max of the scaled scores,
    L = sum exp(s - M), both float64 and unrounded; rows without a key have O = L = M = 0 and has_any False.
    Keys at or past a slice's length are never read, whatever they hold."""
    b, d, nq = Q.shape
    bkv, vd, cap = V.shape
    assert b == bkv * g and K.shape == (bkv, d, cap) and len(lens) == bkv
    scale = 1.0 / math.sqrt(d)
    O = np.zeros((b, vd, nq))
    Ls = np.zeros((b, nq))
    M = np.zeros((b, nq))
    has_any = np.zeros((b, nq), dtype=bool)
    for bi in range(b):
        s_kv = bi // g
        L = min(max(int(lens[s_kv]), 0), cap)
        mask = ragged_mask(nq, cap, L, tail_causal)[:, :L]
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
