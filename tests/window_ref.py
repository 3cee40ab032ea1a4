"""Float64 reference of the sliding-window decode forwards (include/fa_api.h, "Sliding-window decode"): Q slice bi
attends K/V slice bi // g of L = lens[bi // g] live keys (clamped to [0, capacity]); the nq queries are the last nq
positions, query i sits at pos_i = L - nq + i and sees the keys max(0, pos_i - W + 1) <= j <= pos_i.  Written
directly from that definition (one mask per slice); tests/test_window_ref.py checks it against oracle.forward_f64 on
a sliced K / V and against tests/ragged_ref.py for a window that reaches the capacity.

``lo_shift`` / ``hi_shift`` move the lower / upper end of every query's interval by that many keys: a WRONG rule, there
so that tests/test_window_ref.py can show that the "beacon" inputs below tell an off-by-one edge from the right one.
Test infrastructure only."""

import math

import numpy as np


def window_lo(length, nq, window, cap):
    """The first key the block as a whole sees: max(0, L - nq - W + 1), L the clamped length."""
    L = min(max(int(length), 0), cap)
    return max(0, L - nq - int(window) + 1)


def window_mask(nq, cap, length, window, lo_shift=0, hi_shift=0):
    """bool [nq, cap]: the keys each query sees in a slice of ``length`` live keys under window W."""
    L = min(max(int(length), 0), cap)
    j = np.arange(cap)[None, :]
    pos = (L - nq + np.arange(nq))[:, None]
    mask = (j >= pos - int(window) + 1 + lo_shift) & (j <= pos + hi_shift) & (j >= 0)
    return mask & (pos >= 0) & ((j < L) if hi_shift <= 0 else (j < cap))


def forward_f64(Q, K, V, lens, window, g=1, lo_shift=0, hi_shift=0):
    """Q [b, d, nq], K [b // g, d, cap], V [b // g, vd, cap] (dtype-rounded inputs), ``lens`` one length per K/V
    slice.  Returns (O [b, vd, nq], L [b, nq], M [b, nq], has_any [b, nq]) as tests/ragged_ref.forward_f64 does.
    Only the keys of a query's interval are read, whatever the others hold."""
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
        mask = window_mask(nq, cap, lens[s_kv], window, lo_shift, hi_shift)
        ha = mask.any(axis=1)
        has_any[bi] = ha
        if not ha.any():
            continue
        cols = np.nonzero(mask.any(axis=0))[0]
        j0, j1 = int(cols[0]), int(cols[-1]) + 1  # nothing outside [j0, j1) is touched
        mk = mask[:, j0:j1]
        k = K[s_kv, :, j0:j1].astype(np.float64)
        v = V[s_kv, :, j0:j1].astype(np.float64)
        s = np.where(mk, (Q[bi].astype(np.float64).T @ k) * scale, -np.inf)
        m = np.where(ha, s.max(axis=1, initial=-np.inf), 0.0)
        p = np.exp(s - m[:, None])
        l = p.sum(axis=1)
        o = v @ (p / np.where(ha, l, 1.0)[:, None]).T
        o[:, ~ha] = 0.0
        O[bi], Ls[bi], M[bi] = o, np.where(ha, l, 0.0), m
    return O, Ls, M, has_any


# ---- beacon inputs: an off-by-one window edge moves O by far more than the fp16 tolerance
BEACON_V = 1.5


def beacon_queries(nq):
    """The queries that get beacons: the first and the last (their four keys each are then distinct for W >= 4)."""
    return sorted({0, nq - 1})


def plant_beacons(Q, K, V, lens, window, g=1):
    """Copies of K and V in which, for every K/V slice and every beacon query i of its FIRST head (position
    pos = L - nq + i), four keys equal that query's vector, so their scores |q|^2 / sqrt(d) tower over a random key's:
      pos - W      just outside the lower edge   V = -x        pos       just inside the upper edge    V = +y
      pos - W + 1  just inside it                V = +x        pos + 1   just outside it               V = -y
    with x = BEACON_V on every channel and y = BEACON_V with alternating sign, so dropping either inside key or
    admitting either outside key moves O by about BEACON_V / 2 or more on some channel.  Keys outside [0, capacity)
    are left out; key pos + 1 of the last query lies past the length and is planted all the same (the right rule
    never reads it).  Returns (K, V, rows): rows [(bi, i)] the planted (Q slice, query) pairs whose four keys all
    exist inside the capacity and whose lower pair lies at or above key 0."""
    K, V = K.copy(), V.copy()
    b, d, nq = Q.shape
    bkv, vd, cap = V.shape
    x = np.full(vd, BEACON_V, np.float16)
    y = (BEACON_V * (1 - 2 * (np.arange(vd) % 2))).astype(np.float16)
    rows = []
    for s in range(bkv):
        L = min(max(int(lens[s]), 0), cap)
        bi = s * g
        for i in beacon_queries(nq):
            pos = L - nq + i
            keys = [(pos - window, -x), (pos - window + 1, x), (pos, y), (pos + 1, -y)]
            if pos - window < 0 or pos + 1 >= cap:
                continue
            for j, val in keys:
                K[s, :, j] = Q[bi, :, i]
                V[s, :, j] = val
            rows.append((bi, i))
    return K, V, rows
