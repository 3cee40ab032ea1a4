"""Beacon inputs for the query-blocked forwards, and a float64 reference that takes each query's
newest key directly.  Test infrastructure only.

Random Q, K, V hide an off-by-one in a key bound: one key more or less among hundreds moves O by less than the fp16
tolerance.  A beacon makes it a gross error.  Under the tail rule query i of a slice of L live keys sits at position
pos = L - nq + i.  For the first and the last query of every query block (block_shape) `plant` writes, on a set of
channels that the beacon has to itself,
  * into Q (every head of the group) a vector 2u, and u / 2 into K at key pos and at key pos + 1, scaled so that
    u . u / sqrt(d) = SCORE towers over every other score of the row;
  * into V at key pos the value +A and at key pos + 1 the value -A, on the beacon's V channels.
The query sees pos and not pos + 1, so its O is +A there; seeing pos + 1 too makes it 0, and losing pos makes it the
average of the other keys.  Beacons of one slice use disjoint channels, so the neighbours at a block edge (the last
query of a block and the first of the next, one position apart) do not disturb each other: key pos of the second
holds both vectors."""

import math

import numpy as np
import torch

SCORE = 48.0   # the beacon's scaled score; random scores stay below about 15
A = 2.0


def block_shape(g, nq):
    """(P_b, nqb): include/fa_api.h's block shape."""
    pb = max(p for p in (1, 2, 4, 8, 16, 32, 64, 128) if g * p <= 128)
    return pb, -(-nq // pb)


def beacon_queries(g, nq):
    """The first and the last query of every block, ascending."""
    pb, nqb = block_shape(g, nq)
    return sorted({q for qb in range(nqb) for q in (qb * pb, min(nq, (qb + 1) * pb) - 1)})


def plant(Q, K, V, lens, g):
    """Copies of Q [b, d, nq], K [b // g, d, cap], V [b // g, vd, cap] (float16) with the beacons of every slice whose
    position is inside the sequence, and the list of (K/V slice, query, pos, V channels) planted."""
    Q, K, V = Q.copy(), K.copy(), V.copy()
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    qs = beacon_queries(g, nq)
    nb = len(qs)
    assert nb <= d // 4 and nb <= vd // 2, "too many blocks for disjoint beacon channels"
    planted = []
    for s in range(K.shape[0]):
        L = min(max(int(lens[s]), 0), cap)
        for t, q in enumerate(qs):
            pos = L - nq + q
            if pos < 0:
                continue
            ch = np.arange(t, d, nb)
            # three quarters of the tower's height come from the query: the two keys stay near the magnitude of
            # the others (about 3 against 2), so the scores of the OTHER queries against them, and with them the
            # rounding those scores carry from the fp16 pre-scaled Q, stay what the gate's tolerance was made for
            base = math.sqrt(SCORE * math.sqrt(d) / len(ch))
            q_amp, k_amp = np.float16(2 * base), np.float16(base / 2)
            vch = np.arange(t, vd, nb)
            # the beacon's channels belong to it alone, in the queries of the slice and in the keys near it
            Q[s * g:(s + 1) * g, :, q] = 0
            Q[s * g:(s + 1) * g, ch, q] = q_amp
            for k, sign in ((pos, 1.0), (pos + 1, -1.0)):
                if k < cap:
                    K[s, ch, k] = k_amp
                    V[s, vch, k] = np.float16(sign * A)
            planted.append((s, q, pos, vch))
    return Q, K, V, planted


def tail_khi(lens, g, b, nq, cap):
    """[b, nq]: the newest key query i of Q slice bi sees under the tail rule, L - nq + i (below 0: none)."""
    L = np.clip(np.repeat(np.asarray(lens), g)[:b], 0, cap)
    return L[:, None] - nq + np.arange(nq)[None, :]


def forward_khi_f64(Q, K, V, khi, g, rows=None):
    """ragged_ref.forward_f64's tuple where query i of Q slice bi sees the keys [0, min(khi[bi, i], cap - 1)].
    rows: only these (bi, i) pairs are computed (the others are zero / False)."""
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    scale = 1.0 / math.sqrt(d)
    O, Ls, M = np.zeros((b, vd, nq)), np.zeros((b, nq)), np.zeros((b, nq))
    ha = np.zeros((b, nq), bool)
    for bi, i in (rows if rows is not None else [(bi, i) for bi in range(b) for i in range(nq)]):
        n = min(int(khi[bi, i]) + 1, cap)
        if n <= 0:
            continue
        k, v = K[bi // g, :, :n].astype(np.float64), V[bi // g, :, :n].astype(np.float64)
        s = (Q[bi, :, i].astype(np.float64) @ k) * scale
        m = s.max()
        p = np.exp(s - m)
        O[bi, :, i], Ls[bi, i], M[bi, i], ha[bi, i] = v @ (p / p.sum()), p.sum(), m, True
    return O, Ls, M, ha


def as_outputs(ref):
    """(O, l, m) as a forward would store a float64 reference: O and m rounded to float16, l relative to the stored
    m in float32, the rows without a key O = 0, l = 0, m of bytes 0xFA (CPU tensors)."""
    O64, L64, M64, ha = ref
    m16 = M64.astype(np.float16)
    l = np.where(ha, L64 * np.exp(M64 - m16.astype(np.float64)), 0.0).astype(np.float32)
    m16 = np.where(ha, m16, np.frombuffer(b"\xfa\xfa", np.float16)[0])
    o = np.where(ha[:, None, :], O64, 0.0).astype(np.float16)
    return torch.from_numpy(o), torch.from_numpy(l), torch.from_numpy(m16)
