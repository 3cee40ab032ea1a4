"""Beacon inputs for the sliding-window prefill forwards.  Test infrastructure only.

tests/window_ref.plant_beacons plants its four keys (just outside and just inside either window edge) for queries 0
and nq - 1 only, with keys that copy the query's vector.  A query-blocked forward can also go wrong at a block edge,
where the block's key end L_b and window start lo_b change; so here the same four keys are planted for the queries on
both sides of the first two block edges as well: {0, P - 1, P, nq - 1} and, with three or more blocks, 2P - 1 and 2P
(P = prefill_beacons.block_shape's P_b).  Neighbours at a block edge sit one position apart and share two of their
four key positions with opposite roles, so the keys cannot copy the query; as in tests/prefill_beacons.py every beacon
has a set of Q / K channels and a set of V channels to itself:
  * Q of the beaconed query (every head of the group) is about 2u on the beacon's channels and 0 elsewhere, and its
    four keys hold u / 2 there, u . u / sqrt(d) = SCORE: four equal scores that tower over every other score of the
    row.  The query's value is the float16 within 10 % of 2u that the kernels' pre-scaling of Q (to float16, by
    scale * log2 e) rounds least (score_ramp._best_prescaled): every channel of a beacon holds the same value, so its
    rounding would not average out over the channels but move the whole score, and with it l, which the gate holds
    to 1e-3, by up to 48 * 2^-11;
  * with pos the query's position and W the window, on the beacon's V channels
      pos - W      just outside the lower edge   V = -x        pos       just inside the upper edge    V = +y
      pos - W + 1  just inside it                V = +x        pos + 1   just outside it               V = -y
    x = BEACON_V on each of them and y = BEACON_V with alternating sign along them.  The right rule answers
    (x + y) / 2 there; dropping an inside key or admitting an outside key moves some channel by BEACON_V * 2 / 3 or
    more (tests/test_window_prefill_beacons.py)."""

import math

import numpy as np

from tests.prefill_beacons import SCORE, block_shape
from tests.score_ramp import _best_prescaled
from tests.window_ref import BEACON_V


def beacon_queries(g, nq):
    """0, nq - 1 and the queries on both sides of the first two block edges, ascending."""
    pb, nqb = block_shape(g, nq)
    qs = {0, nq - 1}
    for edge in (pb, 2 * pb)[:max(min(nqb - 1, 2), 0)]:
        qs |= {edge - 1, edge}
    return sorted(qs)


def values(nv):
    """(x, y) on a beacon's nv V channels."""
    return np.full(nv, BEACON_V, np.float16), (BEACON_V * (1 - 2 * (np.arange(nv) % 2))).astype(np.float16)


def plant(Q, K, V, lens, window, g):
    """Copies of Q [b, d, nq], K [b // g, d, cap], V [b // g, vd, cap] (float16) with the beacons of every K/V slice,
    and the list of (K/V slice, query, V channels) planted.  A beacon one of whose four keys lies outside
    [0, capacity) is skipped (the caller asserts that none was); key pos + 1 of the last query lies past the length and
    is planted all the same (the right rule never reads it)."""
    Q, K, V = Q.copy(), K.copy(), V.copy()
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    qs = beacon_queries(g, nq)
    nb = len(qs)
    assert nb <= d // 4 and 2 * nb <= vd, "too many beacons for disjoint channels"
    assert window >= 2, "a beacon's four keys are distinct from W = 2 on"
    planted = []
    for s in range(K.shape[0]):
        L = min(max(int(lens[s]), 0), cap)
        for t, q in enumerate(qs):
            pos = L - nq + q
            if pos - window < 0 or pos + 1 >= cap:
                continue
            ch, vch = np.arange(t, d, nb), np.arange(t, vd, nb)
            base = math.sqrt(SCORE * math.sqrt(d) / len(ch))
            x, y = values(len(vch))
            Q[s * g:(s + 1) * g, :, q] = 0
            Q[s * g:(s + 1) * g, ch, q] = np.float16(_best_prescaled(d, 1.8 * base, 2.2 * base))
            for key, val in ((pos - window, -x), (pos - window + 1, x), (pos, y), (pos + 1, -y)):
                K[s, ch, key] = np.float16(base / 2)
                V[s, vch, key] = val
            planted.append((s, q, vch))
    return Q, K, V, planted
