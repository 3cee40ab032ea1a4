"""CPU tests of tests/window_prefill_beacons.py: on its inputs, at the GPU tests' trap shapes, moving either end of the
window by one key (tests/window_ref.forward_f64's lo_shift / hi_shift) moves O by at least BEACON_V / 4 on every
planted row, which is hundreds of times the allowance of the GPU gate, while the right rule as a forward would store
it (O rounded to float16) stays inside that allowance.  So a GPU result that passes the gate on these inputs has both
edges right at queries 0 and nq - 1 and on both sides of the first two block edges."""

import numpy as np
import pytest

from tests import gate
from tests import prefill_beacons as B
from tests import window_prefill_beacons as WB
from tests import window_ref as W
from tests.gate import TOL

CAP = 2600
# (g, nq, d, vd): two blocks with a one-query tail; three blocks, the last short; the lane trap; two full blocks
SHAPES = [(1, 129, 64, 64), (8, 37, 32, 40), (16, 20, 64, 64), (1, 256, 128, 128), (128, 2, 64, 64)]


def _inputs(b, g, nq, d, vd, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(b, d, nq), mk(b // g, d, CAP), mk(b // g, vd, CAP)


def test_the_beaconed_queries_straddle_the_block_edges():
    assert WB.beacon_queries(1, 129) == [0, 127, 128]
    assert WB.beacon_queries(1, 256) == [0, 127, 128, 255]
    assert WB.beacon_queries(8, 37) == [0, 15, 16, 31, 32, 36]
    assert WB.beacon_queries(16, 20) == [0, 7, 8, 15, 16, 19]
    assert WB.beacon_queries(8, 100) == [0, 15, 16, 31, 32, 99]
    assert WB.beacon_queries(128, 2) == [0, 1]
    assert WB.beacon_queries(4, 7) == [0, 6] and WB.beacon_queries(1, 1) == [0]


@pytest.mark.parametrize("window", [2, 64, 513])
@pytest.mark.parametrize("g,nq,d,vd", SHAPES)
def test_an_off_by_one_edge_moves_o_by_a_quarter_beacon_on_every_planted_row(g, nq, d, vd, window):
    pb = B.block_shape(g, nq)[0]
    # every planted key exists: L - nq - W >= 0 and L + 1 <= capacity; the second puts block 1's window start on key 0
    lens = [window + nq + 700, window + nq, CAP - 1]
    Q, K, V = _inputs(len(lens) * g, g, nq, d, vd, seed=window + nq)
    Q, K, V, planted = WB.plant(Q, K, V, lens, window, g)
    assert len(planted) == len(lens) * len(WB.beacon_queries(g, nq))  # none skipped
    assert {q for _, q, _ in planted} >= {0, pb - 1, pb, nq - 1}
    right = W.forward_f64(Q, K, V, lens, window, g)[0]
    allow = gate.plain_bound(right, *TOL[np.float16]["fwd"])
    stored = right.astype(np.float16).astype(np.float64)
    assert (np.abs(stored - right) <= allow).all()
    for s, q, vch in planted:  # the two inside keys carry nearly all of the row's weight
        x, y = WB.values(len(vch))
        for bi in range(s * g, (s + 1) * g):
            assert np.abs(right[bi, vch, q] - (x.astype(np.float64) + y) / 2).max() < 0.02, (s, q)
    for lo_shift, hi_shift in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        wrong = W.forward_f64(Q, K, V, lens, window, g, lo_shift=lo_shift, hi_shift=hi_shift)[0]
        for s, q, vch in planted:
            for bi in range(s * g, (s + 1) * g):
                moved = np.abs(wrong[bi, :, q] - right[bi, :, q])
                assert moved.max() >= W.BEACON_V / 4, (lo_shift, hi_shift, s, q, moved.max())
                assert (moved / allow[bi, :, q]).max() > 100
