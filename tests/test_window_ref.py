"""CPU tests of tests/window_ref.py, the float64 reference of the sliding-window decode forwards: against
oracle.forward_f64 on the slice of K / V that one query's window is, against tests/ragged_ref.py where the window
reaches the capacity, and the boundary sensitivity of its beacon inputs: on them, moving either end of the window by
one key moves O by far more than the allowance of tests.test_gpu_ragged._check_ref's rule, so a GPU result that
passes that rule on these inputs has both edges right.  (With random inputs an off-by-one edge drops or admits one
key among hundreds and hides below the fp16 tolerance.)"""

import numpy as np
import pytest

from oracle import fa_oracle as O
from tests import gate
from tests import ragged_ref
from tests import window_ref as W
from tests.gate import TOL

D, VD, CAP = 8, 6, 40


def _inputs(b, g, nq, seed, d=D, vd=VD, cap=CAP):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(b, d, nq), mk(b // g, d, cap), mk(b // g, vd, cap)


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("window", [1, 2, 7, CAP - 1])
def test_one_query_is_the_oracle_on_the_sliced_keys(g, window):
    lens = [0, 1, 2, window, window + 1, 23, CAP, CAP + 9, -4]
    Q, K, V = _inputs(len(lens) * g, g, 1, seed=window)
    got = W.forward_f64(Q, K, V, lens, window, g)
    for bi in range(Q.shape[0]):
        L = min(max(lens[bi // g], 0), CAP)
        lo = max(0, L - window)
        assert lo == W.window_lo(L, 1, window, CAP)
        if L == 0:
            assert not got[3][bi].any() and not got[0][bi].any() and not got[1][bi].any()
            continue
        ref = O.forward_f64(Q[bi][None], K[bi // g][None, :, lo:L], V[bi // g][None, :, lo:L],
                            O.Problem("full", 1, "none_front"))
        for a, r in zip(got[:3], ref[:3]):
            np.testing.assert_allclose(a[bi], r[0], rtol=1e-12, atol=1e-12)
        assert got[3][bi].all()


@pytest.mark.parametrize("g,nq", [(1, 1), (1, 5), (2, 7)])
@pytest.mark.parametrize("window", [CAP, CAP + 1, 10 * CAP])
def test_a_window_that_reaches_the_capacity_is_the_tail_rule(g, nq, window):
    lens = [0, 1, nq - 1, nq, nq + 1, 23, CAP]
    Q, K, V = _inputs(len(lens) * g, g, nq, seed=10 + nq)
    for a, r in zip(W.forward_f64(Q, K, V, lens, window, g), ragged_ref.forward_f64(Q, K, V, lens, g, True)):
        assert np.array_equal(a, r)


def test_each_query_sees_w_keys_ending_at_its_position():
    nq, window = 5, 4
    for L in range(0, CAP + 1):
        mask = W.window_mask(nq, CAP, L, window)
        for i in range(nq):
            pos = L - nq + i
            want = set(range(max(0, pos - window + 1), pos + 1)) if pos >= 0 else set()
            assert set(np.nonzero(mask[i])[0].tolist()) == want
        seen = np.nonzero(mask.any(axis=0))[0]
        if len(seen):
            assert seen[0] == W.window_lo(L, nq, window, CAP) and seen[-1] == L - 1
            assert len(seen) <= min(CAP, window + nq - 1)


def test_keys_outside_the_window_are_not_read():
    lens, window, nq = [30, 0], 6, 3
    Q, K, V = _inputs(2, 1, nq, seed=4)
    ref = W.forward_f64(Q, K, V, lens, window)
    K2, V2 = K.copy(), V.copy()
    lo = W.window_lo(30, nq, window, CAP)
    K2[0, :, :lo], V2[0, :, :lo], K2[0, :, 30:], V2[0, :, 30:], K2[1], V2[1] = np.nan, np.inf, np.inf, np.nan, np.nan, np.nan
    for a, b in zip(W.forward_f64(Q, K2, V2, lens, window), ref):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ boundary sensitivity of the beacon inputs
@pytest.mark.parametrize("window", [64, 65, 512, 513])
@pytest.mark.parametrize("nq", [1, 4])
def test_an_off_by_one_edge_moves_o_beyond_the_gate_on_beacon_inputs(window, nq):
    """The GPU tests' shapes (d = 64, capacity 2600).  For every planted (slice, query) and each of the four wrong
    rules (lower edge one key down / up, upper edge one key down / up) some channel of O differs from the right
    rule's by more than 100 x the allowance atol * max(|O|, 1) + rtol * |O| of _check_ref."""
    d = vd = 64
    cap, g = 2600, 2
    lens = [window + nq + 700, cap - 1, 1500]
    Q, K, V = _inputs(len(lens) * g, g, nq, seed=window + nq, d=d, vd=vd, cap=cap)
    K, V, rows = W.plant_beacons(Q, K, V, lens, window, g)
    assert len(rows) == len(lens) * len(W.beacon_queries(nq))
    right = W.forward_f64(Q, K, V, lens, window, g)[0]
    allow = gate.plain_bound(right, *TOL[np.float16]["fwd"])
    for lo_shift, hi_shift in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        wrong = W.forward_f64(Q, K, V, lens, window, g, lo_shift=lo_shift, hi_shift=hi_shift)[0]
        for bi, i in rows:
            ratio = (np.abs(wrong[bi, :, i] - right[bi, :, i]) / allow[bi, :, i]).max()
            assert ratio > 100, (lo_shift, hi_shift, bi, i, ratio)
    # and the beacons do what they are meant to: the two inside keys carry nearly all of the row's weight
    x, y = np.full(vd, W.BEACON_V), W.BEACON_V * (1 - 2 * (np.arange(vd) % 2))
    for bi, i in rows:
        assert np.abs(right[bi, :, i] - (x + y) / 2).max() < 0.1
