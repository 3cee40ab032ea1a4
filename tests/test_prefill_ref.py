"""CPU tests of what the GPU tests of the query-blocked forwards stand on: tests/ragged_ref.py at
more than 128 queries against the oracle, the identity that makes one query block the twin's problem, and the beacon
inputs of tests/prefill_beacons.py: the gate of tests/test_gpu_ragged._check_ref must refuse a result in which any
one block's key end L_b, or any one beaconed query's newest key, is off by one in either direction."""

import numpy as np
import pytest

from oracle import fa_oracle as O
from tests import prefill_beacons as B
from tests import ragged_ref as R
from tests import test_gpu_ragged as rg


def _inputs(b, g, d, vd, nq, cap, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(b, d, nq), mk(b // g, d, cap), mk(b // g, vd, cap)


@pytest.mark.parametrize("nq", [129, 260])
def test_the_reference_at_full_length_is_the_oracles_causal_rule(nq):
    """L = nq = cap: query i sees j <= i."""
    Q, K, V = _inputs(2, 1, 8, 6, nq, nq, seed=nq)
    got = R.forward_f64(Q, K, V, [nq, nq], 1, tail_causal=True)
    ref = O.forward_f64(Q, K, V, O.Problem("causal", 1, "none_front"))
    for a, r in zip(got[:3], ref[:3]):
        np.testing.assert_allclose(a, r, rtol=1e-12, atol=1e-12)
    assert got[3].all()


@pytest.mark.parametrize("g,nq", [(1, 200), (8, 37), (16, 20)])
def test_a_query_block_is_the_twins_problem_on_a_slice_of_q(g, nq):
    """Queries [q0, q0 + n) of a slice of L keys under the tail rule are the n tail queries of a slice of
    clamp(L - (nq - q0 - n), 0, L) keys; under the full rule, of L keys."""
    cap = 300
    lens = [0, 5, nq - 1, nq + 1, 230, cap]
    Q, K, V = _inputs(len(lens) * g, g, 8, 6, nq, cap, seed=g)
    pb, nqb = B.block_shape(g, nq)
    for tail in (False, True):
        whole = R.forward_f64(Q, K, V, lens, g, tail)
        for qb in range(nqb):
            q0, n = qb * pb, min(pb, nq - qb * pb)
            lb = [min(max(L - (nq - q0 - n), 0), L) if tail else L for L in lens]
            part = R.forward_f64(Q[:, :, q0:q0 + n], K, V, lb, g, tail)
            for a, r in zip(part, (whole[0][:, :, q0:q0 + n], whole[1][:, q0:q0 + n], whole[2][:, q0:q0 + n],
                                   whole[3][:, q0:q0 + n])):
                np.testing.assert_allclose(a, r, rtol=1e-12, atol=1e-12)


def test_the_reference_by_newest_key_is_the_tail_rule():
    g, nq, cap = 2, 37, 90
    lens = [0, 20, 37, 60, cap, cap + 4]
    Q, K, V = _inputs(len(lens) * g, g, 8, 6, nq, cap, seed=5)
    got = B.forward_khi_f64(Q, K, V, B.tail_khi(lens, g, Q.shape[0], nq, cap), g)
    for a, r in zip(got, R.forward_f64(Q, K, V, lens, g, True)):
        np.testing.assert_allclose(a, r, rtol=1e-12, atol=1e-12)


def test_block_shapes_and_beacon_queries():
    assert B.block_shape(1, 129) == (128, 2) and B.block_shape(8, 37) == (16, 3) and B.block_shape(16, 20) == (8, 3)
    assert B.block_shape(3, 40) == (32, 2) and B.block_shape(5, 40) == (16, 3) and B.block_shape(128, 2) == (1, 2)
    assert B.beacon_queries(8, 37) == [0, 15, 16, 31, 32, 36]
    assert B.beacon_queries(1, 129) == [0, 127, 128] and B.beacon_queries(128, 2) == [0, 1]


BEACON_SHAPES = [(8, 37, 32, 40), (16, 20, 64, 64), (1, 256, 32, 32)]


@pytest.mark.parametrize("g,nq,d,vd", BEACON_SHAPES)
def test_the_gate_refuses_a_key_bound_that_is_off_by_one(g, nq, d, vd):
    cap = nq + 40
    lens = [nq + 9]
    Q, K, V = _inputs(g, g, d, vd, nq, cap, seed=nq)
    Q, K, V, planted = B.plant(Q, K, V, lens, g)
    assert [q for _, q, _, _ in planted] == B.beacon_queries(g, nq)
    khi = B.tail_khi(lens, g, g, nq, cap)
    base = B.forward_khi_f64(Q, K, V, khi, g)
    # every beaconed query answers +A on its channels, and the unmoved reference rounded to fp16 passes the gate
    for s, q, pos, vch in planted:
        assert np.abs(base[0][:, vch, q] - B.A).max() < 1e-6
    rg._check_ref(B.as_outputs(base), Q, K, V, lens, g, True)
    pb, nqb = B.block_shape(g, nq)

    def refused(rows, delta):
        moved = khi.copy()
        for bi, i in rows:
            moved[bi, i] += delta
        part = B.forward_khi_f64(Q, K, V, moved, g, rows)
        mut = [x.copy() for x in base]
        for bi, i in rows:
            mut[0][bi, :, i], mut[1][bi, i], mut[2][bi, i], mut[3][bi, i] = part[0][bi, :, i], part[1][bi, i], part[2][bi, i], part[3][bi, i]
        with pytest.raises(AssertionError):
            rg._check_ref(B.as_outputs(mut), Q, K, V, lens, g, True)

    for delta in (-1, 1):
        for qb in range(nqb):  # one block's L_b
            refused([(bi, i) for bi in range(g) for i in range(qb * pb, min(nq, (qb + 1) * pb))], delta)
        for _, q, _, _ in planted:  # one beaconed query's newest key, in one head
            refused([(g - 1, q)], delta)
