"""CPU tests of tests/ragged_ref.py, the float64 reference of the ragged forward, against the oracle:
the full form is oracle.forward_f64 on K / V truncated to the length; the tail-causal form is the float64
merge, by the formula include/fa_api.h documents for fa_merge_partials, of `full` over the first L - nq keys
and `causal` / `none_front` over the last nq keys."""

import numpy as np
import pytest

from oracle import fa_oracle as O
from tests import ragged_ref as R

D, VD, CAP = 8, 6, 40


def _inputs(b, g, nq, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(b, D, nq), mk(b // g, D, CAP), mk(b // g, VD, CAP)


def _merge(parts):
    """fa_merge_partials' formula in float64 over (O [vd, nq], L [nq], M [nq], has_any [nq]) parts."""
    nq = parts[0][1].shape[0]
    ha = np.zeros(nq, bool)
    m = np.full(nq, -np.inf)
    for _, _, Mi, hi in parts:
        ha |= hi
        m = np.where(hi, np.maximum(m, Mi), m)
    L = np.zeros(nq)
    for _, Li, Mi, hi in parts:
        L += np.where(hi, Li * np.exp(np.where(hi, Mi - m, 0.0)), 0.0)
    Oo = np.zeros_like(parts[0][0])
    for Oi, Li, Mi, hi in parts:
        w = np.where(hi, Li * np.exp(np.where(hi, Mi - m, 0.0)) / np.where(ha, L, 1.0), 0.0)
        Oo += Oi * w[None, :]
    return Oo, np.where(ha, L, 0.0), np.where(ha, m, 0.0), ha


def _oracle(policy, q, k, v):
    """One slice through oracle.forward_f64; an empty key set is the empty part."""
    nq = q.shape[1]
    if k.shape[1] == 0 or nq == 0:
        return np.zeros((v.shape[0], nq)), np.zeros(nq), np.zeros(nq), np.zeros(nq, bool)
    Oo, L, M, ha = O.forward_f64(q[None], k[None], v[None], O.Problem(policy, 1, "none_front"))
    return Oo[0], L[0], M[0], ha


@pytest.mark.parametrize("g,nq", [(1, 1), (1, 5), (3, 4)])
def test_full_form_is_the_oracle_on_truncated_keys(g, nq):
    lens = [0, 1, 17, CAP, CAP + 9, -4]
    Q, K, V = _inputs(len(lens) * g, g, nq, seed=nq)
    got = R.forward_f64(Q, K, V, lens, g, tail_causal=False)
    for bi in range(Q.shape[0]):
        L = min(max(lens[bi // g], 0), CAP)
        ref = _oracle("full", Q[bi], K[bi // g][:, :L], V[bi // g][:, :L])
        for a, r in zip(got, ref):
            np.testing.assert_allclose(a[bi], r, rtol=1e-12, atol=1e-12)
        assert got[3][bi].all() == (L > 0)


@pytest.mark.parametrize("g,nq", [(1, 1), (1, 5), (2, 7)])
def test_tail_causal_form_is_the_merge_of_two_oracle_calls(g, nq):
    lens = [0, 1, nq - 1, nq, nq + 1, 23, CAP]
    Q, K, V = _inputs(len(lens) * g, g, nq, seed=10 + nq)
    got = R.forward_f64(Q, K, V, lens, g, tail_causal=True)
    for bi in range(Q.shape[0]):
        L = lens[bi // g]
        k, v = K[bi // g][:, :L], V[bi // g][:, :L]
        n_tail = min(nq, L)  # the queries that have a position in the sequence: the last n_tail
        head = _oracle("full", Q[bi], k[:, :L - n_tail], v[:, :L - n_tail])
        t = _oracle("causal", Q[bi][:, nq - n_tail:], k[:, L - n_tail:], v[:, L - n_tail:])
        pad = nq - n_tail  # queries before the sequence's first position see nothing
        tail = (np.concatenate([np.zeros((VD, pad)), t[0]], axis=1), np.concatenate([np.zeros(pad), t[1]]),
                np.concatenate([np.zeros(pad), t[2]]), np.concatenate([np.zeros(pad, bool), t[3]]))
        ref = _merge([head, tail])
        for a, r in zip(got, ref):
            np.testing.assert_allclose(a[bi], r, rtol=1e-12, atol=1e-12)
        assert (got[3][bi] == (np.arange(nq) >= nq - L)).all()


def test_one_query_under_the_tail_rule_is_the_full_form():
    lens = [0, 3, CAP]
    Q, K, V = _inputs(3, 1, 1, seed=3)
    for a, b in zip(R.forward_f64(Q, K, V, lens, 1, True), R.forward_f64(Q, K, V, lens, 1, False)):
        assert np.array_equal(a, b)


def test_keys_past_the_length_are_not_read():
    lens = [5, 0]
    Q, K, V = _inputs(2, 1, 3, seed=4)
    ref = R.forward_f64(Q, K, V, lens)
    K2, V2 = K.copy(), V.copy()
    K2[0, :, 5:], V2[0, :, 5:], K2[1], V2[1] = np.nan, np.inf, np.nan, np.nan
    for a, b in zip(R.forward_f64(Q, K2, V2, lens), ref):
        assert np.array_equal(a, b)
