"""CPU tests of tests/paged_ref.py, the reference of the paged forward."""

import numpy as np

from tests import paged_ref
from tests import ragged_ref


def test_gather_of_a_hand_built_example():
    """2 sequences, Hk = 2, C = 1, page = 2, max_pages = 2, 5 pool pages whose elements spell their own address
    1000 * page + 100 * head + key-in-page."""
    page, hk = 2, 2
    pool = np.zeros((5, hk, 1, page), np.float16)
    for n in range(5):
        for h in range(hk):
            for j in range(page):
                pool[n, h, 0, j] = 1000 * n + 100 * h + j
    table = np.array([[3, 0], [4, 3]], np.int32)  # (page 3 is shared)
    got = paged_ref.gather(pool, table, page)
    want = np.array([
        [[3000, 3001, 0, 1]],          # sequence 0, head 0: pages 3, 0
        [[3100, 3101, 100, 101]],      # sequence 0, head 1
        [[4000, 4001, 3000, 3001]],    # sequence 1, head 0: pages 4, 3
        [[4100, 4101, 3100, 3101]],    # sequence 1, head 1
    ], np.float16)
    assert got.shape == (4, 1, 4) and got.dtype == np.float16
    assert np.array_equal(got, want)


def _inputs(seed, seqs=3, hk=2, g=2, d=8, vd=5, nq=3, page=4, max_pages=3, num_pages=12):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    table = rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    return mk(seqs * hk * g, d, nq), mk(num_pages, hk, d, page), mk(num_pages, hk, vd, page), table


def test_a_permuted_table_with_the_pool_permuted_to_match_is_the_same_reference():
    page, g = 4, 2
    Q, Kp, Vp, table = _inputs(1)
    lens = [12, 5, 0]
    perm = np.random.default_rng(2).permutation(Kp.shape[0])  # new page perm[n] holds what page n held
    Kp2, Vp2 = np.empty_like(Kp), np.empty_like(Vp)
    Kp2[perm], Vp2[perm] = Kp, Vp
    table2 = perm[table].astype(np.int32)
    assert not np.array_equal(table, table2)
    for tail in (False, True):
        a = paged_ref.forward_f64(Q, Kp, Vp, table, lens, page, g, tail)
        b = paged_ref.forward_f64(Q, Kp2, Vp2, table2, lens, page, g, tail)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert a[3].any() and not a[3].all()


def test_the_reference_is_the_ragged_one_on_an_in_order_pool():
    """Pages laid out in order are the padded cache itself."""
    page, g, hk, seqs, max_pages = 4, 2, 2, 3, 3
    Q, Kp, Vp, _ = _inputs(3, num_pages=seqs * max_pages)
    table = np.arange(seqs * max_pages, dtype=np.int32).reshape(seqs, max_pages)
    # [seq, page, head, c, key] -> [seq, head, c, page, key]
    pad = lambda P: P.reshape(seqs, max_pages, hk, P.shape[2], page).transpose(0, 2, 3, 1, 4).reshape(  # noqa: E731
        seqs * hk, P.shape[2], max_pages * page)
    lens = [7, 12, 1]
    a = paged_ref.forward_f64(Q, Kp, Vp, table, lens, page, g, True)
    b = ragged_ref.forward_f64(Q, pad(Kp), pad(Vp), np.repeat(lens, hk), g, True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
