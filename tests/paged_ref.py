"""Float64 reference of the paged few-query forward (include/fa_api.h, "Paged few-query forward"): ``gather``
rebuilds the padded cache that the block table describes, and the reference is tests/ragged_ref.forward_f64 on it.
Test infrastructure only."""

import numpy as np

from tests import ragged_ref


def gather(pool, table, page):
    """pool [num_pages, Hk, C, page], table [sequences, max_pages] -> the padded cache [sequences * Hk, C,
    max_pages * page]: keys [p * page, (p + 1) * page) of every head of sequence s are pool[table[s, p]]."""
    pool, table = np.asarray(pool), np.asarray(table)
    num_pages, hk, c, pg = pool.shape
    assert pg == page and table.ndim == 2
    seqs, max_pages = table.shape
    out = np.empty((seqs * hk, c, max_pages * page), pool.dtype)
    for s in range(seqs):
        for p in range(max_pages):
            out[s * hk:(s + 1) * hk, :, p * page:(p + 1) * page] = pool[table[s, p]]
    return out


def forward_f64(Q, K_pool, V_pool, table, lens, page, g=1, tail_causal=False):
    """Q [sequences * Hk * g, d, nq]; ``lens`` one length per SEQUENCE.  Returns ragged_ref.forward_f64's tuple.
    Every table entry is gathered, so the entries of dead pages must be valid pages here."""
    hk = np.asarray(K_pool).shape[1]
    return ragged_ref.forward_f64(Q, gather(K_pool, table, page), gather(V_pool, table, page),
                                  np.repeat(np.asarray(lens), hk), g, tail_causal)
