"""Numpy reference of the fused K/V append (include/fa_api.h, "Fused K/V append").  Test
infrastructure only.

Sequence s holds L = clamp(k_lens[s], 0, nk) keys after the append; its last n = min(clamp(new_lens[s], 0, n_new), L)
positions (new_lens None: min(n_new, L)) take the LAST n of the n_new slots: slot n_new - n + t goes to position
L - n + t.  Every function works on COPIES of the cache and returns them.  An fp16 cache (float16 arrays) takes a bit
copy; an FP8 cache (uint8 arrays of e4m3fn bytes) takes fp8_ref.encode of the FLOAT32 quotient float32(x) / scale[h]:
numpy divides float32 by float32 in float32, correctly rounded, which is what the kernel and the torch recipe of
quantize_kv_fp8 do.  fp8_ref.quantize divides in float64, and the second rounding moves a few codes.

Layouts, the batch flattened to one axis: K_new [S, Hk, C, n_new]; ragged cache [S, Hk, C, nk]; pools
[num_pages, Hk, C, page] with table [S, max_pages], every entry that is used clamped to [0, num_pages - 1]."""

import numpy as np

from tests import fp8_ref


def runs(k_lens, new_lens, n_new, nk):
    """[(L, n)] per sequence, after the clamps."""
    out = []
    for s, kl in enumerate(np.asarray(k_lens).reshape(-1)):
        L = min(max(int(kl), 0), nk)
        n = n_new if new_lens is None else min(max(int(np.asarray(new_lens).reshape(-1)[s]), 0), n_new)
        out.append((L, min(n, L)))
    return out


def convert(x, cache_dtype, scale=None):
    """float16 tokens [Hk, C, ...] -> the cache's elements; ``scale`` [Hk] float32 or None (1.0), FP8 only."""
    x = np.asarray(x)
    assert x.dtype == np.float16
    if np.dtype(cache_dtype) == np.float16:
        assert scale is None
        return x
    assert np.dtype(cache_dtype) == np.uint8
    sc = np.ones(x.shape[0], np.float32) if scale is None else np.asarray(scale, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = x.astype(np.float32) / sc.reshape((-1,) + (1,) * (x.ndim - 1))
    assert q.dtype == np.float32
    return fp8_ref.encode(q)


def ragged_one(cache, new, k_lens, new_lens=None, scale=None):
    """One tensor (K or V): cache [S, Hk, C, nk], new [S, Hk, C, n_new] -> the appended copy."""
    out = np.array(cache, copy=True)
    n_new, nk = new.shape[-1], cache.shape[-1]
    for s, (L, n) in enumerate(runs(k_lens, new_lens, n_new, nk)):
        if n:
            out[s, :, :, L - n:L] = convert(new[s, :, :, n_new - n:], cache.dtype, scale)
    return out


def ragged(K, V, K_new, V_new, k_lens, new_lens=None, k_scale=None, v_scale=None):
    return ragged_one(K, K_new, k_lens, new_lens, k_scale), ragged_one(V, V_new, k_lens, new_lens, v_scale)


def written_ragged(cache_shape, n_new, k_lens, new_lens=None):
    """Boolean mask of the cache elements a call may touch."""
    m = np.zeros(cache_shape, bool)
    for s, (L, n) in enumerate(runs(k_lens, new_lens, n_new, cache_shape[-1])):
        m[s, :, :, L - n:L] = True
    return m


def _places(table, page, num_pages, L, n):
    """(pool page, offset) of positions L - n .. L - 1 of one sequence's table row."""
    pos = np.arange(L - n, L)
    return np.clip(np.asarray(table)[pos // page].astype(np.int64), 0, num_pages - 1), pos % page


def paged_one(pool, new, table, k_lens, new_lens=None, scale=None):
    """One pool: pool [num_pages, Hk, C, page], new [S, Hk, C, n_new], table [S, max_pages] -> the appended copy.
    Sequences are written in order (two that name one page at a written position race in the kernel)."""
    out = np.array(pool, copy=True)
    num_pages, page, n_new = pool.shape[0], pool.shape[-1], new.shape[-1]
    table = np.asarray(table)
    table = table.reshape(new.shape[0], table.shape[-1])
    for s, (L, n) in enumerate(runs(k_lens, new_lens, n_new, table.shape[1] * page)):
        if n:
            pg, off = _places(table[s], page, num_pages, L, n)
            out[pg, :, :, off] = np.moveaxis(convert(new[s, :, :, n_new - n:], pool.dtype, scale), -1, 0)
    return out


def paged(K_pool, V_pool, K_new, V_new, table, k_lens, new_lens=None, k_scale=None, v_scale=None):
    return (paged_one(K_pool, K_new, table, k_lens, new_lens, k_scale),
            paged_one(V_pool, V_new, table, k_lens, new_lens, v_scale))


def written_paged(pool_shape, n_new, table, k_lens, new_lens=None):
    m = np.zeros(pool_shape, bool)
    table = np.asarray(table)
    table = table.reshape(-1, table.shape[-1])
    for s, (L, n) in enumerate(runs(k_lens, new_lens, n_new, table.shape[1] * pool_shape[-1])):
        if n:
            pg, off = _places(table[s], pool_shape[-1], pool_shape[0], L, n)
            m[pg, :, :, off] = True
    return m
