"""CPU tests of the numpy reference of the fused K/V append (tests/append_ref.py): against the torch
recipe of the paged_1d docstring token by token, the paged reference against the ragged one through paged_ref.gather,
the clamps, and the float32 quotient of the FP8 encoding."""

import numpy as np
import pytest
import torch

from tests import append_ref, fp8_ref, paged_ref
from tf_flash_attention_amd import flash_attention as fa

HK, C, CV, PAGE, MAX_PAGES, NUM_PAGES = 2, 5, 3, 64, 3, 13


def _case(seed, n_new, k_lens, fp8):
    rng = np.random.default_rng(seed)
    S = len(k_lens)
    K_new = rng.uniform(-300, 300, (S, HK, C, n_new)).astype(np.float16)
    V_new = rng.uniform(-3, 3, (S, HK, CV, n_new)).astype(np.float16)
    table = rng.permutation(NUM_PAGES)[:S * MAX_PAGES].reshape(S, MAX_PAGES).astype(np.int32)
    if fp8:
        K_pool = rng.integers(0, 127, (NUM_PAGES, HK, C, PAGE)).astype(np.uint8)
        V_pool = rng.integers(0, 127, (NUM_PAGES, HK, CV, PAGE)).astype(np.uint8)
        ks, vs = np.array([0.7, 1.9], np.float32), np.array([0.013, 0.0071], np.float32)
    else:
        K_pool = rng.uniform(-1, 1, (NUM_PAGES, HK, C, PAGE)).astype(np.float16)
        V_pool = rng.uniform(-1, 1, (NUM_PAGES, HK, CV, PAGE)).astype(np.float16)
        ks = vs = None
    return K_new, V_new, K_pool, V_pool, table, np.asarray(k_lens, np.int32), ks, vs


def _recipe(pool, new, table, k_lens, new_lens, scale):
    """The paged_1d docstring's recipe, one token at a time, on CPU tensors."""
    fp8 = pool.dtype == np.uint8
    pool_t, table_t = torch.from_numpy(pool.copy()), torch.from_numpy(table).long()
    page, n_new = pool.shape[-1], new.shape[-1]
    for s, (L, n) in enumerate(append_ref.runs(k_lens, new_lens, n_new, table.shape[1] * page)):
        for t in range(n):
            pos = torch.tensor(L - n + t)
            tok = torch.from_numpy(new[s, :, :, n_new - n + t].copy())
            if fp8:
                tok8, _ = fa.quantize_kv_fp8(tok, head_axis=0, scale=torch.from_numpy(scale))
                tok = tok8.view(torch.uint8)
            pool_t[table_t[s, pos // page], :, :, pos % page] = tok
    return pool_t.numpy()


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("n_new,k_lens,new_lens", [
    (1, [1, 64, 65, 192], None),
    (9, [9, 70, 130, 192], None),
    (70, [70, 100, 192], [70, 1, 33]),
    (5, [3, 0, 64], [5, 2, 0]),
])
def test_reference_is_the_docstring_recipe_token_by_token(fp8, n_new, k_lens, new_lens):
    K_new, V_new, K_pool, V_pool, table, kl, ks, vs = _case(1, n_new, k_lens, fp8)
    nl = None if new_lens is None else np.asarray(new_lens, np.int32)
    Kr, Vr = append_ref.paged(K_pool, V_pool, K_new, V_new, table, kl, nl, ks, vs)
    np.testing.assert_array_equal(Kr, _recipe(K_pool, K_new, table, kl, nl, ks))
    np.testing.assert_array_equal(Vr, _recipe(V_pool, V_new, table, kl, nl, vs))
    assert not np.array_equal(Kr, K_pool)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_gathered_paged_reference_is_the_ragged_reference(fp8):
    K_new, V_new, K_pool, V_pool, table, kl, ks, vs = _case(2, 70, [70, 150, 192], fp8)
    nl = np.array([70, 3, 64], np.int32)
    Kp, Vp = append_ref.paged(K_pool, V_pool, K_new, V_new, table, kl, nl, ks, vs)
    g = lambda pool: paged_ref.gather(pool, table, PAGE).reshape(len(kl), HK, -1, MAX_PAGES * PAGE)  # noqa: E731
    Kr, Vr = append_ref.ragged(g(K_pool), g(V_pool), K_new, V_new, kl, nl, ks, vs)
    np.testing.assert_array_equal(g(Kp), Kr)
    np.testing.assert_array_equal(g(Vp), Vr)


def test_clamps_and_more_slots_than_keys():
    nk, n_new = 20, 6
    cases = [  # k_lens, new_lens -> (L, n)
        (0, None, (0, 0)), (-5, None, (0, 0)), (99, None, (20, 6)), (2 ** 31 - 1, 3, (20, 3)), (-2 ** 31, 3, (0, 0)),
        (4, None, (4, 4)),                     # n_new > L: the first slots lie before position 0
        (10, 0, (10, 0)), (10, 1, (10, 1)), (10, 6, (10, 6)), (10, 7, (10, 6)), (10, -1, (10, 0)), (3, 5, (3, 3)),
        (10, 2 ** 31 - 1, (10, 6)), (10, -2 ** 31, (10, 0)),
    ]
    for kl, nl, want in cases:
        got = append_ref.runs(np.array([kl], np.int64), None if nl is None else np.array([nl], np.int64), n_new, nk)
        assert got == [want], (kl, nl, got)
    rng = np.random.default_rng(3)
    new = rng.uniform(-1, 1, (1, 1, 2, n_new)).astype(np.float16)
    cache = np.zeros((1, 1, 2, nk), np.float16)
    out = append_ref.ragged_one(cache, new, np.array([4], np.int32))
    np.testing.assert_array_equal(out[..., :4], new[..., 2:])     # right-aligned: the LAST 4 slots
    assert not out[..., 4:].any()
    out = append_ref.ragged_one(cache, new, np.array([10], np.int32), np.array([2], np.int32))
    np.testing.assert_array_equal(out[..., 8:10], new[..., 4:])
    assert not out[..., :8].any() and not out[..., 10:].any()


def test_written_masks_cover_exactly_what_changes():
    K_new, V_new, K_pool, V_pool, table, kl, _, _ = _case(4, 9, [9, 70, 130], False)
    nl = np.array([9, 4, 0], np.int32)
    K_pool[:] = 7
    Kp = append_ref.paged_one(K_pool, K_new, table, kl, nl)
    m = append_ref.written_paged(K_pool.shape, 9, table, kl, nl)
    assert m.sum() == (9 + 4) * HK * C
    np.testing.assert_array_equal(Kp[~m], K_pool[~m])
    assert (Kp[m] != 7).all()
    cache = np.full((3, HK, C, 192), 7, np.float16)
    Kr = append_ref.ragged_one(cache, K_new, kl, nl)
    m = append_ref.written_ragged(cache.shape, 9, kl, nl)
    assert m.sum() == (9 + 4) * HK * C and (Kr[m] != 7).all() and (Kr[~m] == 7).all()


def test_the_fp8_reference_divides_in_float32():
    """Every float16 bit pattern that is not NaN, against quantize_kv_fp8 on CPU tensors: encode of numpy's float32
    quotient is the recipe bit for bit; the float64 quotient of fp8_ref.quantize is not (double rounding)."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = bits.view(np.float16)
    x = x[~np.isnan(x)]
    scales = np.array([0.013, 1.0, 2.0 ** -3, 0.7, 3.3], np.float32)
    X = np.broadcast_to(x, (len(scales), len(x))).copy()
    ref = append_ref.convert(X, np.uint8, scales)
    got, _ = fa.quantize_kv_fp8(torch.from_numpy(X), head_axis=0, scale=torch.from_numpy(scales))
    np.testing.assert_array_equal(ref, got.view(torch.uint8).numpy())
    fin = np.isfinite(X)
    f64 = fp8_ref.quantize(np.where(fin, X, 0), scales, 0)
    assert 0 < (f64 != ref)[fin].sum() < 100
    # null scales are 1.0
    np.testing.assert_array_equal(append_ref.convert(X[:1], np.uint8), append_ref.convert(X[:1], np.uint8, scales[1:2]))
