"""GPU tests of the tree-masked draft forwards (include/fa_api.h, "Tree-masked draft attention")
over the four K/V caches: parity against tests/tree_ref.py under the fp16 forward gate of the twins, the four bitwise
guarantees, poison past the lengths and in pages that are not live, corrupt table entries, the merge with a second
call, graph replay, and a seeded sweep.

Shapes are the smallest at which the form can go wrong: capacities of 1536 keys (chunks of 512 where the folded rows
are <= 64) and 2112 keys (chunks of 1024 above), so every case has at least two key chunks, which each test asserts;
lengths around 0, nq, a tile, a chunk and the capacity, with the draft straddling a tile and a chunk boundary, mixed
in one batch; W from 1 to 4 words and the pitch below 8, at 32 and above 32."""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import fp8_ref, gate, paged_ref, ragged_ref, tree_ref
from tests import test_gpu_parity as parity
from tests import test_gpu_ragged as rg
from tests.gate import TOL
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

HK = 2
CACHES = [("ragged", False), ("paged", False), ("ragged", True), ("paged", True)]
CACHE_IDS = ["ragged", "paged", "ragged_fp8", "paged_fp8"]
SHAPES = [(1, 1), (1, 5), (1, 33), (1, 64), (1, 128), (4, 16), (8, 7), (8, 16)]  # (g, nq)
KINDS = ("forest", "random", "zero_rows")
K_SCALE = [0.037, 2.0 ** -12 * 1.37]  # (tests/test_gpu_fp8_cache.py: e inside the clamp, and at its lower end)
V_SCALE = [300.0, 0.0123]
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _rows(g, nq):
    return g * (1 << max(nq - 1, 0).bit_length())


def _capacity(g, nq, fast=True, cache="ragged"):
    cap = 1536 if _rows(g, nq) <= 64 else 2112
    return cap if fast or cache == "paged" else cap - 5  # 1531: rows that are not 16-byte aligned


def _chunk(g, nq):
    return 512 if _rows(g, nq) <= 64 else 1024


def _lengths(g, nq, cap):
    c = _chunk(g, nq)
    return [0, 1, nq - 1, nq, nq + 1, 63, 64, 65, c - 1, c, c + 1, c + nq // 2, 64 * 5 + nq // 2, cap]


def _problem(nq, cap, d, vd, b):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, vd)


def _masks(kinds, nq, rng):
    """uint32 [len(kinds), nq, W], the unused bits of the last word set to ones."""
    out = []
    for kind in kinds:
        if kind == "forest":
            bits = tree_ref.ancestors(np.array([rng.integers(-1, i) for i in range(nq)]))
        else:
            bits = rng.random((nq, nq)) < 0.5
            if kind == "zero_rows":
                bits[rng.random(nq) < 0.4] = False
                bits[rng.integers(nq)] = False
        out.append(tree_ref.pack_mask(bits))
    return tree_ref.set_unused_bits(np.stack(out), nq)


def _pools(cache, table, page, num_pages, fill):
    """The padded cache [seqs * HK, c, cap] as a pool [num_pages, HK, c, page] through ``table``; pages that the
    table does not name hold ``fill``."""
    seqs, max_pages = table.shape
    c = cache.shape[1]
    pool = np.full((num_pages, HK, c, page), fill, cache.dtype)
    pool[table] = cache.reshape(seqs, HK, c, max_pages, page).transpose(0, 3, 1, 2, 4)
    return pool


def _table(seqs, max_pages, rng, spare=5):
    num_pages = seqs * max_pages + spare
    return rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32), num_pages


def _inputs(seqs, g, nq, d, vd, cap, seed, fp8):
    """Q, and K / V as the cache stores them (fp16, or e4m3fn bytes of K, V ~ U(-2, 2) under the per-head scales) and
    as the reference reads them (the same fp16 values, or the dequantized float64 ones)."""
    Q, K, V = rg._np_inputs(seqs * HK, g, d, vd, nq, cap, seed)
    if not fp8:
        return Q, K, V, K, V
    byhead = lambda x: x.reshape(seqs, HK, x.shape[1], cap)  # noqa: E731
    K8 = fp8_ref.quantize(byhead(K), K_SCALE, 1).reshape(K.shape)
    V8 = fp8_ref.quantize(byhead(V), V_SCALE, 1).reshape(V.shape)
    return (Q, K8, V8, fp8_ref.dequantize(byhead(K8), K_SCALE, 1).reshape(K.shape),
            fp8_ref.dequantize(byhead(V8), V_SCALE, 1).reshape(V.shape))


def _dev(x):
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")  # (a copy: the kept batches are read-only)


def _scales(fp8, unit=False):
    if not fp8 or unit:
        return None, None
    return _dev(np.asarray(K_SCALE, np.float32)), _dev(np.asarray(V_SCALE, np.float32))


def _run(cache, fp8, g, Q, K, V, lens, masks=None, table=None, scales=(None, None), tail=1, fill=None, ws_fill=None,
         ws_short=0):
    """The C entry point of (cache, fp8) on device tensors: the tree form with ``masks`` (a device int32 tensor
    [seqs, nq, W]), else the plain twin with ``tail``.  K, V: the padded cache, or the pools with ``table``.  Returns
    (status, O, l, m)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    if cache == "paged":
        num_pages, _, vd, page = V.shape
        max_pages = table.shape[-1]
        cap, own = max_pages * page, (g, page)
    else:
        vd, cap = V.shape[1], V.shape[2]
        own = (g,)
    prob = _problem(nq, cap, d, vd, b)
    _, ws_name, forward = _lib.decode_entry_points(cache, "plain" if masks is None else "tree", fp8)
    need = int(getattr(L, ws_name)(prob, *own))
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O_, l, m):
            t.view(torch.uint8).fill_(fill)
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = [torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr()]
    args += [ptr(scales[0]), ptr(scales[1])] if fp8 else []
    args += [table.data_ptr(), max_pages, page, num_pages] if cache == "paged" else []
    args += [lens.data_ptr(), HK, int(tail) if masks is None else masks.data_ptr(), O_.data_ptr(), l.data_ptr(),
             m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0)]
    st = getattr(L, forward)(*args)
    torch.cuda.synchronize()
    return st, O_, l, m


def _two_chunks(cache, g, nq, d, vd, cap, page):
    out = (ctypes.c_int32 * 6)()
    own = (g, page) if cache == "paged" else (g,)
    assert getattr(_lib.lib(), f"fa_forward_{cache}_tree_plan")(_problem(nq, cap, d, vd, g), *own, out) == 0
    assert out[0] >= 2 and out[1] == _chunk(g, nq), tuple(out)


def _check_tree(got, Q, K, V, kv_lens, masks, g):
    """tests/test_gpu_ragged._check_ref with tests/tree_ref.py as the reference: O and l within TOL[float16]['fwd']
    (l relative to the stored m), m within 2 ulp plus the larger of 1e-3 * max(|m|, 1) and
    (2^-11 + d 2^-24) * max_j sum_c |q_c k_jc| / sqrt(d) + 4.9e-4, the maximum taken over the keys the row SEES.
    Returns the worst |error| / allowance of O, l and m."""
    O64, L64, M64, ha = tree_ref.forward_f64(Q, K, V, kv_lens, masks, g, HK)
    o, l, m = (t.cpu().numpy() for t in got)
    b, d, nq = Q.shape
    cap = K.shape[2]
    rtol, atol = TOL[np.float16]["fwd"]
    rg._check_empty(got, ~ha)
    live = ha[:, None, :] & np.ones_like(O64, bool)
    print("O max err / scale", parity._close("O", np.where(live, o, 0.0), O64, rtol, atol))
    assert np.isfinite(o.astype(np.float64)).all()
    res = {"O": float((np.abs(np.where(live, o, 0.0) - O64) / gate.plain_bound(O64, rtol, atol)).max())}
    if not ha.any():
        return res
    m_f, M = m.astype(np.float64)[ha], M64[ha]
    rowdot = np.zeros((b, nq))
    for bi in range(b):
        mask = tree_ref.tree_mask(nq, cap, kv_lens[bi // g], masks[bi // g // HK])
        rowdot[bi] = gate.max_abs_dot(Q[bi][None], K[bi // g][None], mask)[0] / math.sqrt(d)
    ulp = np.abs(np.spacing(np.abs(M).astype(np.float16))).astype(np.float64)
    m_tol = 2 * ulp + np.maximum(1e-3 * np.maximum(np.abs(M), 1.0), (2.0 ** -11 + d * 2.0 ** -24) * rowdot[ha] + 4.9e-4)
    res["m"] = float((np.abs(m_f - M) / m_tol).max())
    print("m worst err / allowance", res["m"])
    assert (np.abs(m_f - M) <= m_tol).all(), f"m: max err {np.abs(m_f - M).max():.3e}"
    l_ref = L64[ha] * np.exp(M - m_f)
    parity._close("l", l.astype(np.float64)[ha], l_ref, max(rtol, 1e-6), atol)
    res["l"] = float((np.abs(l.astype(np.float64)[ha] - l_ref) / gate.plain_bound(l_ref, max(rtol, 1e-6), atol)).max())
    return res


@functools.lru_cache(maxsize=None)
def _batch(g, nq, d, vd, fast, cache, fp8):
    """One batch of a shape: every length of _lengths in it, the mask kinds in turn.  Kept: the tests of a shape share
    it, and nothing writes to it."""
    cap = _capacity(g, nq, fast, cache)
    lens = _lengths(g, nq, cap)
    seqs = len(lens)
    rng = np.random.default_rng(1000 * g + nq + d)
    Q, K, V, Kref, Vref = _inputs(seqs, g, nq, d, vd, cap, 7 * g + nq + d, fp8)
    masks = _masks([KINDS[(s + nq + d) % 3] for s in range(seqs)], nq, rng)
    for x in (Q, K, V, Kref, Vref, masks):
        x.setflags(write=False)
    return Q, K, V, Kref, Vref, np.array(lens), masks, cap


def _stored(cache, K, V, page, rng, fill):
    """(K, V, table) as device tensors: the padded caches, or pools behind a random table."""
    if cache == "ragged":
        return _dev(K), _dev(V), None, None
    seqs = K.shape[0] // HK
    table, num_pages = _table(seqs, K.shape[2] // page, rng)
    return _dev(_pools(K, table, page, num_pages, fill)), _dev(_pools(V, table, page, num_pages, fill)), _dev(table), table


def _fill(fp8):
    return 0x7F if fp8 else np.nan  # what a page that no sequence owns holds: NaN either way


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("g,nq", SHAPES)
def test_parity_with_the_float64_reference(cache, fp8, d, g, nq):
    page = 64 if (g + nq) % 2 else 192
    Q, K, V, Kref, Vref, lens, masks, cap = _batch(g, nq, d, d, True, cache, fp8)
    _two_chunks(cache, g, nq, d, d, cap, page)
    tk, tv, tt, _ = _stored(cache, K, V, page, np.random.default_rng(nq), _fill(fp8))
    st, *got = _run(cache, fp8, g, _dev(Q), tk, tv, _dev(lens.astype(np.int32)), _dev(masks), tt, _scales(fp8), ws_fill=0xFF)
    assert st == 0, _lib.last_error()
    print(cache, fp8, d, g, nq, _check_tree(got, Q, Kref, Vref, np.repeat(lens, HK), masks, g))


@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("g,nq", [(1, 5), (4, 16)])
def test_parity_without_fast_staging(cache, fp8, g, nq):
    """d = 40, v_d = 72 (and a ragged capacity of 1531 keys): the element-wise staging."""
    d, vd = 40, 72
    Q, K, V, Kref, Vref, lens, masks, cap = _batch(g, nq, d, vd, False, cache, fp8)
    assert cap == (1536 if cache == "paged" else 1531)
    _two_chunks(cache, g, nq, d, vd, cap, 64)
    tk, tv, tt, _ = _stored(cache, K, V, 64, np.random.default_rng(nq), _fill(fp8))
    st, *got = _run(cache, fp8, g, _dev(Q), tk, tv, _dev(lens.astype(np.int32)), _dev(masks), tt, _scales(fp8), ws_fill=0xFF)
    assert st == 0, _lib.last_error()
    print(cache, fp8, g, nq, _check_tree(got, Q, Kref, Vref, np.repeat(lens, HK), masks, g))


# ------------------------------------------------------------------ the bitwise guarantees
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("g,nq,d", [(1, 33, 64), (8, 7, 128), (1, 128, 64)])
def test_a_slice_does_not_depend_on_the_batch_or_on_other_masks(cache, fp8, g, nq, d):
    """(a): each of three sequences alone is bitwise its rows of the batch, whose other sequences have other lengths
    and other masks; and the batch again with those others' masks and lengths changed."""
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, d, True, cache, fp8)
    _two_chunks(cache, g, nq, d, d, cap, 64)
    tk, tv, tt, _ = _stored(cache, K, V, 64, np.random.default_rng(3), _fill(fp8))
    tq, tl, tm, sc = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks), _scales(fp8)
    st, *whole = _run(cache, fp8, g, tq, tk, tv, tl, tm, tt, sc)
    assert st == 0
    for s in (3, 11, 13):  # lengths nq, c + nq / 2 and the capacity
        qs, ks = slice(s * HK * g, (s + 1) * HK * g), slice(s * HK, (s + 1) * HK)
        kv = (tk, tv) if cache == "paged" else (tk[ks].contiguous(), tv[ks].contiguous())
        st, *alone = _run(cache, fp8, g, tq[qs].contiguous(), *kv, tl[s:s + 1].contiguous(), tm[s:s + 1].contiguous(),
                          None if tt is None else tt[s:s + 1].contiguous(), sc)
        assert st == 0
        assert rg._same(alone, [t[qs] for t in whole]), s
        others = np.arange(len(lens)) != s
        lens2, masks2 = lens.copy(), masks.copy()
        lens2[others] = (lens2[others] * 7 + 5) % (cap + 1)
        masks2[others] ^= np.uint32(0xFFFFFFFF)
        st, *again = _run(cache, fp8, g, tq, tk, tv, _dev(lens2.astype(np.int32)), _dev(masks2), tt, sc)
        assert st == 0
        assert rg._same([t[qs] for t in again], alone), s


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("g,nq,d,page", [(4, 16, 64, 64), (1, 64, 128, 192), (1, 128, 64, 192), (1, 5, 40, 64)])
def test_the_paged_result_is_the_ragged_result_on_the_gathered_cache(fp8, g, nq, d, page):
    """(b): a shuffled table, with the first page of sequence 1 shared with sequence 0."""
    vd = 72 if d == 40 else d
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, vd, d != 40, "paged", fp8)
    K, V = K.copy(), V.copy()
    K[HK:2 * HK, :, :page] = K[:HK, :, :page]
    V[HK:2 * HK, :, :page] = V[:HK, :, :page]
    table, num_pages = _table(len(lens), cap // page, np.random.default_rng(5))
    Kp, Vp = _pools(K, table, page, num_pages, _fill(fp8)), _pools(V, table, page, num_pages, _fill(fp8))
    Kp[table[1, 0]] = Vp[table[1, 0]] = _fill(fp8)  # sequence 1's own copy is no longer named by any entry
    table[1, 0] = table[0, 0]
    assert (paged_ref.gather(Kp, table, page).view(np.uint8) == K.view(np.uint8)).all()
    lens = lens.copy()
    lens[:2] = [page + nq // 2, page + 1]  # both read the shared page
    tq, tl, tm, sc = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks), _scales(fp8)
    st0, *paged = _run("paged", fp8, g, tq, _dev(Kp), _dev(Vp), tl, tm, _dev(table), sc)
    st1, *ragged = _run("ragged", fp8, g, tq, _dev(K), _dev(V), tl, tm, None, sc)
    assert st0 == 0 and st1 == 0
    assert rg._same(paged, ragged)


@pytest.mark.parametrize("cache", ["ragged", "paged"])
@pytest.mark.parametrize("g,nq,d", [(4, 16, 64), (1, 33, 128), (1, 5, 40)])
def test_unit_scales_are_the_fp16_forward_on_the_converted_cache(cache, g, nq, d):
    """(c): null scales, and scales of 1.0."""
    vd = 72 if d == 40 else d
    Q, K8, V8, _, _, lens, masks, cap = _batch(g, nq, d, vd, d != 40, cache, True)
    K16, V16 = fp8_ref.decode(K8).astype(np.float16), fp8_ref.decode(V8).astype(np.float16)
    assert np.isfinite(K16).all() and np.isfinite(V16).all()
    tq, tl, tm = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks)
    tk8, tv8, tt, _ = _stored(cache, K8, V8, 64, np.random.default_rng(9), 0x7F)
    tk, tv, _, _ = _stored(cache, K16, V16, 64, np.random.default_rng(9), np.nan)
    st, *ref = _run(cache, False, g, tq, tk, tv, tl, tm, tt)
    assert st == 0
    one = _dev(np.ones(HK, np.float32))
    for sc in ((None, None), (one, one), (None, one)):
        st, *got = _run(cache, True, g, tq, tk8, tv8, tl, tm, tt, sc)
        assert st == 0
        assert rg._same(got, ref)


@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("g,nq,d", [(g, nq, 64 if i % 2 else 128) for i, (g, nq) in enumerate(SHAPES)] + [(4, 16, 40), (1, 33, 40)])
def test_the_lower_triangle_is_bitwise_the_tail_causal_twin(cache, fp8, g, nq, d):
    """(d): (O, l, m) of the chain mask, its unused bits ones, are the bits of the twin with tail_causal = 1."""
    vd = 72 if d == 40 else d
    Q, K, V, _, _, lens, _, cap = _batch(g, nq, d, vd, d != 40, cache, fp8)
    chain = tree_ref.set_unused_bits(np.broadcast_to(tree_ref.lower_triangle(nq), (len(lens), nq, tree_ref.mask_words(nq))), nq)
    tk, tv, tt, _ = _stored(cache, K, V, 64, np.random.default_rng(11), _fill(fp8))
    tq, tl, sc = _dev(Q), _dev(lens.astype(np.int32)), _scales(fp8)
    st0, *tree = _run(cache, fp8, g, tq, tk, tv, tl, _dev(chain), tt, sc, ws_fill=0xFF)
    st1, *twin = _run(cache, fp8, g, tq, tk, tv, tl, None, tt, sc, tail=1)
    assert st0 == 0 and st1 == 0
    assert rg._same(tree, twin)


# ------------------------------------------------------------------ poison and corrupt tables
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("g,nq,d", [(4, 16, 64), (1, 128, 128), (1, 5, 40)])
def test_values_at_and_past_the_length_and_pages_that_are_not_live_reach_no_output(cache, fp8, g, nq, d):
    """K and V at and past every length are NaN, Inf or the largest finite value (an FP8 cache: the NaN codes and
    +-448), the pool pages that no sequence owns NaN, the workspace 0xFF bytes: bitwise the call with zeros there."""
    vd = 72 if d == 40 else d
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, vd, d != 40, cache, fp8)
    past = np.arange(cap)[None, None, :] >= np.repeat(np.clip(lens, 0, cap), HK)[:, None, None]
    poisons = (0x7F, 0xFF, 0x7E, 0xFE) if fp8 else (np.nan, np.inf, -np.inf, 65504.0)
    put = lambda x, val: np.where(past, np.asarray(val, x.dtype), x)  # noqa: E731
    tq, tl, tm, sc = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks), _scales(fp8)
    tk, tv, tt, _ = _stored(cache, put(K, 0), put(V, 0), 64, np.random.default_rng(13), 0)
    st, *ref = _run(cache, fp8, g, tq, tk, tv, tl, tm, tt, sc)
    assert st == 0
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    for poison in poisons:
        tk, tv, tt, _ = _stored(cache, put(K, poison), put(V, poison), 64, np.random.default_rng(13), _fill(fp8))
        st, *got = _run(cache, fp8, g, tq, tk, tv, tl, tm, tt, sc, ws_fill=0xFF)
        assert st == 0
        assert rg._same(got, ref), f"poison {poison}"


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("page", [64, 192])
def test_a_corrupt_table_faults_nothing_and_changes_nothing_for_live_pages(fp8, page):
    """Entries of pages without a live key hold values far outside the pool: never loaded, the same bits.  A LIVE
    entry outside the pool is clamped to [0, num_pages - 1] before it forms an address: the bits of the call with
    the clamped entry."""
    g, nq, d = 4, 16, 64
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, d, True, "paged", fp8)
    table, num_pages = _table(len(lens), cap // page, np.random.default_rng(17))
    tk, tv = _dev(_pools(K, table, page, num_pages, 0)), _dev(_pools(V, table, page, num_pages, 0))  # (finite everywhere)
    tq, tl, tm, sc = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks), _scales(fp8)
    dead = np.arange(cap // page)[None, :] >= -(-np.clip(lens, 0, cap) // page)[:, None]
    assert dead.any() and not dead.all()
    st, *ref = _run("paged", fp8, g, tq, tk, tv, tl, tm, _dev(np.where(dead, 0, table).astype(np.int32)), sc)
    assert st == 0
    for junk in (INT32_MIN, -1, num_pages, INT32_MAX):
        st, *got = _run("paged", fp8, g, tq, tk, tv, tl, tm, _dev(np.where(dead, junk, table).astype(np.int32)), sc)
        assert st == 0
        assert rg._same(got, ref), junk
    live_bad, clamped = table.copy(), table.copy()
    live_bad[-1, 0], clamped[-1, 0] = INT32_MAX, num_pages - 1
    live_bad[-2, 1], clamped[-2, 1] = -7, 0
    assert not dead[-1, 0] and not dead[-2, 1]
    st0, *got = _run("paged", fp8, g, tq, tk, tv, tl, tm, _dev(live_bad), sc)
    st1, *want = _run("paged", fp8, g, tq, tk, tv, tl, tm, _dev(clamped), sc)
    assert st0 == 0 and st1 == 0
    assert rg._same(got, want)
    untouched = slice(0, (len(lens) - 2) * HK * g)  # the sequences whose live entries are intact
    assert rg._same([t[untouched] for t in got], [t[untouched] for t in ref])


# ------------------------------------------------------------------ the ABI's statuses on the device
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
def test_a_short_workspace_and_a_shape_outside_the_envelope_write_nothing(cache, fp8):
    g, nq, d = 4, 16, 64
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, d, True, cache, fp8)
    tk, tv, tt, _ = _stored(cache, K, V, 64, np.random.default_rng(19), _fill(fp8))
    tq, tl, tm = _dev(Q), _dev(lens.astype(np.int32)), _dev(masks)
    st, *out = _run(cache, fp8, g, tq, tk, tv, tl, tm, tt, ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert all(bool((t.view(torch.uint8) == 0x5A).all()) for t in out)
    # 64 queries of g = 4 heads are 256 folded rows
    wide = torch.zeros((Q.shape[0], d, 64), dtype=torch.float16, device=tq.device)
    st, *out = _run(cache, fp8, g, wide, tk, tv, tl, _dev(np.zeros((len(lens), 64, 2), np.uint32)), tt, fill=0x5A)
    assert st == _lib.FA_ERR_UNSUPPORTED and "envelope" in _lib.last_error()
    assert all(bool((t.view(torch.uint8) == 0x5A).all()) for t in out)


# ------------------------------------------------------------------ the merge with a second call
@pytest.mark.parametrize("cache", ["ragged", "paged"])
def test_a_tree_call_merges_with_a_second_call_to_the_reference_of_the_union(cache):
    """The tree call over the sequence's cache and a plain ragged call over a second key set (a prefix shared by the
    batch, every key seen), joined by merge_partials: the float64 attention over the union of the two key sets."""
    g, nq, d = 4, 16, 64
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, d, True, cache, False)
    seqs, cap2 = len(lens), 192
    rng = np.random.default_rng(23)
    K2 = rng.uniform(-2, 2, (seqs * HK, d, cap2)).astype(np.float16)
    V2 = rng.uniform(-2, 2, (seqs * HK, d, cap2)).astype(np.float16)
    lens2 = np.array([(37 * s) % (cap2 + 1) for s in range(seqs)])
    lens2[0] = lens2[5] = 0  # with length 0 in the tree call too: rows without a key in either part; and in one part
    assert lens[0] == 0 and lens[5] > 0
    tq = _dev(Q).reshape(seqs, HK * g, d, nq)
    tm, tl = _dev(masks), _dev(lens.astype(np.int32))
    if cache == "ragged":
        one = fa.ragged_1d(tq, _dev(K).reshape(seqs, HK, d, cap), _dev(V).reshape(seqs, HK, d, cap), tl, tail_causal=True,
                           returning_l_m=True, draft_mask=tm)
    else:
        tk, tv, tt, _ = _stored(cache, K, V, 64, rng, np.nan)
        one = fa.paged_1d(tq, tk, tv, tt, tl, tail_causal=True, returning_l_m=True, draft_mask=tm)
    two = fa.ragged_1d(tq, _dev(K2).reshape(seqs, HK, d, cap2), _dev(V2).reshape(seqs, HK, d, cap2),
                       _dev(lens2.astype(np.int32)), returning_l_m=True)
    O_, l, m = fa.merge_partials([one[0], two[0]], [one[1], two[1]], [one[2], two[2]])
    torch.cuda.synchronize()
    # the union in float64: the parts' exact statistics joined
    O1, L1, M1, h1 = tree_ref.forward_f64(Q, K, V, np.repeat(lens, HK), masks, g, HK)
    O2, L2, M2, h2 = ragged_ref.forward_f64(Q, K2, V2, np.repeat(lens2, HK), g)
    ha = h1 | h2
    M = np.where(h1 & h2, np.maximum(M1, M2), np.where(h1, M1, M2))
    w1, w2 = np.where(h1, L1 * np.exp(M1 - M), 0.0), np.where(h2, L2 * np.exp(M2 - M), 0.0)
    Lu = w1 + w2
    Ou = (O1 * w1[:, None, :] + O2 * w2[:, None, :]) / np.where(ha, Lu, 1.0)[:, None, :]
    got = [t.reshape((-1,) + t.shape[2:]) for t in (O_, l, m)]
    assert (~ha).any() and (h1 & ~h2).any() and (h2 & ~h1).any() and (h1 & h2).any()
    rg._check_empty(got, ~ha)
    rtol, atol = TOL[np.float16]["fwd"]
    o = got[0].cpu().numpy()
    print("O max err / scale", parity._close("O", np.where(ha[:, None, :], o, 0.0), Ou, rtol, atol))
    m_f = got[2].cpu().numpy().astype(np.float64)[ha]
    l_ref = Lu[ha] * np.exp(M[ha] - m_f)
    parity._close("l", got[1].cpu().numpy().astype(np.float64)[ha], l_ref, max(rtol, 1e-6), atol)


# ------------------------------------------------------------------ the wrappers
def test_the_wrappers_are_the_abi_calls_and_the_helper_runs_on_the_device():
    """Leading batch axes [2, 7]; the mask of a forest built on the device equals the one built from numpy."""
    g, nq, d = 4, 16, 64
    Q, K, V, _, _, lens, _, cap = _batch(g, nq, d, d, True, "ragged", False)
    seqs = len(lens)
    rng = np.random.default_rng(29)
    parents = np.stack([np.array([rng.integers(-1, i) for i in range(nq)]) for _ in range(seqs)])
    tm = fa.draft_mask_from_parents(_dev(parents.astype(np.int32)).reshape(2, 7, nq))
    assert tm.is_cuda and tm.dtype == torch.int32 and tuple(tm.shape) == (2, 7, nq, 1)
    assert (tm.cpu().numpy().view(np.uint32).reshape(seqs, nq, 1) == tree_ref.pack_mask(tree_ref.ancestors(parents))).all()
    tq, tl = _dev(Q), _dev(lens.astype(np.int32))
    st, *direct = _run("ragged", False, g, tq, _dev(K), _dev(V), tl, tm.reshape(seqs, nq, 1).contiguous())
    assert st == 0
    got = fa.ragged_1d(tq.reshape(2, 7, HK * g, d, nq), _dev(K).reshape(2, 7, HK, d, cap), _dev(V).reshape(2, 7, HK, d, cap),
                       tl.reshape(2, 7), tail_causal=True, returning_l_m=True, draft_mask=tm)
    torch.cuda.synchronize()
    assert got[0].shape == (2, 7, HK * g, d, nq)
    assert rg._same([t.reshape(r.shape) for t, r in zip(got, direct)], direct)
    tk, tv, tt, _ = _stored("paged", K, V, 192, rng, np.nan)
    paged = fa.paged_1d(tq.reshape(2, 7, HK * g, d, nq), tk, tv, tt.reshape(2, 7, -1), tl.reshape(2, 7), tail_causal=True,
                        returning_l_m=True, draft_mask=tm)
    torch.cuda.synchronize()
    assert rg._same([t.reshape(r.shape) for t, r in zip(paged, direct)], direct)
    # a strided mask is made contiguous
    strided = tm.reshape(seqs, nq).t().contiguous().t().reshape(2, 7, nq, 1)
    again = fa.ragged_1d(tq.reshape(2, 7, HK * g, d, nq), _dev(K).reshape(2, 7, HK, d, cap),
                         _dev(V).reshape(2, 7, HK, d, cap), tl.reshape(2, 7), tail_causal=True, draft_mask=strided)
    assert torch.equal(again, got[0])


# ------------------------------------------------------------------ graph replay
def test_a_captured_call_follows_mask_lengths_and_table_on_the_device():
    """One paged_1d tree call captured in a graph.  Between replays draft_mask, k_lens and block_table are overwritten
    in place (the pools' pages move to match the table): every replay is bitwise a fresh call on the same state."""
    g, nq, d, page = 4, 16, 64, 64
    Q, K, V, _, _, lens, masks, cap = _batch(g, nq, d, d, True, "paged", False)
    Q, K, V, lens, masks = Q[:3 * HK * g], K[:3 * HK], V[:3 * HK], lens[[3, 11, 13]], masks[[3, 11, 13]]
    rng = np.random.default_rng(31)
    table, num_pages = _table(3, cap // page, rng)
    tq = _dev(Q).reshape(3, HK * g, d, nq)
    tk, tv = _dev(_pools(K, table, page, num_pages, np.nan)), _dev(_pools(V, table, page, num_pages, np.nan))
    tt, tl, tm = _dev(table), _dev(lens.astype(np.int32)), _dev(masks)
    call = lambda *a: fa.paged_1d(tq, *a[:4], tail_causal=True, returning_l_m=True, draft_mask=a[4])  # noqa: E731
    call(tk, tv, tt, tl, tm)  # (first launches raise the kernels' LDS limit: not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(tk, tv, tt, tl, tm)
    seen = []
    for i, now in enumerate(([5, cap, 0], [513, 64, cap - 1], [77, 520, 1024])):
        tl.copy_(torch.tensor(now, dtype=torch.int32))
        new_mask = _masks([KINDS[(i + s) % 3] for s in range(3)], nq, rng)
        tm.copy_(_dev(new_mask))
        new = rng.permutation(num_pages)[:table.size].reshape(table.shape).astype(np.int32)
        tt.copy_(torch.from_numpy(new))
        tk.copy_(torch.from_numpy(_pools(K, new, page, num_pages, np.nan)))
        tv.copy_(torch.from_numpy(_pools(V, new, page, num_pages, np.nan)))
        graph.replay()
        torch.cuda.synchronize()
        fresh = call(tk.clone(), tv.clone(), tt.clone(), tl.clone(), tm.clone())
        torch.cuda.synchronize()
        assert rg._same(out, fresh), now
        st, *ragged = _run("ragged", False, g, tq.reshape(-1, d, nq), _dev(K), _dev(V), tl, tm)
        assert st == 0 and rg._same([t.reshape(r.shape) for t, r in zip(out, ragged)], ragged), now
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    del graph


# ------------------------------------------------------------------ a seeded sweep
SWEEP_DRAWS, SWEEP_PARTS = 60, 6


def _draws():
    """60 draws over (cache, d, g, nq, lengths, mask kind), from the lists above."""
    rng = np.random.default_rng(20240607)
    out = []
    for i in range(SWEEP_DRAWS):
        cache, fp8 = CACHES[i % 4] if i < 8 else CACHES[rng.integers(4)]
        g, nq = SHAPES[i % len(SHAPES)] if i < 16 else SHAPES[rng.integers(len(SHAPES))]
        d = (64, 128, 40)[i % 3] if i < 6 else (64, 128, 40)[rng.integers(3)]
        fast = d != 40
        cap = _capacity(g, nq, fast, cache)
        pool = _lengths(g, nq, cap)
        first = pool[i % len(pool)]  # (every family of lengths occurs: 60 draws walk the 14 of them four times)
        lens = [first] + [pool[rng.integers(len(pool))] if rng.random() < 0.7 else int(rng.integers(0, cap + 1)) for _ in range(2)]
        kinds = [KINDS[i % 3]] + [KINDS[rng.integers(3)] for _ in range(2)]
        out.append(dict(cache=cache, fp8=fp8, g=g, nq=nq, d=d, vd=72 if d == 40 else d, cap=cap, lens=lens, kinds=kinds,
                        page=(64, 192)[rng.integers(2)], seed=int(rng.integers(1 << 30)), family=i % len(pool)))
    return out


def test_every_family_occurs_in_the_sweep():
    draws = _draws()
    assert len(draws) == SWEEP_DRAWS
    assert {(x["cache"], x["fp8"]) for x in draws} == set(CACHES)
    assert {(x["g"], x["nq"]) for x in draws} == set(SHAPES)
    assert {x["d"] for x in draws} == {64, 128, 40}
    assert {x["family"] for x in draws} == set(range(14))
    assert {k for x in draws for k in x["kinds"]} == set(KINDS)
    assert {x["page"] for x in draws if x["cache"] == "paged"} == {64, 192}
    for x in draws:  # every draw inside the envelope: a draw outside it is an error, not a skip
        assert _rows(x["g"], x["nq"]) <= 128 and max(x["d"], x["vd"]) <= 128
        assert x["cache"] == "ragged" or (x["page"] % 64 == 0 and x["cap"] % x["page"] == 0)


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_sweep(part):
    for x in _draws()[part::SWEEP_PARTS]:
        g, nq, d, vd, cap, cache, fp8 = x["g"], x["nq"], x["d"], x["vd"], x["cap"], x["cache"], x["fp8"]
        rng = np.random.default_rng(x["seed"])
        Q, K, V, Kref, Vref = _inputs(3, g, nq, d, vd, cap, x["seed"] % 9973, fp8)
        masks = _masks(x["kinds"], nq, rng)
        lens = np.array(x["lens"])
        _two_chunks(cache, g, nq, d, vd, cap, x["page"])
        tk, tv, tt, _ = _stored(cache, K, V, x["page"], rng, _fill(fp8))
        st, *got = _run(cache, fp8, g, _dev(Q), tk, tv, _dev(lens.astype(np.int32)), _dev(masks), tt, _scales(fp8), ws_fill=0xFF)
        assert st == 0, (x, _lib.last_error())
        print(x, _check_tree(got, Q, Kref, Vref, np.repeat(lens, HK), masks, g))
