"""GPU tests of the fused K/V append (csrc/fa_cache_append.hip, fa_append_ragged / fa_append_paged and their _fp8 forms,
flash_attention.ragged_append_1d / paged_append_1d).

Everything is bit for bit against tests/append_ref.py: there are no tolerances.  Every cache starts as a random canary
pattern and the WHOLE cache is compared, so a stray store fails the test as well as a missing or a wrong one.  The shapes
are the smallest that reach each failure mode (a handful of sequences, Hk = 2, pools of a few dozen pages)."""

import numpy as np
import pytest
import torch

from tests import append_ref, fp8_ref
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F8 = getattr(torch, "float8_e4m3fn", None)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
CACHES = [("ragged", False), ("ragged", True), ("paged", False), ("paged", True)]
CACHE_IDS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _canary(rng, shape, fp8):
    """Random bytes: every bit pattern of the element type, NaN patterns included."""
    if fp8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.integers(0, 65536, shape, dtype=np.uint16).view(np.float16)


def _bits(t):
    """A cache tensor (or a numpy cache) as unsigned integers, for an exact comparison that NaN patterns survive."""
    if isinstance(t, torch.Tensor):
        t = (t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)).cpu().numpy()
    return t.view(np.uint8 if t.itemsize == 1 else np.uint16)


def _tokens(rng, S, hk, c, n, scale):
    """fp16 tokens whose quotients by `scale` (per head, or None) spread over and beyond the e4m3fn range."""
    amp = 600.0 * (np.ones(hk, np.float32) if scale is None else np.asarray(scale, np.float32))
    x = rng.standard_normal((S, hk, c, n)) * (amp.reshape(1, -1, 1, 1) / 3)
    return np.clip(x, -65000, 65000).astype(np.float16)


def _run(cache, fp8, batch, hk, c, cv, n_new, k_lens, new_lens=None, page=64, max_pages=2, table=None, num_pages=None,
         scales=True, seed=0, K_new=None, V_new=None, spare_pages=3, strided_new=False, as_uint8=False):
    """One append on the device against the reference, the whole cache compared.  `batch` is the batch shape; k_lens,
    new_lens and table are given flat over the sequences.  Returns (device K, device V, reference K, reference V)."""
    rng = np.random.default_rng(seed)
    S = int(np.prod(batch, dtype=np.int64))
    cap = max_pages * page
    ks, vs = ((np.array([0.7, 1.9, 0.33][:hk], np.float32), np.array([0.013, 0.0071, 0.5][:hk], np.float32))
              if fp8 and scales else (None, None))
    K_new = _tokens(rng, S, hk, c, n_new, ks) if K_new is None else K_new
    V_new = _tokens(rng, S, hk, cv, n_new, vs) if V_new is None else V_new
    kl = np.asarray(k_lens, np.int32)
    nl = None if new_lens is None else np.asarray(new_lens, np.int32)
    if cache == "paged":
        num_pages = S * max_pages + spare_pages if num_pages is None else num_pages
        if table is None:  # a permutation over non-adjacent pool pages
            table = rng.permutation(num_pages)[:S * max_pages].reshape(S, max_pages)
        table = np.asarray(table, np.int32).reshape(S, max_pages)
        K0, V0 = _canary(rng, (num_pages, hk, c, page), fp8), _canary(rng, (num_pages, hk, cv, page), fp8)
        Kr, Vr = append_ref.paged(K0, V0, K_new, V_new, table, kl, nl, ks, vs)
    else:
        K0, V0 = _canary(rng, (S, hk, c, cap), fp8), _canary(rng, (S, hk, cv, cap), fp8)
        Kr, Vr = append_ref.ragged(K0, V0, K_new, V_new, kl, nl, ks, vs)
    tK, tV = _dev(K0), _dev(V0)
    if cache == "ragged":
        tK, tV = tK.reshape(batch + tK.shape[1:]), tV.reshape(batch + tV.shape[1:])
    view = (lambda t: t.view(F8)) if fp8 and not as_uint8 else (lambda t: t)
    tKn, tVn = _dev(K_new).reshape(batch + K_new.shape[1:]), _dev(V_new).reshape(batch + V_new.shape[1:])
    if strided_new:  # the same values in a tensor that is not contiguous
        wide = torch.zeros(tKn.shape[:-1] + (2 * n_new,), dtype=tKn.dtype, device=DEV)
        wide[..., ::2] = tKn
        tKn = wide[..., ::2]
        assert not tKn.is_contiguous()
    kw = {}
    if nl is not None:
        kw["new_lens"] = _dev(nl).reshape(batch)
    if ks is not None:
        kw.update(k_scale=_dev(ks), v_scale=_dev(vs))
    lens = _dev(kl).reshape(batch)
    if cache == "paged":
        out = fa.paged_append_1d(view(tK), view(tV), tKn, tVn, _dev(table).reshape(batch + (max_pages,)), lens, **kw)
    else:
        out = fa.ragged_append_1d(view(tK), view(tV), tKn, tVn, lens, **kw)
    torch.cuda.synchronize()
    assert out is None
    gK, gV = _bits(tK).reshape(Kr.shape), _bits(tV).reshape(Vr.shape)
    for name, got, ref, before in (("K", gK, _bits(Kr), _bits(K0)), ("V", gV, _bits(Vr), _bits(V0))):
        bad = got != ref
        assert not bad.any(), (f"{name}: {bad.sum()} elements differ, {(bad & (ref == before)).sum()} of them outside "
                               f"the new positions; first at {tuple(np.argwhere(bad)[0])}")
    return tK, tV, Kr, Vr


# ------------------------------------------------------------------ alignment
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("n_new", [1, 2, 7, 8, 9, 17])
def test_alignment_sweep(cache, fp8, n_new):
    """L - n_new takes every residue mod 8 across the sequences (the last run crosses the page end at 64): the source
    misaligned against the destination in every way, and both partial-chunk ends."""
    starts = [0, 9, 18, 27, 36, 45, 54, 63]
    assert sorted(s % 8 for s in starts) == list(range(8))
    _run(cache, fp8, (8,), 2, 64, 64, n_new, [s + n_new for s in starts], seed=n_new)


# ------------------------------------------------------------------ pages
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("page", [64, 192])
def test_page_crossings(fp8, page):
    """A permuted table over non-adjacent pool pages.  Short runs that start in the last keys of one page and end in
    the next; 200 tokens over 4 - 5 pages of 64 keys (2 of 192); more slots than keys, where the first slots lie before
    position 0."""
    max_pages = 6 if page == 64 else 3
    _run("paged", fp8, (4,), 2, 64, 64, 5, [page + 2, 2 * page + 4, page, page + 5], page=page, max_pages=max_pages, seed=1)
    _run("paged", fp8, (4,), 2, 64, 64, 200, [260, 200, 150, max_pages * page], page=page, max_pages=max_pages, seed=2)
    _run("paged", fp8, (3,), 2, 64, 64, 200, [263, 3, 64], [200, 200, 64], page=page, max_pages=max_pages, seed=3)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_never_loaded_entries(fp8):
    """INT32_MIN, -1 and INT32_MAX in every table entry of a page that receives no new position (the values of the
    read side's test): such entries are never loaded, so the result is the reference's, which does not read them."""
    page, max_pages, n_new, S = 64, 4, 9, 3
    k_lens = [70, 9, 200]               # new positions [61, 70): pages 0, 1; [0, 9): page 0; [191, 200): pages 2, 3
    live = {0: (0, 1), 1: (0,), 2: (2, 3)}
    table = np.random.default_rng(5).permutation(S * max_pages + 3)[:S * max_pages].reshape(S, max_pages)
    poison = [I32_MIN, -1, I32_MAX]
    i = 0
    for s in range(S):
        for p in range(max_pages):
            if p not in live[s]:
                table[s, p] = poison[i % 3]
                i += 1
    assert i == S * max_pages - 5
    _run("paged", fp8, (S,), 2, 64, 64, n_new, k_lens, page=page, max_pages=max_pages, table=table,
         num_pages=S * max_pages + 3, seed=6)


def test_shared_prefix_page_is_untouched():
    """Two sequences share pool page 0 as their first page and append to their own second pages."""
    table = [[0, 3], [0, 5], [2, 4]]
    for fp8 in (False, True):
        tK, tV, Kr, Vr = _run("paged", fp8, (3,), 2, 64, 64, 7, [64 + 7, 64 + 20, 30], [7, 7, 7], table=table, num_pages=7,
                              seed=7)
        m = append_ref.written_paged(Kr.shape, 7, np.asarray(table), [71, 84, 30], [7, 7, 7])
        assert not m[0].any() and m[3].any() and m[5].any() and m[2].any() and not m[[1, 4, 6]].any()


# ------------------------------------------------------------------ clamps
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
def test_clamps_of_the_lengths(cache, fp8):
    cap, n_new = 128, 9
    k_lens = [0, -7, cap + 100, I32_MAX, I32_MIN, 50, 50, 50, 50, 50, 5, 50, 50]
    new_lens = [3, 3, 9, 2, 2, 0, 1, n_new, n_new + 5, -1, 8, I32_MAX, I32_MIN]
    _run(cache, fp8, (len(k_lens),), 2, 64, 64, n_new, k_lens, new_lens, seed=8)
    _run(cache, fp8, (len(k_lens),), 2, 64, 64, n_new, k_lens, None, seed=9)       # null new_lens: n = min(n_new, L)
    _run(cache, fp8, (3,), 2, 64, 64, n_new, [0, -1, 77], [4, 4, 0], seed=10)       # every n == 0: nothing stored


def test_nothing_to_do():
    """No sequences, no slots: FA_OK with nothing launched, the cache as it was."""
    for cache, fp8 in CACHES:
        _run(cache, fp8, (3,), 2, 64, 64, 0, [5, 6, 7], seed=11)
        _run(cache, fp8, (0,), 2, 64, 64, 4, [], seed=12, num_pages=3)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
@pytest.mark.parametrize("batch,hk,c,cv", [((3,), 2, 64, 128), ((3,), 1, 1, 40), ((2,), 3, 160, 1), ((2, 3), 2, 40, 64),
                                           ((), 3, 64, 64)], ids=str)
def test_shapes(cache, fp8, batch, hk, c, cv):
    """d != v_d, channels 1, 40 and 160 (a (sequence, head) slice of 1 to 4 blocks with a ragged last one), Hk 1 and 3,
    batch shapes (2, 3) and ().  A ragged capacity of 100 keys is no multiple of 8: its rows are not aligned, and the
    kernel falls back to element stores where a row is not."""
    S = int(np.prod(batch, dtype=np.int64))
    k_lens = [20 + 13 * s for s in range(S)]
    for n_new, new_lens in ((17, None), (3, [3 - s % 3 for s in range(S)])):
        _run(cache, fp8, batch, hk, c, cv, n_new, k_lens, new_lens, seed=13)
    if cache == "ragged":  # cap = 100: rows at odd multiples of 4 elements
        _run(cache, fp8, batch, hk, c, cv, 30, [40 + 7 * s for s in range(S)], page=50, seed=14)


@pytest.mark.parametrize("cache,fp8", CACHES, ids=CACHE_IDS)
def test_k_new_that_is_not_contiguous_and_uint8_caches(cache, fp8):
    _run(cache, fp8, (3,), 2, 64, 64, 11, [11, 70, 128], strided_new=True, as_uint8=True, seed=15)


# ------------------------------------------------------------------ FP8 codes
def _code_tokens(scale):
    """Every finite e4m3fn value, every midpoint between adjacent codes (ties, the one above 448 included), +-0,
    +-65504 / scale-free extremes and +-Inf, all times `scale` = 2^-3: exact in fp16, so the quotient is exact."""
    fin = fp8_ref.TABLE[:127]
    mids = (fin[1:] + fin[:-1]) / 2
    pos = np.concatenate([fin, mids, [464.0, 480.0, 1000.0]]) * scale
    vals = np.concatenate([pos, -pos, [65504.0, -65504.0, np.inf, -np.inf]])
    x = vals.astype(np.float16)
    assert np.array_equal(x.astype(np.float64), vals)  # exact in fp16
    return x


@pytest.mark.parametrize("cache", ["ragged", "paged"])
def test_fp8_codes(cache):
    """The binding reference is numpy's float32 quotient encoded by fp8_ref (tests/test_append_ref.py checks it
    against quantize_kv_fp8 on the CPU); equality with quantize_kv_fp8 on the GPU is asserted as well."""
    scale = 2.0 ** -3
    x = _code_tokens(scale)
    n = len(x)
    pages = -(-n // 64) + 1
    sc = np.array([scale, scale], np.float32)
    rng = np.random.default_rng(16)
    # exact codes and ties: head 0 in order, head 1 shuffled; V the negated tokens
    K_new = np.stack([x, rng.permutation(x)]).reshape(1, 2, 1, n)
    V_new = -K_new
    for L in (n, n + 3):
        rngc = np.random.default_rng(17)
        K0, V0 = _canary(rngc, (pages, 2, 1, 64), True), _canary(rngc, (pages, 2, 1, 64), True)
        table = rngc.permutation(pages).astype(np.int32).reshape(1, pages)
        tK, tV = _dev(K0), _dev(V0)
        tKn, tVn, ts = _dev(K_new), _dev(V_new), _dev(sc)
        lens = torch.tensor([L], dtype=torch.int32, device=DEV)
        if cache == "paged":
            Kr, Vr = append_ref.paged(K0, V0, K_new, V_new, table, [L], None, sc, sc)
            fa.paged_append_1d(tK.view(F8), tV.view(F8), tKn, tVn, _dev(table), lens, k_scale=ts, v_scale=ts)
            got = tK.cpu().numpy()[table[0]].transpose(1, 2, 0, 3).reshape(2, pages * 64)[:, L - n:L]
        else:
            K0, V0 = K0.reshape(1, 2, 1, -1), V0.reshape(1, 2, 1, -1)
            tK, tV = _dev(K0), _dev(V0)
            Kr, Vr = append_ref.ragged(K0, V0, K_new, V_new, [L], None, sc, sc)
            fa.ragged_append_1d(tK.view(F8), tV.view(F8), tKn, tVn, lens, k_scale=ts, v_scale=ts)
            got = tK.cpu().numpy().reshape(2, -1)[:, L - n:L]
        torch.cuda.synchronize()
        assert np.array_equal(tK.cpu().numpy(), Kr) and np.array_equal(tV.cpu().numpy(), Vr)
        # what the codes must be, spelled out: exact values map to their own code, a tie to the even code
        want = fp8_ref.encode(x.astype(np.float64) / scale)
        assert np.array_equal(got[0], want)
        exact = fp8_ref.decode(want[:127])
        assert np.array_equal(exact, fp8_ref.TABLE[:127]) and (want[127:253] % 2 == 0).all()
        assert want[253] == 0x7E and want[-1] == 0xFE and want[-2] == 0x7E and want[-3] == 0xFE and want[-4] == 0x7E
        q8, _ = fa.quantize_kv_fp8(tKn, head_axis=1, scale=ts)
        assert np.array_equal(q8.view(torch.uint8).cpu().numpy().reshape(2, n), got), "torch's device division differs"


@pytest.mark.parametrize("cache", ["ragged", "paged"])
def test_fp8_random_tokens_with_a_scale_per_head(cache):
    """Random tokens (normal, spread beyond the range) with a different non-power-of-two scale per head, against the
    reference and against quantize_kv_fp8 run on the GPU."""
    hk, c, n = 3, 8, 512
    tK, tV, Kr, Vr = _run(cache, True, (2,), hk, c, c, n, [n, n + 64], max_pages=10, seed=18)
    rng = np.random.default_rng(18)
    ks, vs = np.array([0.7, 1.9, 0.33], np.float32), np.array([0.013, 0.0071, 0.5], np.float32)
    K_new = _tokens(rng, 2, hk, c, n, ks)
    q8, _ = fa.quantize_kv_fp8(_dev(K_new), head_axis=1, scale=_dev(ks))
    assert np.array_equal(q8.view(torch.uint8).cpu().numpy(), append_ref.convert(K_new.swapaxes(0, 1), np.uint8, ks).swapaxes(0, 1)), \
        "torch's device division differs from numpy's float32 division"


# ------------------------------------------------------------------ graph replay
def test_a_captured_append_follows_every_device_input():
    """One paged_append_1d (FP8) captured in a graph; K_new, V_new, k_lens, new_lens, block_table and the scales are
    overwritten in place and the graph replayed: the pools equal the eager call's on the same data (and the
    reference's)."""
    S, hk, c, n_new, page, max_pages = 3, 2, 64, 9, 64, 3
    num_pages = S * max_pages + 2
    rng = np.random.default_rng(19)
    K0, V0 = _canary(rng, (num_pages, hk, c, page), True), _canary(rng, (num_pages, hk, c, page), True)

    def data(i):
        r = np.random.default_rng(100 + i)
        ks, vs = r.uniform(0.01, 2, hk).astype(np.float32), r.uniform(0.01, 2, hk).astype(np.float32)
        return dict(K_new=_tokens(r, S, hk, c, n_new, ks), V_new=_tokens(r, S, hk, c, n_new, vs),
                    table=r.permutation(num_pages)[:S * max_pages].reshape(S, max_pages).astype(np.int32),
                    k_lens=r.integers(0, max_pages * page + 1, S).astype(np.int32),
                    new_lens=r.integers(0, n_new + 1, S).astype(np.int32), ks=ks, vs=vs)

    d0 = data(0)
    t = {k: _dev(v) for k, v in d0.items()}
    tK, tV = _dev(K0), _dev(V0)
    call = lambda K, V, t: fa.paged_append_1d(K.view(F8), V.view(F8), t["K_new"], t["V_new"], t["table"], t["k_lens"],  # noqa: E731
                                              new_lens=t["new_lens"], k_scale=t["ks"], v_scale=t["vs"])
    call(tK, tV, t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(tK, tV, t)
    for i in (1, 2, 3):
        d = data(i)
        for k, v in d.items():
            t[k].copy_(torch.from_numpy(v))
        tK.copy_(torch.from_numpy(K0))
        tV.copy_(torch.from_numpy(V0))
        graph.replay()
        torch.cuda.synchronize()
        eK, eV = _dev(K0), _dev(V0)
        call(eK, eV, {k: _dev(v) for k, v in d.items()})
        torch.cuda.synchronize()
        assert torch.equal(tK, eK) and torch.equal(tV, eV), i
        Kr, Vr = append_ref.paged(K0, V0, d["K_new"], d["V_new"], d["table"], d["k_lens"], d["new_lens"], d["ks"], d["vs"])
        assert np.array_equal(tK.cpu().numpy(), Kr) and np.array_equal(tV.cpu().numpy(), Vr), i
    del graph


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_decode_steps_and_a_prefill_chunk_end_to_end(fp8):
    """From an empty paged cache: six steps of (append one token, paged_1d), then one step of a 70-token
    paged_append_1d plus paged_prefill_1d with new_lens mixing 70 and 1.  Every output equals, bit for bit, the same
    forward on pools written by append_ref."""
    S, hk, g, c, page, max_pages = 3, 2, 2, 64, 64, 3
    num_pages = S * max_pages + 1
    rng = np.random.default_rng(20)
    ks, vs = ((np.array([0.05, 0.02], np.float32), np.array([0.03, 0.01], np.float32)) if fp8 else (None, None))
    zero = np.zeros((num_pages, hk, c, page), np.uint8 if fp8 else np.float16)
    Kr, Vr = zero.copy(), zero.copy()
    tK, tV = _dev(Kr), _dev(Vr)
    table = rng.permutation(num_pages)[:S * max_pages].reshape(S, max_pages).astype(np.int32)
    tt = _dev(table)
    view = (lambda x: x.view(F8)) if fp8 else (lambda x: x)
    sc = dict(k_scale=_dev(ks), v_scale=_dev(vs)) if fp8 else {}
    lens = np.zeros(S, np.int32)
    steps = [(1, None)] * 6 + [(70, np.array([70, 1, 70], np.int32))]
    for n_new, new_lens in steps:
        K_new = rng.uniform(-2, 2, (S, hk, c, n_new)).astype(np.float16)
        V_new = rng.uniform(-2, 2, (S, hk, c, n_new)).astype(np.float16)
        Q = rng.uniform(-2, 2, (S, hk * g, c, n_new)).astype(np.float16)
        lens = lens + (n_new if new_lens is None else new_lens)
        tl = _dev(lens.astype(np.int32))
        fa.paged_append_1d(view(tK), view(tV), _dev(K_new), _dev(V_new), tt, tl,
                           new_lens=None if new_lens is None else _dev(new_lens), **sc)
        Kr, Vr = append_ref.paged(Kr, Vr, K_new, V_new, table, lens, new_lens, ks, vs)
        forward = fa.paged_1d if n_new == 1 else fa.paged_prefill_1d
        got = forward(_dev(Q), view(tK), view(tV), tt, tl, tail_causal=True, returning_l_m=True, **sc)
        want = forward(_dev(Q), view(_dev(Kr)), view(_dev(Vr)), tt, tl, tail_causal=True, returning_l_m=True, **sc)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(tK), _bits(Kr)) and np.array_equal(_bits(tV), _bits(Vr))
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a.view(torch.int32),
                               b.view(torch.int16) if b.dtype == torch.float16 else b.view(torch.int32)), n_new
    assert list(lens) == [76, 7, 76]
