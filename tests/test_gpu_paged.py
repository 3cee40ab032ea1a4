"""GPU tests of the paged few-query forward (csrc/fa_fwd_f16_decode.hip over PagedCache, fa_forward_paged, flash_attention.paged_1d;
DESIGN.md §3.10): K and V live in pools of pages [num_pages, Hk, channels, page], a device block table says which
page holds keys [p * page, (p + 1) * page) of which sequence, and the lengths are device data.

The main instrument is bitwise equality with fa_forward_ragged on the gathered padded cache with the same lengths:
the plan, the tiles and the staged values are the same, so an addressing error shows without a tolerance.  One
check per form (full, tail-causal) goes against tests/paged_ref.py under test_gpu_ragged._check_ref's tolerance rule,
so that the suite does not rest on the ragged kernel alone.  Every cache is built padded first and scattered into
the pool through a seeded random table; pool pages that no sequence owns are NaN."""

import ctypes

import numpy as np
import pytest
import torch

from tests import paged_ref
from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

HK = 2            # K/V heads of a sequence (kv_per_len)
SPARE = 5         # pool pages that no sequence owns
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _problem(nq, cap, d, vd, b):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, vd)


def _plan(nq, cap, d, vd, g, page):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_paged_plan(_problem(nq, cap, d, vd, g), g, page, out) == 0
    return tuple(out)


def _max_pages(page):
    """About 2600 keys, as in the ragged tests: 6 chunks of 512 keys, 3 of 1024 above 64 folded rows."""
    return -(-2600 // page)


def _scatter(cache, table, page, num_pages, fill=np.nan):
    """The padded cache [seqs * HK, c, cap] as a pool [num_pages, HK, c, page] through ``table``; pages that the
    table does not name hold ``fill``."""
    seqs, max_pages = table.shape
    c = cache.shape[1]
    pool = np.full((num_pages, HK, c, page), fill, np.float16)
    pool[table] = cache.reshape(seqs, HK, c, max_pages, page).transpose(0, 3, 1, 2, 4)
    return pool


def _case(seqs, g, d, vd, nq, page, seed, max_pages=None):
    """Q, the padded K / V caches, a random table over seqs * max_pages + SPARE pages, and the pools."""
    max_pages = _max_pages(page) if max_pages is None else max_pages
    cap = max_pages * page
    Q, K, V = rg._np_inputs(seqs * HK, g, d, vd, nq, cap, seed)
    num_pages = seqs * max_pages + SPARE
    table = np.random.default_rng(seed + 1).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    return Q, K, V, table, _scatter(K, table, page, num_pages), _scatter(V, table, page, num_pages)


def _dev(x, misalign=False):
    return rg._dev(x, misalign)


def _abi(g, Q, Kp, Vp, table, lens, tail=False, ws_short=0, fill=None, ws_fill=None, page=None, max_pages=None):
    """fa_forward_paged on device tensors (table, lens: device int32 tensors, numpy arrays or lists); returns
    (status, O, l, m).  ``page`` / ``max_pages`` override what the shapes say (the out-of-envelope test)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    num_pages, hk, vd, pg = Vp.shape
    page = pg if page is None else page
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    table, lens = as_dev(table), as_dev(lens)
    max_pages = table.shape[-1] if max_pages is None else max_pages
    prob = _problem(nq, max_pages * page, d, vd, b)
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O_, l, m):
            t.view(torch.uint8).fill_(fill)
    need = int(L.fa_forward_paged_workspace_bytes(prob, g, page))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    st = L.fa_forward_paged(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(),
                            table.data_ptr(), max_pages, page, num_pages, lens.data_ptr(), hk, int(tail), O_.data_ptr(),
                            l.data_ptr(), m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0))
    torch.cuda.synchronize()
    return st, O_, l, m


def _ragged(g, Q, K, V, lens, tail=False):
    """fa_forward_ragged on the padded cache, one length per sequence."""
    st, *out = rg._abi(g, Q, K, V, lens, kv_per_len=HK, tail=tail)
    assert st == 0
    return out


# ------------------------------------------------------------------ tables, page sizes and instances
@pytest.mark.parametrize("g,nq", [(1, 1), (1, 33), (8, 1), (3, 3), (2, 64)])
@pytest.mark.parametrize("d,vd", [(128, 128), (64, 64), (32, 32), (96, 40), (8, 8)])
@pytest.mark.parametrize("page", [64, 128, 192])
def test_a_random_table_is_bitwise_the_ragged_forward_on_the_gathered_cache(page, d, vd, g, nq):
    """Both stagings (16-byte at d == v_d in {32, 64, 128}, element-wise otherwise), every D instance, several
    pitches of the fold; then pools misaligned by one element (element-wise staging on both sides)."""
    max_pages = _max_pages(page)
    cap = max_pages * page
    assert _plan(nq, cap, d, vd, g, page)[0] >= 3
    lens = [cap, 1300, 77]
    Q, K, V, table, Kp, Vp = _case(3, g, d, vd, nq, page, seed=1000 * d + 10 * g + nq + page)
    tq = _dev(Q)
    st, *got = _abi(g, tq, _dev(Kp), _dev(Vp), table, lens)
    assert st == 0
    assert rg._same(got, _ragged(g, tq, _dev(K), _dev(V), lens))
    st, *mis = _abi(g, tq, _dev(Kp, True), _dev(Vp, True), table, lens)
    assert st == 0
    assert rg._same(mis, _ragged(g, tq, _dev(K, True), _dev(V, True), lens))


# ------------------------------------------------------------------ length edges
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("nq", [1, 4, 33])
@pytest.mark.parametrize("page", [64, 128, 192])
def test_lengths_at_page_tile_and_chunk_edges(page, nq, tail):
    g, d = (1 if nq == 33 else 2), 64
    max_pages = _max_pages(page)
    cap = max_pages * page
    chunks, chunk = _plan(nq, cap, d, d, g, page)[:2]
    assert chunks >= 3
    lens = [0, 1, 63, 64, 65, page - 1, page, page + 1, chunk - 1, chunk, chunk + 1, cap - 1, cap, cap + 7]
    Q, K, V, table, Kp, Vp = _case(len(lens), g, d, d, nq, page, seed=page + nq)
    tq = _dev(Q)
    st, *got = _abi(g, tq, _dev(Kp), _dev(Vp), table, lens, tail=tail)
    assert st == 0
    assert rg._same(got, _ragged(g, tq, _dev(K), _dev(V), lens, tail))
    rg._check_empty(got, np.repeat(np.asarray(lens) == 0, HK * g)[:, None] & np.ones((1, nq), bool))


# ------------------------------------------------------------------ an independent reference
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_against_the_float64_reference(tail):
    g, nq, d, vd, page = 2, 4, 96, 40, 192
    Q, _, _, table, Kp, Vp = _case(3, g, d, vd, nq, page, seed=21)
    cap = table.shape[1] * page
    lens = [cap, 3, 1000]
    st, *got = _abi(g, _dev(Q), _dev(Kp), _dev(Vp), table, lens, tail=tail)
    assert st == 0
    rg._check_ref(got, Q, paged_ref.gather(Kp, table, page), paged_ref.gather(Vp, table, page), np.repeat(lens, HK), g, tail)


# ------------------------------------------------------------------ dead table entries
@pytest.mark.parametrize("page", [64, 192])
def test_entries_of_pages_without_a_live_key_are_never_read(page):
    g, nq, d = 4, 4, 64
    Q, _, _, table, Kp, Vp = _case(3, g, d, d, nq, page, seed=31)
    max_pages = table.shape[1]
    lens = np.array([0, page, page + 1])
    dead = np.arange(max_pages)[None, :] >= -(-lens // page)[:, None]
    tq, tk, tv = _dev(Q), _dev(Kp), _dev(Vp)
    for tail in (False, True):
        st, *ref = _abi(g, tq, tk, tv, np.where(dead, 0, table), lens, tail=tail)
        assert st == 0
        for junk in (INT32_MIN, -1, INT32_MAX):
            st, *got = _abi(g, tq, tk, tv, np.where(dead, junk, table).astype(np.int32), lens, tail=tail)
            assert st == 0
            assert rg._same(got, ref), junk


# ------------------------------------------------------------------ poison
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("misalign", [False, True], ids=["fast", "elementwise"])
def test_values_past_the_length_and_unused_pages_do_not_reach_the_result(misalign, tail):
    """Pool values past each length (the rest of the last live page and every later page of the sequence) are NaN,
    Inf or 65504, pages that no sequence owns are NaN, the workspace is 0xFF bytes: bitwise the call with zeros."""
    g, nq, d, page = 4, 4, 64, 128
    Q, K, V, table, _, _ = _case(3, g, d, d, nq, page, seed=41)
    cap = K.shape[2]
    lens = [1, 577, cap - 1]
    past = np.arange(cap)[None, None, :] >= np.repeat(lens, HK)[:, None, None]
    num_pages = table.size + SPARE
    pools = lambda x, spare: (_dev(_scatter(np.where(past, np.float16(x), K), table, page, num_pages, spare), misalign),  # noqa: E731
                              _dev(_scatter(np.where(past, np.float16(x), V), table, page, num_pages, spare), misalign))
    tq = _dev(Q)
    st, *ref = _abi(g, tq, *pools(0.0, 0.0), table, lens, tail=tail)
    assert st == 0
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    for poison in (np.nan, np.inf, 65504.0):
        st, *got = _abi(g, tq, *pools(poison, np.nan), table, lens, tail=tail, ws_fill=0xFF)
        assert st == 0
        assert rg._same(got, ref), f"poison {poison}"


# ------------------------------------------------------------------ shared pages, batch independence
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_a_shared_prefix_and_a_sequence_alone(tail):
    """Sequences 0 and 1 name the same two physical pages for their first 2 * page keys: bitwise the run in which
    sequence 1 owns private copies of them.  And a sequence's bits do not depend on the batch."""
    g, nq, d, vd, page = 2, 5, 96, 40, 128
    Q, K, V, table, _, _ = _case(3, g, d, vd, nq, page, seed=51)
    K[HK:2 * HK, :, :2 * page] = K[:HK, :, :2 * page]
    V[HK:2 * HK, :, :2 * page] = V[:HK, :, :2 * page]
    num_pages = table.size + SPARE
    Kp, Vp = _scatter(K, table, page, num_pages), _scatter(V, table, page, num_pages)
    shared = table.copy()
    shared[1, :2] = table[0, :2]
    Ks, Vs = Kp.copy(), Vp.copy()
    Ks[table[1, :2]] = np.nan  # sequence 1's own copies are no longer named by any entry
    Vs[table[1, :2]] = np.nan
    lens = [2 * page + 9, 2 * page + 300, 40]
    tq = _dev(Q)
    st0, *private = _abi(g, tq, _dev(Kp), _dev(Vp), table, lens, tail=tail)
    st1, *got = _abi(g, tq, _dev(Ks), _dev(Vs), shared, lens, tail=tail)
    assert st0 == 0 and st1 == 0
    assert rg._same(got, private)
    assert rg._same(got, _ragged(g, tq, _dev(K), _dev(V), lens, tail))
    q1 = slice(HK * g, 2 * HK * g)
    st2, *alone = _abi(g, tq[q1].contiguous(), _dev(Ks), _dev(Vs), shared[1:2], lens[1:2], tail=tail)
    assert st2 == 0
    assert rg._same([t[q1] for t in got], alone)


# ------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_python_wrapper_is_the_abi_call(tail):
    """Leading batch axes [2, 3]; and tensors without a batch axis with a 1-d table and a 0-d k_lens."""
    g, nq, d, page = 4, 4, 64, 192
    Q, _, _, table, Kp, Vp = _case(6, g, d, d, nq, page, seed=61, max_pages=6)
    cap = 6 * page
    lens = [[cap, 5, 513], [0, 700, 64]]
    tq, tk, tv = _dev(Q), _dev(Kp), _dev(Vp)
    tt = torch.tensor(table, dtype=torch.int32, device=tq.device)
    tl = torch.tensor(lens, dtype=torch.int32, device=tq.device)
    st, *direct = _abi(g, tq, tk, tv, tt, tl.reshape(-1), tail=tail)
    assert st == 0
    got = fa.paged_1d(tq.reshape(2, 3, HK * g, d, nq), tk, tv, tt.reshape(2, 3, -1), tl, tail_causal=tail, returning_l_m=True)
    torch.cuda.synchronize()
    assert got[0].shape == (2, 3, HK * g, d, nq) and got[1].shape == got[2].shape == (2, 3, HK * g, nq)
    assert rg._same([t.reshape(r.shape) for t, r in zip(got, direct)], direct)
    q1 = slice(HK * g, 2 * HK * g)
    one = fa.paged_1d(tq[q1], tk, tv, tt[1], tl[0, 1], tail_causal=tail, returning_l_m=True)
    torch.cuda.synchronize()
    assert rg._same(one, [t[q1] for t in direct])
    assert torch.equal(fa.paged_1d(tq[q1], tk, tv, tt[1], tl[0, 1], tail_causal=tail), one[0])


# ------------------------------------------------------------------ ABI statuses
def test_short_workspace_is_rejected_and_nothing_is_written():
    Q, _, _, table, Kp, Vp = _case(2, 4, 64, 64, 8, 64, seed=71)
    st, *out = _abi(4, _dev(Q), _dev(Kp), _dev(Vp), table, [2600, 100], ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


def test_a_page_of_32_keys_is_unsupported_and_nothing_is_written():
    """The pool of 64-key pages handed in as twice as many 32-key pages: a well-formed call outside the envelope."""
    Q, _, _, table, Kp, Vp = _case(2, 4, 64, 64, 8, 64, seed=72)
    table32 = np.stack([2 * table, 2 * table + 1], axis=-1).reshape(2, -1).astype(np.int32)
    st, *out = _abi(4, _dev(Q), _dev(Kp), _dev(Vp), table32, [2600, 100], fill=0x5A, page=32)
    assert st == _lib.FA_ERR_UNSUPPORTED and "page % 64" in _lib.last_error()
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


# ------------------------------------------------------------------ graph replay
def test_a_captured_call_follows_the_lengths_and_the_table_on_the_device():
    """One paged_1d call captured in a (linear, one-stream) graph.  Between replays k_lens is overwritten in place,
    and so is block_table, with a new permutation, while the pools' pages move to match: every replay is bitwise
    the eager call on the same state."""
    g, nq, d, page = 4, 4, 64, 128
    Q, K, V, table, Kp, Vp = _case(3, g, d, d, nq, page, seed=81)
    num_pages, cap = Kp.shape[0], K.shape[2]
    tq = _dev(Q).reshape(3, HK * g, d, nq)
    tk, tv = _dev(Kp), _dev(Vp)
    tt = torch.tensor(table, dtype=torch.int32, device=tq.device)
    lens = torch.tensor([cap, 1, 700], dtype=torch.int32, device=tq.device)
    for tail in (False, True):
        fa.paged_1d(tq, tk, tv, tt, lens, tail_causal=tail)  # (first launches raise the kernels' LDS limit: not capturable)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fa.paged_1d(tq, tk, tv, tt, lens, tail_causal=tail, returning_l_m=True)
        for i, now in enumerate(([5, cap, 0], [513, 64, cap - 1], [77, 77, 1024])):
            lens.copy_(torch.tensor(now, dtype=torch.int32))
            new = np.random.default_rng(90 + i).permutation(num_pages)[:table.size].reshape(table.shape).astype(np.int32)
            tt.copy_(torch.from_numpy(new))
            tk.copy_(torch.from_numpy(_scatter(K, new, page, num_pages)))
            tv.copy_(torch.from_numpy(_scatter(V, new, page, num_pages)))
            graph.replay()
            torch.cuda.synchronize()
            eager = fa.paged_1d(tq, tk.clone(), tv.clone(), tt.clone(), lens.clone(), tail_causal=tail, returning_l_m=True)
            torch.cuda.synchronize()
            assert rg._same(out, eager), now
            assert rg._same([t.reshape((-1,) + t.shape[2:]) for t in out],
                            _ragged(g, tq.reshape(-1, d, nq), _dev(K), _dev(V), now, tail)), now
        del graph
