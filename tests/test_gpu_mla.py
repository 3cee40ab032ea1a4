"""GPU tests of MLA decode over a paged latent cache (csrc/fa_fwd_f16_mla.hip, fa_forward_mla_paged,
flash_attention.mla_paged_1d): Hq query heads against one K/V head whose keys are the pool's
vectors and whose values are their first v channels.

The reference is tests/ragged_ref.forward_f64 on the cache gathered through the table, V = K[:, :v, :] and g = Hq,
under test_gpu_ragged._check_ref (the fp16 forward rule: O and l within gate.TOL[float16]['fwd'], m within its ulp and
dot-product bound).  Every cache is built padded first and scattered into the pool through a seeded random table;
pool pages that no sequence owns are NaN.  The table, batch, poison and graph tests are bitwise."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

SPARE = 5  # pool pages that no sequence owns
DEV = "cuda:0"


def _problem(nq, cap, c, v, b):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), c, v)


def _plan(nq, cap, c, v, hq, page):
    out = (ctypes.c_int32 * 5)()
    assert _lib.lib().fa_forward_mla_paged_plan(_problem(nq, cap, c, v, hq), hq, page, out) == 0
    return tuple(out)


def _case(seqs, hq, c, nq, page, seed, identity=False):
    """Q [seqs * hq, c, nq], the padded latent cache [seqs, c, cap] of about 2600 keys, a table over
    seqs * max_pages + SPARE pages (random, or in order) and the pool."""
    max_pages = -(-2600 // page)
    Q, K, _ = rg._np_inputs(seqs, hq, c, 1, nq, max_pages * page, seed)
    num_pages = seqs * max_pages + SPARE
    order = np.arange(num_pages) if identity else np.random.default_rng(seed + 1).permutation(num_pages)
    table = order[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    pool = np.full((num_pages, c, page), np.nan, np.float16)
    pool[table] = K.reshape(seqs, c, max_pages, page).transpose(0, 2, 1, 3)
    return Q, K, table, pool


def _t(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def _abi(hq, v, Q, pool, table, lens, tail=False, scale=None):
    """fa_forward_mla_paged on device tensors; returns (O [b, v, nq], l, m)."""
    L = _lib.lib()
    b, c, nq = Q.shape
    num_pages, _, page = pool.shape
    table, lens = _t(table, torch.int32), _t(lens, torch.int32)
    max_pages = table.shape[-1]
    prob = _problem(nq, max_pages * page, c, v, b)
    O_ = torch.empty((b, v, nq), dtype=torch.float16, device=DEV)
    l = torch.empty((b, nq), dtype=torch.float32, device=DEV)
    m = torch.empty((b, nq), dtype=torch.float16, device=DEV)
    need = int(L.fa_forward_mla_paged_workspace_bytes(prob, hq, page))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=DEV)
    st = L.fa_forward_mla_paged(torch.cuda.current_stream().cuda_stream, prob, hq, Q.data_ptr(), pool.data_ptr(),
                                table.data_ptr(), max_pages, page, num_pages, lens.data_ptr(), int(tail),
                                1.0 / math.sqrt(c) if scale is None else scale, O_.data_ptr(), l.data_ptr(),
                                m.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == 0, _lib.last_error()
    return O_, l, m


def _check(got, Q, K, v, lens, hq, tail, scale=None):
    c = Q.shape[1]
    Qr = Q if scale is None else Q.astype(np.float64) * scale * math.sqrt(c)
    res = rg._check_ref(got, Qr, K, K[:, :v, :], lens, hq, tail)
    print("worst |error| / allowance:", res)


# ------------------------------------------------------------------ parity over the instance space
@pytest.mark.parametrize("hq,nq,tail", [(1, 1, False), (16, 1, False), (128, 1, False), (65, 1, False), (16, 3, True),
                                        (128, 2, True), (128, 4, True)])
@pytest.mark.parametrize("c,v", [(576, 512), (320, 256), (64, 64)])
@pytest.mark.parametrize("page", [64, 192])
def test_parity_with_the_float64_reference(page, c, v, hq, nq, tail):
    """One row, one full block, two blocks, a ragged second block, pitch 4 with a dead slot, R = 256 and 512; the
    full instance, fewer channel groups on both sides, and one group."""
    Q, K, table, pool = _case(3, hq, c, nq, page, seed=1000 * c + 10 * hq + nq + page)
    cap = K.shape[2]
    assert _plan(nq, cap, c, v, hq, page)[0] >= 3
    lens = [cap, 1300, 77]
    _check(_abi(hq, v, _t(Q), _t(pool), table, lens, tail), Q, K, v, lens, hq, tail)


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_lengths_at_tile_chunk_and_capacity_edges(tail):
    """(576, 512), Hq = 16, Nq = 3: under the tail rule the rows before position 0 are empty rows; lengths outside
    [0, capacity] are clamped."""
    hq, nq, c, v, page = 16, 3, 576, 512, 64
    cap = -(-2600 // page) * page
    chunks, chunk = _plan(nq, cap, c, v, hq, page)[:2]
    assert chunks >= 3
    lens = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, cap - 1, cap + 7, -3]
    Q, K, table, pool = _case(len(lens), hq, c, nq, page, seed=7 + tail)
    _check(_abi(hq, v, _t(Q), _t(pool), table, lens, tail), Q, K, v, lens, hq, tail)


def test_softmax_scale_of_mla():
    hq, nq, c, v, page = 16, 2, 576, 512, 64
    Q, K, table, pool = _case(3, hq, c, nq, page, seed=192)
    lens = [K.shape[2], 1300, 77]
    scale = 1.0 / math.sqrt(192)
    _check(_abi(hq, v, _t(Q), _t(pool), table, lens, True, scale), Q, K, v, lens, hq, True, scale)


# ------------------------------------------------------------------ bitwise guarantees
BIT = dict(hq=16, nq=2, c=576, v=512, page=64)


def test_a_random_table_is_bitwise_the_identity_table():
    lens = [2600, 1300, 77]
    got = []
    for identity in (False, True):
        Q, _, table, pool = _case(3, BIT["hq"], BIT["c"], BIT["nq"], BIT["page"], seed=11, identity=identity)
        got.append(_abi(BIT["hq"], BIT["v"], _t(Q), _t(pool), table, lens, True))
    assert rg._same(*got)


def test_a_sequence_alone_is_bitwise_itself_in_a_batch():
    hq = BIT["hq"]
    Q, _, table, pool = _case(3, hq, BIT["c"], BIT["nq"], BIT["page"], seed=12)
    lens = [2600, 1300, 77]
    batch = _abi(hq, BIT["v"], _t(Q), _t(pool), table, lens, True)
    for s in range(3):
        alone = _abi(hq, BIT["v"], _t(Q[s * hq:(s + 1) * hq]), _t(pool), table[s:s + 1], lens[s:s + 1], True)
        assert rg._same(alone, [t[s * hq:(s + 1) * hq] for t in batch])


def test_poison_past_the_lengths_and_in_dead_table_entries_is_harmless():
    """NaN past each length, and the table entries of pages without a live key pointed at an all-NaN page (in
    range: the clamp of loaded entries is the code's, not this test's)."""
    hq, page = BIT["hq"], BIT["page"]
    Q, K, table, pool = _case(3, hq, BIT["c"], BIT["nq"], page, seed=13)
    lens = [2500, 1300, 77]
    clean = _abi(hq, BIT["v"], _t(Q), _t(pool), table, lens, True)
    K2, table2 = K.copy(), table.copy()
    for s, n in enumerate(lens):
        K2[s, :, n:] = np.nan
        table2[s, -(-n // page):] = pool.shape[0] - 1  # an unowned page: all NaN
    pool2 = pool.copy()
    pool2[table] = K2.reshape(3, BIT["c"], -1, page).transpose(0, 2, 1, 3)
    assert np.isnan(pool2[-1].astype(np.float32)).all()
    assert rg._same(clean, _abi(hq, BIT["v"], _t(Q), _t(pool2), table2, lens, True))


def test_graph_replay_after_the_lengths_and_the_table_change():
    hq, v = BIT["hq"], BIT["v"]
    Q, K, table, pool = _case(3, hq, BIT["c"], BIT["nq"], BIT["page"], seed=14)
    tq, tp = _t(Q).reshape(3, hq, BIT["c"], BIT["nq"]), _t(pool)
    tt, tl = _t(table, torch.int32), _t([2600, 1300, 77], torch.int32)
    call = lambda: fa.mla_paged_1d(tq, tp, tt, tl, v, tail_causal=True, returning_l_m=True)  # noqa: E731
    call()  # (warm: the kernel's LDS limit is raised outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    tl.copy_(_t([5, 2048, 700], torch.int32))
    tt.copy_(_t(table[::-1].copy(), torch.int32))
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert rg._same(out, call())


# ------------------------------------------------------------------ the Python wrapper
@pytest.mark.parametrize("returning_l_m", [False, True])
def test_wrapper_over_a_two_axis_batch(returning_l_m):
    hq, nq, c, v, page = 8, 2, 128, 64, 64
    Q, K, table, pool = _case(6, hq, c, nq, page, seed=15)
    lens = [2600, 1300, 77, 0, 64, 513]
    got = fa.mla_paged_1d(_t(Q).reshape(2, 3, hq, c, nq), _t(pool), _t(table.reshape(2, 3, -1)),
                          _t(lens, torch.int32).reshape(2, 3), v, returning_l_m=returning_l_m)
    torch.cuda.synchronize()
    O = got[0] if returning_l_m else got
    assert isinstance(got, tuple) == returning_l_m
    assert O.shape == (2, 3, hq, v, nq) and O.dtype == torch.float16
    if returning_l_m:
        assert got[1].shape == got[2].shape == (2, 3, hq, nq)
        assert got[1].dtype == torch.float32 and got[2].dtype == torch.float16
        _check(tuple(t.reshape((-1,) + t.shape[3:]) for t in got), Q, K, v, lens, hq, False)
    else:
        assert rg._same([O.reshape(-1, v, nq)], _abi(hq, v, _t(Q), _t(pool), table, lens)[:1])
