"""GPU tests of the 256-channel paged forward (csrc/fa_fwd_f16_paged_wide.hip, fa_forward_paged_wide, the wide route
of flash_attention.paged_1d) against the float64 references of the paged and windowed forwards, under
test_gpu_ragged._check_ref's and test_gpu_window._check_window's rules, and bit for bit against itself."""

import ctypes

import numpy as np
import pytest
import torch

from tests import test_gpu_paged as pg
from tests import test_gpu_ragged as rg
from tests import test_gpu_window as gw
from tests import window_ref
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu
HK = pg.HK


def _plan(nq, cap, d, vd, g, page):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_paged_wide_plan(pg._problem(nq, cap, d, vd, g), g, page, out) == 0
    return tuple(out)


def _wide(g, Q, Kp, Vp, table, lens, tail=False, window=0):
    """fa_forward_paged_wide on device tensors (table, lens: device int32 tensors, arrays or lists): (O, l, m), the
    outputs filled with 0x5A and the workspace with 0xFF bytes first."""
    L = _lib.lib()
    b, d, nq = Q.shape
    num_pages, hk, vd, page = Vp.shape
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    table, lens = as_dev(table), as_dev(lens)
    prob = pg._problem(nq, table.shape[-1] * page, d, vd, b)
    out = [torch.empty(s, dtype=t, device=Q.device) for s, t in (((b, vd, nq), torch.float16), ((b, nq), torch.float32),
                                                               ((b, nq), torch.float16))]
    for t in out:
        t.view(torch.uint8).fill_(0x5A)
    need = int(L.fa_forward_paged_wide_workspace_bytes(prob, g, page))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=Q.device)
    st = L.fa_forward_paged_wide(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), Kp.data_ptr(),
                                 Vp.data_ptr(), table.data_ptr(), table.shape[-1], page, num_pages, lens.data_ptr(), hk,
                                 int(tail), window, *(t.data_ptr() for t in out), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == 0, _lib.last_error()
    return out


@pytest.mark.parametrize("page", [64, 192])
@pytest.mark.parametrize("g,nq,tail", [(1, 1, False), (2, 1, False), (5, 2, True), (8, 3, True), (16, 8, True)])
@pytest.mark.parametrize("d,vd", [(256, 256), (192, 128), (128, 256)])
def test_paged_1d_against_float64(d, vd, g, nq, tail, page):
    """One row, a ragged fold, a dead query slot, and two row blocks at R = 128, through the public call."""
    lens = [pg._max_pages(page) * page, 1300, 77]
    assert _plan(nq, lens[0], d, vd, g, page)[0] >= 3
    Q, K, V, table, Kp, Vp = pg._case(3, g, d, vd, nq, page, seed=d + vd + 10 * g + nq + page)
    dev = lambda x: torch.tensor(x, device="cuda:0")  # noqa: E731
    got = fa.paged_1d(dev(Q).reshape(3, HK * g, d, nq), dev(Kp), dev(Vp), dev(table), dev(np.int32(lens)),
                      tail_causal=tail, returning_l_m=True)
    res = rg._check_ref([t.reshape(r) for t, r in zip(got, ((-1, vd, nq), (-1, nq), (-1, nq)))], Q, K, V,
                        np.repeat(lens, HK), g, tail)
    print(f"d={d} vd={vd} g={g} nq={nq} page={page}: worst error / allowance {res}")


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_length_edges(tail):
    """Tile, chunk and capacity edges, lengths past the capacity and below zero (clamped), and the empty rows."""
    g, nq, d, page = 2, 3, 256, 64
    cap = pg._max_pages(page) * page
    chunk = _plan(nq, cap, d, d, g, page)[1]
    lens = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, cap - 1, cap + 7, -3]
    Q, K, V, table, Kp, Vp = pg._case(len(lens), g, d, d, nq, page, seed=7)
    got = _wide(g, pg._dev(Q), pg._dev(Kp), pg._dev(Vp), table, lens, tail)
    rg._check_ref(got, Q, K, V, np.repeat(np.clip(lens, 0, cap), HK), g, tail)


@pytest.mark.parametrize("nq", [1, 4])
@pytest.mark.parametrize("window", [1, 63, 64, 65, 700])
def test_windows_at_edge_lengths(window, nq):
    g, d, page = 2, 256, 192
    cap = pg._max_pages(page) * page
    lens = gw._edge_lengths(cap, nq, window, _plan(nq, cap, d, d, g, page)[1])
    Q, K, V, table, Kp, Vp = pg._case(len(lens), g, d, d, nq, page, seed=window + nq)
    got = _wide(g, pg._dev(Q), pg._dev(Kp), pg._dev(Vp), table, lens, True, window)
    gw._check_window(got, Q, K, V, np.repeat(lens, HK), g, window)


def test_bitwise_guarantees():
    """A window that reaches the capacity is the tail call; a random table is the identity table; a sequence alone is
    itself in a batch; the wrapper is the ABI call."""
    g, nq, d, vd, page, window = 4, 3, 256, 192, 192, 300
    lens = [2 * page + 9, 2688, 40, 1100]
    Q, K, V, table, Kp, Vp = pg._case(4, g, d, vd, nq, page, seed=51)
    cap = K.shape[2]
    tq, tk, tv = pg._dev(Q), pg._dev(Kp), pg._dev(Vp)
    tail = _wide(g, tq, tk, tv, table, lens, True)
    for w in (cap, cap + 1, 2 ** 31 - 1):
        assert rg._same(_wide(g, tq, tk, tv, table, lens, True, w), tail), w
    a = _wide(g, tq, tk, tv, table, lens, True, window)
    ident = np.arange(table.size, dtype=np.int32).reshape(table.shape)
    ik, iv = (pg._dev(pg._scatter(x, ident, page, table.size + pg.SPARE)) for x in (K, V))
    assert rg._same(_wide(g, tq, ik, iv, ident, lens, True, window), a)
    for s in range(4):
        q1 = slice(s * HK * g, (s + 1) * HK * g)
        alone = _wide(g, tq[q1].contiguous(), tk, tv, table[s:s + 1], lens[s:s + 1], True, window)
        assert rg._same([t[q1] for t in a], alone), s
    tt, tl = torch.tensor(table, device="cuda:0"), torch.tensor(lens, dtype=torch.int32, device="cuda:0")
    got = fa.paged_1d(tq.reshape(4, HK * g, d, nq), tk, tv, tt, tl, tail_causal=True, returning_l_m=True, window_size=window)
    assert rg._same([t.reshape(r.shape) for t, r in zip(got, a)], a)
    q1 = tq[:, :, :1].contiguous()  # (one query under a window needs no tail_causal)
    one = _wide(g, q1, tk, tv, table, lens, True, window)
    got = fa.paged_1d(q1.reshape(4, HK * g, d, 1), tk, tv, tt, tl, returning_l_m=True, window_size=window)
    assert rg._same([t.reshape(r.shape) for t, r in zip(got, one)], one)


@pytest.mark.parametrize("nq,window", [(1, 0), (4, 300), (1, 64)])
def test_poison_does_not_reach_the_result(nq, window):
    """NaN in every pool element past a length, in the pages wholly below the window's first tile and in the spare
    pages; the table entries of dead pages name a spare NaN page (in range).  Finite, and bitwise the clean run."""
    g, d, page = 2, 256, 128
    cap = pg._max_pages(page) * page
    lens = [cap, 1300, 77, 0, 641]
    Q, K, V, table, _, _ = pg._case(len(lens), g, d, d, nq, page, seed=41 + nq)
    lo64 = np.array([window_ref.window_lo(x, nq, window, cap) // 64 * 64 if window else 0 for x in lens])
    pages = np.arange(table.shape[1])[None, :]
    below = (pages + 1) * page <= lo64[:, None]
    dead_page = below | (pages * page >= np.asarray(lens)[:, None])
    j = np.arange(cap)[None, :]
    dead = np.repeat(np.repeat(below, page, axis=1) | (j >= np.asarray(lens)[:, None]), HK, axis=0)[:, None, :]
    spare = np.setdiff1d(np.arange(table.size + pg.SPARE), table)[0]  # (no sequence owns it)

    def run(poison, tbl):
        k, v = (pg._scatter(np.where(dead, np.float16(poison), x), table, page, table.size + pg.SPARE, poison) for x in (K, V))
        return _wide(g, pg._dev(Q), pg._dev(k), pg._dev(v), tbl, lens, True, window)

    ref = run(0, table)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    assert rg._same(run(np.nan, np.where(dead_page, spare, table).astype(np.int32)), ref)


def test_a_captured_call_follows_lengths_and_table_on_the_device():
    g, nq, d, page, window = 2, 2, 256, 192, 300
    Q, K, V, table, Kp, Vp = pg._case(3, g, d, d, nq, page, seed=81)
    cap = K.shape[2]
    tq, tk, tv = pg._dev(Q).reshape(3, HK * g, d, nq), pg._dev(Kp), pg._dev(Vp)
    tt = torch.tensor(table, dtype=torch.int32, device="cuda:0")
    lens = torch.tensor([cap, 1, 700], dtype=torch.int32, device="cuda:0")
    kw = dict(tail_causal=True, returning_l_m=True, window_size=window)
    fa.paged_1d(tq, tk, tv, tt, lens, **kw)  # (the first launch raises the LDS limit)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fa.paged_1d(tq, tk, tv, tt, lens, **kw)
    lens.copy_(torch.tensor([815, cap, 0], dtype=torch.int32))
    new = np.random.default_rng(90).permutation(table.size + pg.SPARE)[:table.size].reshape(table.shape).astype(np.int32)
    tt.copy_(torch.from_numpy(new))
    for t, x in ((tk, K), (tv, V)):
        t.copy_(torch.from_numpy(pg._scatter(x, new, page, table.size + pg.SPARE)))
    graph.replay()
    torch.cuda.synchronize()
    assert rg._same(out, fa.paged_1d(tq, tk, tv, tt.clone(), lens.clone(), **kw))
    del graph
