"""GPU tests of query-blocked and tree-masked MLA attention over the paged latent cache
(csrc/fa_fwd_f16_mla_prefill.hip, fa_forward_mla_paged_prefill, flash_attention.mla_paged_prefill_1d).

The references are tests/ragged_ref.forward_f64 and tests/tree_ref.forward_f64 on the cache gathered through the table,
V = K[:, :v, :] and g = Hq, under test_gpu_ragged._check_ref / test_gpu_tree._check_tree (the fp16 forward gate).
Caches are test_gpu_mla._case's: about 2600 keys, scattered through a random table, unowned pool pages NaN."""

import ctypes

import numpy as np
import pytest
import torch

from tests import fp8_ref, tree_ref
from tests import test_gpu_mla as mla
from tests import test_gpu_mla_fp8 as mla8
from tests import test_gpu_ragged as rg
from tests import test_gpu_tree as tree
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu
_t = mla._t


def _plan(nq, cap, c, v, hq, page):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_mla_paged_prefill_plan(mla._problem(nq, cap, c, v, hq), hq, page, out) == 0
    return tuple(out)


def _call(hq, v, Q, pool, table, lens, tail, mask=None, kv_scale=None, fn=fa.mla_paged_prefill_1d):
    """The wrapper on numpy inputs (Q [seqs * hq, c, nq]); returns (O [b, v, nq], l, m)."""
    kw = {} if mask is None else {"draft_mask": _t(np.asarray(mask).view(np.int32))}
    ts = None if kv_scale is None else _t([kv_scale], torch.float32)
    got = fn(_t(Q).reshape(len(lens), hq, *Q.shape[1:]), _t(pool), _t(table, torch.int32), _t(lens, torch.int32), v,
             tail_causal=tail, returning_l_m=True, kv_scale=ts, **kw)
    torch.cuda.synchronize()
    return tuple(t.reshape((-1,) + t.shape[2:]) for t in got)


@pytest.mark.parametrize("hq,nq,tail", [(128, 5, True), (16, 33, True), (65, 9, True), (16, 40, False), (1, 70, True)])
@pytest.mark.parametrize("c,v", [(576, 512), (64, 64)])
@pytest.mark.parametrize("page", [64, 192])
def test_parity_with_the_float64_reference(page, c, v, hq, nq, tail):
    """Two head blocks a query, nine query blocks with a ragged last one, a ragged head block, the non-causal rule,
    P_b = 64; length 3 gives rows before position 0."""
    Q, K, table, pool = mla._case(4, hq, c, nq, page, seed=1000 * c + 10 * hq + nq + page)
    cap = K.shape[2]
    plan = _plan(nq, cap, c, v, hq, page)
    assert plan[3] >= 2 and -(-cap // plan[1]) >= 2
    lens = [cap, 1300, 77, 3]
    res = rg._check_ref(_call(hq, v, Q, pool, table, lens, tail), Q, K, K[:, :v, :], lens, hq, tail)
    print("worst |error| / allowance:", res)


def test_block_ends_at_tile_chunk_and_query_edges():
    hq, nq, c, v, page = 16, 33, 576, 512, 64
    cap = -(-2600 // page) * page
    chunk = _plan(nq, cap, c, v, hq, page)[1]
    lens = [nq - 1, nq, 64, 65, chunk - 1, chunk, chunk + 1, chunk + nq - 1, cap]
    Q, K, table, pool = mla._case(len(lens), hq, c, nq, page, seed=33)
    res = rg._check_ref(_call(hq, v, Q, pool, table, lens, True), Q, K, K[:, :v, :], lens, hq, True)
    print("worst |error| / allowance:", res)


@pytest.mark.parametrize("hq,nq", [(128, 8), (16, 64), (16, 128)])
def test_masks_against_the_tree_reference(monkeypatch, hq, nq):
    """A random forest from draft_mask_from_parents and random bits (bits above the diagonal, unused bits set), lengths
    below Nq among them; the lower triangle is bitwise the unmasked tail call."""
    monkeypatch.setattr(tree, "HK", 1)  # (_check_tree's mask index: one K/V head a sequence)
    c, v, page = 576, 512, 64
    rng = np.random.default_rng(nq + hq)
    Q, K, table, pool = mla._case(4, hq, c, nq, page, seed=5 * nq + hq)
    lens = [K.shape[2], 1300, nq - 3, 2]
    parents = np.stack([[rng.integers(-1, i) for i in range(nq)] for _ in lens])
    forest = fa.draft_mask_from_parents(_t(parents)).cpu().numpy().view(np.uint32)
    assert (forest == tree_ref.pack_mask(tree_ref.ancestors(parents))).all()
    for masks in (forest, tree._masks(["random"] * len(lens), nq, rng)):
        res = tree._check_tree(_call(hq, v, Q, pool, table, lens, True, masks), Q, K, K[:, :v, :], lens, masks, hq)
        print("worst |error| / allowance:", res)
    chain = np.broadcast_to(tree_ref.lower_triangle(nq), forest.shape).copy()
    assert rg._same(_call(hq, v, Q, pool, table, lens, True, chain), _call(hq, v, Q, pool, table, lens, True))


def test_inside_the_decode_envelope_the_call_is_mla_paged_1d():
    Q, K, table, pool = mla._case(3, 16, 576, 3, 64, seed=41)
    lens = [2600, 1300, 2]
    assert rg._same(_call(16, 512, Q, pool, table, lens, True),
                    _call(16, 512, Q, pool, table, lens, True, fn=fa.mla_paged_1d))


@pytest.mark.parametrize("masked", [False, True], ids=["tail", "mask"])
def test_an_fp8_pool(masked):
    """kv_scale None and 2^-3: bitwise the fp16 call on the dequantized pool.  0.3: the float64 reference on the
    dequantized cache.  NaN codes past the lengths and behind dead table entries change nothing."""
    hq, nq, c, v, page = 16, 33, 576, 512, 64
    Q, K8, table, pool8 = mla8._case8(3, hq, c, nq, page, seed=51)
    lens = [K8.shape[2], 1300, 7]
    mask = tree._masks(["forest"] * 3, nq, np.random.default_rng(5)) if masked else None
    for kv_scale, e in ((None, 0), (2.0 ** -3, -3)):
        assert rg._same(_call(hq, v, Q, pool8, table, lens, True, mask, kv_scale),
                        _call(hq, v, Q, mla8._twin(pool8, e), table, lens, True, mask))
    K2, table2 = K8.copy(), table.copy()
    dead = int(np.setdiff1d(np.arange(pool8.shape[0]), table)[0])  # an unowned page: all 0x7F
    for s, n in enumerate(lens):
        K2[s, :, n:] = np.where(np.arange(K2.shape[2] - n) % 2, 0x7F, 0xFF)  # the two NaN codes
        table2[s, -(-n // page):] = dead
    assert rg._same(_call(hq, v, Q, pool8, table, lens, True, mask, 0.3),
                    _call(hq, v, Q, mla8._pool8(K2, table, pool8.shape[0]), table2, lens, True, mask, 0.3))
    if not masked:
        Q, K, table, pool = mla._case(3, hq, c, nq, page, seed=52)
        sc = float(np.float32(0.3))
        K8 = fp8_ref.encode(K.astype(np.float64) / sc)
        Kd = fp8_ref.decode(K8) * sc
        got = _call(hq, v, Q, mla8._pool8(K8, table, pool.shape[0]), table, lens, True, None, 0.3)
        print("worst |error| / allowance:", rg._check_ref(got, Q, Kd, Kd[:, :v, :], lens, hq, True))


def test_inf_past_the_lengths_of_an_fp16_pool_is_harmless():
    hq, nq, page = 128, 5, 64
    Q, K, table, pool = mla._case(3, hq, 576, nq, page, seed=61)
    lens = [2500, 1300, 3]
    K2 = K.copy()
    for s, n in enumerate(lens):
        K2[s, :, n:] = np.where(np.arange(K2.shape[2] - n) % 2, np.nan, np.inf)
    pool2 = pool.copy()
    pool2[table] = K2.reshape(3, 576, -1, page).transpose(0, 2, 1, 3)
    assert rg._same(_call(hq, 512, Q, pool, table, lens, True), _call(hq, 512, Q, pool2, table, lens, True))


def test_graph_replay_after_lengths_table_mask_and_scale_change():
    hq, nq, c, v = 16, 8, 576, 512
    Q, K8, table, pool8 = mla8._case8(3, hq, c, nq, 64, seed=71)
    rng = np.random.default_rng(72)
    masks = [tree._masks(["random"] * 3, nq, rng).view(np.int32) for _ in range(2)]
    tq, tp = _t(Q).reshape(3, hq, c, nq), _t(pool8)
    tt, tl, tm, ts = _t(table, torch.int32), _t([2600, 1300, 77], torch.int32), _t(masks[0]), _t([0.3], torch.float32)
    call = lambda: fa.mla_paged_prefill_1d(tq, tp, tt, tl, v, tail_causal=True, returning_l_m=True,  # noqa: E731
                                           kv_scale=ts, draft_mask=tm)
    call()  # (warm: the kernel's LDS limit is raised outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    tl.copy_(_t([5, 2048, 700], torch.int32))
    tt.copy_(_t(table[::-1].copy(), torch.int32))
    tm.copy_(_t(masks[1]))
    ts.copy_(_t([0.7], torch.float32))
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert rg._same(out, call())
