"""GPU tests of MLA decode over an FP8 (e4m3fn) latent pool (mla_paged_1d(kv_scale=...)).  The
conversion is exact, so with kv_scale None, 1.0 or 2^e the call is BITWISE the fp16 call on the pool 2^e * decode(byte);
real scales go against ragged_ref.forward_f64 on the dequantized cache.  Unowned pages hold the NaN code 0x7F."""

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import test_gpu_mla as mla
from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

CODES = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)  # every byte but the two NaN codes


def _pool8(K8, table, num_pages):
    """The byte cache [seqs, c, cap] scattered through the table, as test_gpu_mla._case scatters the fp16 one."""
    seqs, c, _ = K8.shape
    pool = np.full((num_pages, c, K8.shape[2] // table.shape[1]), 0x7F, np.uint8)
    pool[table] = K8.reshape(seqs, c, table.shape[1], -1).transpose(0, 2, 1, 3)
    return pool


def _case8(seqs, hq, c, nq, page, seed):
    """test_gpu_mla._case with a cache of random bytes over CODES: subnormals, +-0 and +-448 occur."""
    Q, K, table, pool = mla._case(seqs, hq, c, nq, page, seed)
    K8 = CODES[np.random.default_rng(seed + 2).integers(0, len(CODES), K.shape)]
    return Q, K8, table, _pool8(K8, table, pool.shape[0])


def _call(hq, v, Q, pool, table, lens, tail, kv_scale=None):
    """mla_paged_1d on a uint8 (FP8) or float16 pool; kv_scale a float or None."""
    ts = None if kv_scale is None else mla._t([kv_scale], torch.float32)
    got = fa.mla_paged_1d(mla._t(Q).reshape(len(lens), hq, *Q.shape[1:]), mla._t(pool), mla._t(table, torch.int32),
                          mla._t(lens, torch.int32), v, tail_causal=tail, returning_l_m=True, kv_scale=ts)
    torch.cuda.synchronize()
    return tuple(t.reshape((-1,) + t.shape[2:]) for t in got)


_twin = lambda pool8, e=0: (fp8_ref.decode(pool8) * 2.0 ** e).astype(np.float16)  # noqa: E731  (exact)


@pytest.mark.parametrize("hq,nq,tail", [(16, 1, False), (65, 1, False), (128, 2, True)])
@pytest.mark.parametrize("c,v", [(576, 512), (320, 256), (64, 64)])
@pytest.mark.parametrize("page", [64, 192])
def test_bitwise_twin_of_the_fp16_call(page, c, v, hq, nq, tail):
    Q, K8, table, pool8 = _case8(3, hq, c, nq, page, seed=1000 * c + 10 * hq + nq + page)
    lens = [K8.shape[2], 1300, 77]
    for kv_scale, e in ((None, 0), (1.0, 0), (2.0 ** -8, -8), (2.0 ** 7, 7)):
        assert rg._same(_call(hq, v, Q, pool8, table, lens, tail, kv_scale), _call(hq, v, Q, _twin(pool8, e), table, lens, tail))


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_length_edges_of_the_byte_run(tail):
    hq, nq, c, v, page = 16, 3, 576, 512, 64
    cap = -(-2600 // page) * page
    chunk = mla._plan(nq, cap, c, v, hq, page)[1]
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, chunk - 1, chunk, chunk + 1, cap, cap + 7, -3]
    Q, K8, table, pool8 = _case8(len(lens), hq, c, nq, page, seed=70 + tail)
    assert rg._same(_call(hq, v, Q, pool8, table, lens, tail), _call(hq, v, Q, _twin(pool8), table, lens, tail))


@pytest.mark.parametrize("kv_scale", [2 / 448, 0.3, 200.0])
def test_real_scales_against_the_float64_reference(kv_scale):
    """r != 1 at both ends of the exponent clamp (200: e = 7, r = 1.5625); the doubled scale must fail the gate."""
    hq, nq, c, v, page = 16, 2, 576, 512, 64
    Q, K, table, pool = mla._case(3, hq, c, nq, page, seed=21)
    sc = float(np.float32(kv_scale))
    K8 = fp8_ref.encode(K.astype(np.float64) / sc)
    Kd, pool8, lens = fp8_ref.decode(K8) * sc, _pool8(K8, table, pool.shape[0]), [K.shape[2], 1300, 77]
    res = rg._check_ref(_call(hq, v, Q, pool8, table, lens, True, kv_scale), Q, Kd, Kd[:, :v, :], lens, hq, True)
    print("kv_scale", kv_scale, "worst |error| / allowance:", res)
    if kv_scale == 0.3:
        with pytest.raises(AssertionError):
            rg._check_ref(_call(hq, v, Q, pool8, table, lens, True, 2 * kv_scale), Q, Kd, Kd[:, :v, :], lens, hq, True)


def test_nan_codes_past_the_lengths_and_in_dead_table_entries_are_harmless():
    hq, nq, c, v, page = 16, 2, 576, 512, 64
    Q, K8, table, pool8 = _case8(3, hq, c, nq, page, seed=23)
    lens = [2500, 1300, 77]
    K2, table2 = K8.copy(), table.copy()
    dead = int(np.setdiff1d(np.arange(pool8.shape[0]), table)[0])  # an unowned page: all 0x7F
    for s, n in enumerate(lens):
        K2[s, :, n:] = np.where(np.arange(K2.shape[2] - n) % 2, 0x7F, 0xFF)
        table2[s, -(-n // page):] = dead
    assert (pool8[dead] == 0x7F).all()
    assert rg._same(_call(hq, v, Q, pool8, table, lens, True, 0.3),
                    _call(hq, v, Q, _pool8(K2, table, pool8.shape[0]), table2, lens, True, 0.3))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_an_invalid_scale_gives_nan_and_leaves_no_error(bad):
    Q, K8, table, pool8 = _case8(3, 16, 576, 1, 64, seed=24)
    lens = [K8.shape[2], 1300, 77]
    assert torch.isnan(_call(16, 512, Q, pool8, table, lens, False, bad)[0]).all()
    assert rg._same(_call(16, 512, Q, pool8, table, lens, False, 1.0), _call(16, 512, Q, _twin(pool8), table, lens, False))


def test_graph_replay_of_append_and_attention_after_lengths_table_and_scale_change():
    hq, nq, c, v, page = 16, 2, 576, 512, 64
    Q, K8, table, pool8 = _case8(3, hq, c, nq, page, seed=25)
    tq, tp = mla._t(Q).reshape(3, hq, c, nq), mla._t(pool8)
    tn = mla._t(np.random.default_rng(26).uniform(-2, 2, (3, c, nq)).astype(np.float16))
    tt, tl, ts = mla._t(table, torch.int32), mla._t([2600, 1300, 77], torch.int32), mla._t([0.5], torch.float32)

    def call():
        fa.mla_paged_append_1d(tp, tn, tt, tl, kv_scale=ts)
        return fa.mla_paged_1d(tq, tp, tt, tl, v, tail_causal=True, returning_l_m=True, kv_scale=ts)

    call()  # (warm: the kernel's LDS limit is raised outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    tl.copy_(mla._t([5, 2048, 700], torch.int32))
    tt.copy_(mla._t(table[::-1].copy(), torch.int32))
    ts.fill_(0.3)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert rg._same(out, call())
