"""GPU tests of the FP8 (e4m3fn) K/V cache of the ragged and the paged few-query forwards
(csrc/fa_fwd_f16_decode.h: RaggedCache8 and PagedCache8, fa_forward_ragged_fp8 / fa_forward_paged_fp8, the k_scale /
v_scale arguments of flash_attention.ragged_1d / paged_1d).

The main instrument is bitwise equality with the fp16 twin on the cache converted to fp16 at unit scales: e4m3fn ->
fp16 is exact, the plan, the tiles and the staged LDS image are the same, so an addressing, masking or conversion
error shows without a tolerance.  Real scales go against the float64 reference on the DEQUANTIZED cache under
test_gpu_ragged._check_ref, the project's own fp16 forward gate.  tests/fp8_ref.py is the only source of quantized
data.  Every capacity is test_gpu_paged._max_pages's (about 2600 keys, at least 3 chunks), but the invalid-scale
test's 1344 keys."""

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import test_gpu_paged as pg
from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

HK = pg.HK
SPARE = pg.SPARE
F8 = torch.float8_e4m3fn
FORMS = ["ragged", "paged"]


# ------------------------------------------------------------------ data
def _scatter8(cache, table, page, num_pages, fill=0x7F):
    """test_gpu_paged._scatter for bytes: pages that the table does not name hold ``fill`` (0x7F: NaN)."""
    seqs, max_pages = table.shape
    c = cache.shape[1]
    pool = np.full((num_pages, HK, c, page), fill, np.uint8)
    pool[table] = cache.reshape(seqs, HK, c, max_pages, page).transpose(0, 3, 1, 2, 4)
    return pool


def _f16(b8):
    """the cache converted to fp16 (exact)"""
    return fp8_ref.decode(b8).astype(np.float16)


def _case(seqs, g, d, vd, nq, page, seed, wide=True):
    """Q (fp16), padded K8 / V8 [seqs * HK, c, cap] bytes and a random table.  ``wide``: K is spread over ten binades
    downwards (subnormals of e4m3fn included) and V over sixteen, so every exponent code goes through the conversion."""
    max_pages = pg._max_pages(page)
    cap = max_pages * page
    Q, K, V = rg._np_inputs(seqs * HK, g, d, vd, nq, cap, seed)
    rng = np.random.default_rng(seed + 7)
    if wide:
        K = K.astype(np.float64) * np.exp2(-rng.integers(0, 10, K.shape))
        V = V.astype(np.float64) * np.exp2(rng.integers(-8, 8, V.shape))
    num_pages = seqs * max_pages + SPARE
    table = np.random.default_rng(seed + 1).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    return Q, fp8_ref.encode(K), fp8_ref.encode(V), table


def _dev(x, misalign=False):
    return rg._dev(np.ascontiguousarray(x), misalign)


def _scale_dev(s):
    return None if s is None else torch.tensor(np.asarray(s, dtype=np.float32), device="cuda:0")


def _call8(form, g, Q, K8, V8, table, lens, ks=None, vs=None, tail=False, ws_short=0, fill=None, ws_fill=None, page=None):
    """fa_forward_ragged_fp8 (K8 / V8 padded caches, table unused) or fa_forward_paged_fp8 (K8 / V8 pools) on device
    tensors; ks / vs: device fp32 tensors or None (a null pointer).  Returns (status, O, l, m)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    lens = as_dev(lens)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if form == "ragged":
        vd, cap = V8.shape[1], V8.shape[2]
        prob = rg._problem(nq, cap, d, vd, b)
        need = int(L.fa_forward_ragged_workspace_bytes(prob, g))
    else:
        num_pages, hk, vd, pg_ = V8.shape
        page = pg_ if page is None else page
        table = as_dev(table)
        max_pages = table.shape[-1]
        prob = pg._problem(nq, max_pages * page, d, vd, b)
        need = int(L.fa_forward_paged_workspace_bytes(prob, g, page))
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O_, l, m):
            t.view(torch.uint8).fill_(fill)
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    stream = torch.cuda.current_stream().cuda_stream
    if form == "ragged":
        st = L.fa_forward_ragged_fp8(stream, prob, g, Q.data_ptr(), K8.data_ptr(), V8.data_ptr(), ptr(ks), ptr(vs),
                                     lens.data_ptr(), HK, int(tail), O_.data_ptr(), l.data_ptr(), m.data_ptr(),
                                     ws.data_ptr(), max(need - ws_short, 0))
    else:
        st = L.fa_forward_paged_fp8(stream, prob, g, Q.data_ptr(), K8.data_ptr(), V8.data_ptr(), ptr(ks), ptr(vs),
                                    table.data_ptr(), max_pages, page, num_pages, lens.data_ptr(), HK, int(tail),
                                    O_.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0))
    torch.cuda.synchronize()
    return st, O_, l, m


def _twin(form, g, Q, K16, V16, table, lens, tail=False):
    """the fp16 forward of the same form on fp16 device tensors"""
    if form == "ragged":
        st, *out = rg._abi(g, Q, K16, V16, lens, kv_per_len=HK, tail=tail)
    else:
        st, *out = pg._abi(g, Q, K16, V16, table, lens, tail=tail)
    assert st == 0
    return out


def _stores(form, K8, V8, table, page, fill=0x7F):
    """what the form reads: the padded caches, or the pools scattered through the table"""
    if form == "ragged":
        return K8, V8
    num_pages = table.size + SPARE
    return _scatter8(K8, table, page, num_pages, fill), _scatter8(V8, table, page, num_pages, fill)


# ------------------------------------------------------------------ 1. unit scales are the fp16 forward, bit for bit
@pytest.mark.parametrize("g,nq", [(1, 1), (8, 1), (3, 3), (2, 64)])
@pytest.mark.parametrize("d,vd", [(128, 128), (64, 64), (32, 32), (96, 40), (8, 8)])
@pytest.mark.parametrize("page", [64, 192])
@pytest.mark.parametrize("form", FORMS)
def test_unit_scales_are_bitwise_the_fp16_forward_on_the_converted_cache(form, page, d, vd, g, nq):
    """Both stagings (8-byte at d == v_d in {32, 64, 128}, element-wise otherwise and with the caches offset by one
    byte), every D instance, several pitches of the fold; scales null, and 1.0 read from a device array."""
    Q, K8, V8, table = _case(3, g, d, vd, nq, page, seed=1000 * d + 10 * g + nq + page)
    cap = K8.shape[2]
    assert pg._plan(nq, cap, d, vd, g, page)[0] >= 3
    lens = [cap, 1300, 77]
    k8, v8 = _stores(form, K8, V8, table, page)
    tq, ones = _dev(Q), _scale_dev(np.ones(HK))
    for misalign in (False, True):
        tk, tv = _dev(k8, misalign), _dev(v8, misalign)
        ref = _twin(form, g, tq, _dev(_f16(k8), misalign), _dev(_f16(v8), misalign), table, lens)
        for ks, vs in ((None, None), (ones, ones)):
            st, *got = _call8(form, g, tq, tk, tv, table, lens, ks, vs)
            assert st == 0
            assert rg._same(got, ref), (misalign, ks is None, vs is None)


# ------------------------------------------------------------------ 2. length edges
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("nq", [1, 4, 33])
@pytest.mark.parametrize("page", [64, 192])
@pytest.mark.parametrize("form", FORMS)
def test_lengths_at_chunk8_page_tile_and_chunk_edges(form, page, nq, tail):
    g, d = (1 if nq == 33 else 2), 64
    cap = pg._max_pages(page) * page
    chunks, chunk = pg._plan(nq, cap, d, d, g, page)[:2]
    assert chunks >= 3
    lens = [0, 1, 7, 8, 9, 63, 64, 65, page - 1, page, page + 1, chunk - 1, chunk, chunk + 1, cap - 1, cap, cap + 7]
    Q, K8, V8, table = _case(len(lens), g, d, d, nq, page, seed=page + nq)
    k8, v8 = _stores(form, K8, V8, table, page)
    tq = _dev(Q)
    st, *got = _call8(form, g, tq, _dev(k8), _dev(v8), table, lens, tail=tail)
    assert st == 0
    assert rg._same(got, _twin(form, g, tq, _dev(_f16(k8)), _dev(_f16(v8)), table, lens, tail))
    rg._check_empty(got, np.repeat(np.asarray(lens) == 0, HK * g)[:, None] & np.ones((1, nq), bool))


# ------------------------------------------------------------------ 3. real scales
K_SCALE = [0.037, 2.0 ** -12 * 1.37]   # e = -5 inside the clamp; e = -12 clamped to -8
V_SCALE = [300.0, 0.0123]


def _real_case(form, d, g, tail, k_scale, v_scale, seed):
    """True K, V ~ U(-2, 2) quantized per head with the scales; the call with ``k_scale`` / ``v_scale``; and what
    _check_ref needs: the dequantized float64 caches."""
    nq, page = 4, 192
    Q, _, _, table = _case(3, g, d, d, nq, page, seed, wide=False)
    cap = table.shape[1] * page
    _, K, V = rg._np_inputs(3 * HK, g, d, d, nq, cap, seed)
    byhead = lambda x: x.reshape(3, HK, d, cap)  # noqa: E731
    K8 = fp8_ref.quantize(byhead(K), K_SCALE, 1).reshape(K.shape)
    V8 = fp8_ref.quantize(byhead(V), V_SCALE, 1).reshape(V.shape)
    Kd = fp8_ref.dequantize(byhead(K8), K_SCALE, 1).reshape(K.shape)
    Vd = fp8_ref.dequantize(byhead(V8), V_SCALE, 1).reshape(V.shape)
    lens = [cap, 3, 1000]
    k8, v8 = _stores(form, K8, V8, table, page)
    st, *got = _call8(form, g, _dev(Q), _dev(k8), _dev(v8), table, lens, _scale_dev(k_scale), _scale_dev(v_scale), tail=tail)
    assert st == 0
    return got, Q, Kd, Vd, np.repeat(lens, HK)


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("d", [64, 128, 40])
@pytest.mark.parametrize("form", FORMS)
def test_real_scales_against_the_float64_reference_on_the_dequantized_cache(form, d, g, tail):
    """Non-power-of-two per-head scales (so the split k_scale = 2^e * r has r != 1, with e inside the clamp for head 0
    and at its lower end for head 1) under the fp16 forward gate, no new tolerance: the dequantized cache is exact
    in fp16 up to the power of two, and the remaining factor goes into the fp32 pre-scale of Q."""
    got, Q, Kd, Vd, kv_lens = _real_case(form, d, g, tail, K_SCALE, V_SCALE, seed=300 + d + g)
    res = rg._check_ref(got, Q, Kd, Vd, kv_lens, g, tail)
    print(f"{form} d={d} g={g} tail={tail}: worst error / allowance {res}")


@pytest.mark.parametrize("form", FORMS)
def test_the_gate_sees_a_wrong_scale(form):
    """The same call with k_scale doubled must fail _check_ref: the gate is not satisfied by any scale."""
    got, Q, Kd, Vd, kv_lens = _real_case(form, 64, 4, False, [2 * s for s in K_SCALE], V_SCALE, seed=368)
    with pytest.raises(AssertionError):
        rg._check_ref(got, Q, Kd, Vd, kv_lens, 4, False)
    got, Q, Kd, Vd, kv_lens = _real_case(form, 64, 4, False, K_SCALE, [2 * s for s in V_SCALE], seed=368)
    with pytest.raises(AssertionError):
        rg._check_ref(got, Q, Kd, Vd, kv_lens, 4, False)


@pytest.mark.parametrize("form", FORMS)
def test_the_upper_end_of_the_exponent_clamp(form):
    """k_scale = 200 (e = 8 clamped to 7, r = 1.5625) and 2^7 exactly (e = 7, r = 1), against the reference."""
    nq, page, d, g = 4, 192, 64, 4
    ks = [200.0, 128.0]
    Q, _, _, table = _case(2, g, d, d, nq, page, seed=77, wide=False)
    cap = table.shape[1] * page
    _, K, V = rg._np_inputs(2 * HK, g, d, d, nq, cap, 77)
    K8 = fp8_ref.quantize(K.reshape(2, HK, d, cap), ks, 1).reshape(K.shape)
    Kd = fp8_ref.dequantize(K8.reshape(2, HK, d, cap), ks, 1).reshape(K.shape)
    V8 = fp8_ref.encode(V)
    lens = [cap, 700]
    k8, v8 = _stores(form, K8, V8, table, page)
    st, *got = _call8(form, g, _dev(Q), _dev(k8), _dev(v8), table, lens, _scale_dev(ks), None)
    assert st == 0
    rg._check_ref(got, Q, Kd, fp8_ref.decode(V8), np.repeat(lens, HK), g, False)


# ------------------------------------------------------------------ 4. poison
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("misalign", [False, True], ids=["fast", "elementwise"])
@pytest.mark.parametrize("form", FORMS)
def test_bytes_past_the_length_and_unowned_pages_do_not_reach_the_result(form, misalign, tail):
    """Bytes past each length and pages that no sequence owns are 0x7F / 0xFF (the NaN codes) or 0x7E (448), the
    workspace is 0xFF bytes and the outputs are pre-filled: bitwise the call with zero bytes there."""
    g, nq, d, page = 4, 4, 64, 192
    Q, K8, V8, table = _case(3, g, d, d, nq, page, seed=41)
    cap = K8.shape[2]
    lens = [1, 577, cap - 1]
    past = np.arange(cap)[None, None, :] >= np.repeat(lens, HK)[:, None, None]
    ks, vs = _scale_dev([0.5, 3.0]), _scale_dev([1.25, 0.01])
    tq = _dev(Q)

    def run(byte):
        k8, v8 = _stores(form, np.where(past, np.uint8(byte), K8), np.where(past, np.uint8(byte), V8), table, page, byte)
        st, *out = _call8(form, g, tq, _dev(k8, misalign), _dev(v8, misalign), table, lens, ks, vs, tail=tail,
                          fill=0x5A, ws_fill=0xFF)
        assert st == 0
        return out

    ref = run(0x00)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    for byte in (0x7F, 0xFF, 0x7E):
        assert rg._same(run(byte), ref), hex(byte)


@pytest.mark.parametrize("page", [64, 192])
def test_entries_of_pages_without_a_live_key_are_never_read(page):
    g, nq, d = 4, 4, 64
    Q, K8, V8, table = _case(3, g, d, d, nq, page, seed=31)
    max_pages = table.shape[1]
    lens = np.array([0, page, page + 1])
    dead = np.arange(max_pages)[None, :] >= -(-lens // page)[:, None]
    k8, v8 = _stores("paged", K8, V8, table, page)
    tq, tk, tv = _dev(Q), _dev(k8), _dev(v8)
    for tail in (False, True):
        st, *ref = _call8("paged", g, tq, tk, tv, np.where(dead, 0, table), lens, tail=tail)
        assert st == 0
        for junk in (pg.INT32_MIN, -1, pg.INT32_MAX):
            st, *got = _call8("paged", g, tq, tk, tv, np.where(dead, junk, table).astype(np.int32), lens, tail=tail)
            assert st == 0
            assert rg._same(got, ref), junk


# ------------------------------------------------------------------ 5. graph replay
def test_a_captured_call_follows_lengths_table_and_scales_on_the_device():
    """One paged_1d call with an FP8 cache captured in a graph.  Between replays k_lens, block_table, k_scale and
    v_scale are overwritten in place (the pools' pages move with the table): every replay is bitwise the eager call
    on the same state."""
    g, nq, d, page = 4, 4, 64, 192
    Q, K8, V8, table = _case(3, g, d, d, nq, page, seed=81)
    num_pages, cap = table.size + SPARE, K8.shape[2]
    tq = _dev(Q).reshape(3, HK * g, d, nq)
    k8, v8 = _stores("paged", K8, V8, table, page)
    tk, tv = _dev(k8).view(F8), _dev(v8).view(F8)
    tt = torch.tensor(table, dtype=torch.int32, device=tq.device)
    lens = torch.tensor([cap, 1, 700], dtype=torch.int32, device=tq.device)
    ks, vs = _scale_dev([1.0, 1.0]), _scale_dev([1.0, 1.0])
    for tail in (False, True):
        fa.paged_1d(tq, tk, tv, tt, lens, tail_causal=tail, k_scale=ks, v_scale=vs)  # (first launches raise the LDS limit)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fa.paged_1d(tq, tk, tv, tt, lens, tail_causal=tail, returning_l_m=True, k_scale=ks, v_scale=vs)
        for i, (now, k_now, v_now) in enumerate((([5, cap, 0], [0.037, 3.0], [300.0, 0.5]),
                                                 ([513, 64, cap - 1], [1.0, 1.0], [1.0, 1.0]),
                                                 ([77, 77, 1024], [2.0 ** -12 * 1.37, 200.0], [0.0123, 7.0]))):
            lens.copy_(torch.tensor(now, dtype=torch.int32))
            ks.copy_(torch.tensor(k_now))
            vs.copy_(torch.tensor(v_now))
            new = np.random.default_rng(90 + i).permutation(num_pages)[:table.size].reshape(table.shape).astype(np.int32)
            tt.copy_(torch.from_numpy(new))
            tk.view(torch.uint8).copy_(torch.from_numpy(_scatter8(K8, new, page, num_pages)))
            tv.view(torch.uint8).copy_(torch.from_numpy(_scatter8(V8, new, page, num_pages)))
            graph.replay()
            torch.cuda.synchronize()
            eager = fa.paged_1d(tq, tk.clone(), tv.clone(), tt.clone(), lens.clone(), tail_causal=tail, returning_l_m=True,
                                k_scale=ks.clone(), v_scale=vs.clone())
            torch.cuda.synchronize()
            assert rg._same(out, eager), now
            if k_now == [1.0, 1.0]:  # and the eager call is the fp16 forward on the converted pools
                twin = fa.paged_1d(tq, _dev(_f16(_scatter8(K8, new, page, num_pages))), _dev(_f16(_scatter8(V8, new, page, num_pages))),
                                   tt, lens, tail_causal=tail, returning_l_m=True)
                torch.cuda.synchronize()
                assert rg._same(out, twin)
        del graph


# ------------------------------------------------------------------ 6. determinism, batch independence, the wrappers
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("form", FORMS)
def test_two_calls_are_equal_and_a_sequence_does_not_depend_on_the_batch(form, tail):
    g, nq, d, vd, page = 2, 5, 96, 40, 192
    Q, K8, V8, table = _case(3, g, d, vd, nq, page, seed=51)
    cap = K8.shape[2]
    lens = [2 * page + 9, cap, 40]
    ks, vs = _scale_dev([0.3, 1.7]), _scale_dev([2.5, 0.04])
    k8, v8 = _stores(form, K8, V8, table, page)
    tq, tk, tv = _dev(Q), _dev(k8), _dev(v8)
    st0, *a = _call8(form, g, tq, tk, tv, table, lens, ks, vs, tail=tail)
    st1, *b = _call8(form, g, tq, tk, tv, table, lens, ks, vs, tail=tail, ws_fill=0xFF)
    assert st0 == 0 and st1 == 0
    assert rg._same(a, b)
    q1 = slice(HK * g, 2 * HK * g)
    alone_k, alone_v = (tk, tv) if form == "paged" else (tk[HK:2 * HK].contiguous(), tv[HK:2 * HK].contiguous())
    st2, *alone = _call8(form, g, tq[q1].contiguous(), alone_k, alone_v, table[1:2], lens[1:2], ks, vs, tail=tail)
    assert st2 == 0
    assert rg._same([t[q1] for t in a], alone)
    # the wrapper is the ABI call, with the cache as float8_e4m3fn and as uint8
    tl = torch.tensor(lens, dtype=torch.int32, device=tq.device)
    tt = torch.tensor(table, dtype=torch.int32, device=tq.device)
    Qw = tq.reshape(3, HK * g, d, nq)
    for view in (lambda t: t, lambda t: t.view(F8)):
        if form == "ragged":
            got = fa.ragged_1d(Qw, view(tk).reshape(3, HK, d, cap), view(tv).reshape(3, HK, vd, cap), tl, tail_causal=tail,
                               returning_l_m=True, k_scale=ks, v_scale=vs)
        else:
            got = fa.paged_1d(Qw, view(tk), view(tv), tt, tl, tail_causal=tail, returning_l_m=True, k_scale=ks, v_scale=vs)
        torch.cuda.synchronize()
        assert rg._same([t.reshape(r.shape) for t, r in zip(got, a)], a)


# ------------------------------------------------------------------ 7. ABI statuses
@pytest.mark.parametrize("form", FORMS)
def test_short_workspace_is_rejected_and_nothing_is_written(form):
    Q, K8, V8, table = _case(2, 4, 64, 64, 8, 64, seed=71)
    k8, v8 = _stores(form, K8, V8, table, 64)
    st, *out = _call8(form, 4, _dev(Q), _dev(k8), _dev(v8), table, [2600, 100], ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


def test_a_page_of_32_keys_is_unsupported_and_nothing_is_written():
    Q, K8, V8, table = _case(2, 4, 64, 64, 8, 64, seed=72)
    k8, v8 = _stores("paged", K8, V8, table, 64)
    table32 = np.stack([2 * table, 2 * table + 1], axis=-1).reshape(2, -1).astype(np.int32)
    st, *out = _call8("paged", 4, _dev(Q), _dev(k8), _dev(v8), table32, [2600, 100], fill=0x5A, page=32)
    assert st == _lib.FA_ERR_UNSUPPORTED and "page % 64" in _lib.last_error()
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_batch_is_ok(form):
    L = _lib.lib()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    prob = rg._problem(4, 2624, 64, 64, 0)
    if form == "ragged":
        st = L.fa_forward_ragged_fp8(stream, prob, 4, None, None, None, None, None, None, HK, 0, None, None, None,
                                     ws.data_ptr(), int(L.fa_forward_ragged_workspace_bytes(prob, 4)))
    else:
        st = L.fa_forward_paged_fp8(stream, prob, 4, None, None, None, None, None, None, 41, 64, 8, None, HK, 0, None,
                                    None, None, ws.data_ptr(), int(L.fa_forward_paged_workspace_bytes(prob, 4, 64)))
    assert st == _lib.FA_OK


# ------------------------------------------------------------------ 8. invalid scales
BAD_SCALES = [0.0, -0.0, -1.0, float("inf"), float("nan")]


@pytest.mark.parametrize("window", [0, 300], ids=["tail", "w300"])
@pytest.mark.parametrize("form", FORMS)
def test_an_invalid_scale_gives_nan_in_its_own_head_only(form, window):
    """include/fa_api.h: "A scale must be finite and positive; any other value gives NaN output".  2 sequences x 2 K/V
    heads, g = 2, nq = 4, d = v_d = 64, a capacity of 1344 keys (three chunks), lengths (1344, 700); the un-windowed
    tail form and W = 300.  0.0, -0.0, -1.0, +Inf and NaN in k_scale[1] and, separately, in v_scale[1]: O of every
    (live) row of head 1 is NaN in every channel, the rows of head 0 are bitwise the clean call, and no call leaves
    an error behind.  A positive subnormal scale is valid: finite output."""
    from tests import test_gpu_window as gw
    g, nq, d, page, seqs = 2, 4, 64, 64, 2
    max_pages = 21
    cap = page * max_pages
    lens = [cap, 700]
    Q, K, V = rg._np_inputs(seqs * HK, g, d, d, nq, cap, seed=91)
    K8, V8 = fp8_ref.encode(K), fp8_ref.encode(V)
    num_pages = seqs * max_pages + SPARE
    table = np.random.default_rng(92).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    k8, v8 = _stores(form, K8, V8, table, page)
    tq, tk, tv = _dev(Q), _dev(k8), _dev(v8)
    if window:
        assert gw._plan(nq, cap, d, d, g, window, page if form == "paged" else None)[6] == 0

    def call(ks, vs):
        ks, vs = _scale_dev(ks), _scale_dev(vs)
        if window:
            st, *out = gw._win(form, g, tq, tk, tv, table, lens, window, fp8=True, ks=ks, vs=vs)
        else:
            st, *out = _call8(form, g, tq, tk, tv, table, lens, ks, vs, tail=True)
        assert st == 0, _lib.last_error()
        return out

    clean_k, clean_v = [0.3, 1.7], [2.5, 0.04]
    clean = call(clean_k, clean_v)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    head = (np.arange(seqs * HK * g) // g) % HK                   # the K/V head of every Q slice
    h0, h1 = (torch.from_numpy(np.nonzero(head == h)[0]).to(tq.device) for h in (0, 1))
    for bad in BAD_SCALES:
        for which, (ks, vs) in (("k_scale", ([clean_k[0], bad], clean_v)), ("v_scale", (clean_k, [clean_v[0], bad]))):
            got = call(ks, vs)
            assert rg._same([t[h0] for t in got], [t[h0] for t in clean]), (which, bad, "head 0 moved")
            o1 = got[0][h1].float()
            assert bool(torch.isnan(o1).all()), (which, bad, f"{int((~torch.isnan(o1)).sum())} of {o1.numel()} outputs of "
                                                 f"head 1 are not NaN; finite max |O| {float(torch.nan_to_num(o1).abs().max())}")
    tiny = float(np.float32(1e-40))                               # a positive subnormal float32
    for ks, vs in (([clean_k[0], tiny], clean_v), (clean_k, [clean_v[0], tiny])):
        got = call(ks, vs)
        assert all(bool(torch.isfinite(t.float()).all()) for t in got)
        assert rg._same([t[h0] for t in got], [t[h0] for t in clean])
