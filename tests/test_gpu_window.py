"""GPU tests of sliding-window decode (csrc/fa_fwd_f16_window*.hip, fa_forward_ragged_window / fa_forward_paged_window
and their FP8 forms, the window_size keyword of ragged_1d / paged_1d): the nq queries are the last nq
positions of a sequence of L keys, query i at pos = L - nq + i sees the W keys [max(0, pos - W + 1), pos].

Against tests/window_ref.py (checked against the oracle by tests/test_window_ref.py) the rule is
tests.test_gpu_ragged._check_ref's, restated in _check_window with the window's mask in place of the ragged one: no
new tolerance.  Random inputs hide an off-by-one edge once W is in the hundreds, so the same check also runs on
window_ref's beacon inputs, on which tests/test_window_ref.py shows either edge moved by one key to be > 100 x the
allowance.  The paged / FP8 / delegation / batch / poison / graph tests are bitwise.  Sizes are the decode tests':
a capacity of about 2600 keys, Hk = 2, inputs from test_gpu_ragged._np_inputs."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import gate
from tests import test_gpu_paged as pg
from tests import test_gpu_parity as parity
from tests import test_gpu_ragged as rg
from tests import window_ref
from tests.gate import TOL
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

HK, SPARE = pg.HK, pg.SPARE
FORMS = ["ragged", "paged"]
F8 = torch.float8_e4m3fn
PITCH = {1: 1, 4: 4, 33: 64}


# ------------------------------------------------------------------ calls
def _plan(nq, cap, d, vd, g, window, page=None):
    out = (ctypes.c_int32 * 8)()
    p = rg._problem(nq, cap, d, vd, g)
    L = _lib.lib()
    st = L.fa_forward_ragged_window_plan(p, g, window, out) if page is None else \
        L.fa_forward_paged_window_plan(p, g, page, window, out)
    assert st == 0
    return tuple(out)


def _dev(x, misalign=False):
    return rg._dev(np.ascontiguousarray(x), misalign)


def _scale_dev(s):
    return None if s is None else torch.tensor(np.asarray(s, dtype=np.float32), device="cuda:0")


def _win(form, g, Q, K, V, table, lens, window, fp8=False, ks=None, vs=None, ws_short=0, fill=None, ws_fill=None,
         page=None):
    """The windowed entry point of ``form`` (fp8: its FP8 twin) on device tensors: K / V the padded caches [bkv, c, cap]
    (table unused) or the pools [num_pages, HK, c, page]; lens (and table) device int32 tensors, arrays or lists, one
    length per sequence of HK heads.  Returns (status, O, l, m)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    lens = as_dev(lens)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if form == "ragged":
        vd, cap = V.shape[1], V.shape[2]
        prob = rg._problem(nq, cap, d, vd, b)
        need = int(L.fa_forward_ragged_window_workspace_bytes(prob, g, window))
    else:
        num_pages, hk, vd, pg_ = V.shape
        page = pg_ if page is None else page
        table = as_dev(table)
        max_pages = table.shape[-1]
        prob = pg._problem(nq, max_pages * page, d, vd, b)
        need = int(L.fa_forward_paged_window_workspace_bytes(prob, g, page, window))
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
    sc = [ptr(ks), ptr(vs)] if fp8 else []
    out = [O_.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0)]
    if form == "ragged":
        fn = L.fa_forward_ragged_window_fp8 if fp8 else L.fa_forward_ragged_window
        st = fn(stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), *sc, lens.data_ptr(), HK, window, *out)
    else:
        fn = L.fa_forward_paged_window_fp8 if fp8 else L.fa_forward_paged_window
        st = fn(stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), *sc, table.data_ptr(), max_pages, page,
                num_pages, lens.data_ptr(), HK, window, *out)
    torch.cuda.synchronize()
    return st, O_, l, m


def _ok(*a, **kw):
    st, *out = _win(*a, **kw)
    assert st == 0, _lib.last_error()
    return out


def _stores(form, K, V, table, page, fill=np.nan):
    """what the form reads: the padded caches, or the pools scattered through the table"""
    if form == "ragged":
        return K, V
    num_pages = table.size + SPARE
    if K.dtype == np.uint8:
        def scatter(x):
            pool = np.full((num_pages, HK, x.shape[1], page), fill, np.uint8)
            pool[table] = x.reshape(table.shape[0], HK, x.shape[1], table.shape[1], page).transpose(0, 3, 1, 2, 4)
            return pool
        return scatter(K), scatter(V)
    return pg._scatter(K, table, page, num_pages, fill), pg._scatter(V, table, page, num_pages, fill)


# ------------------------------------------------------------------ the gate: _check_ref's rule with the window's mask
def _check_window(got, Q, K, V, kv_lens, g, window):
    """Against tests/window_ref.py under test_gpu_ragged._check_ref's rule: O and l within TOL[float16]['fwd'] (l
    relative to the stored m), m within 2 ulp plus the larger of 1e-3 * max(|m|, 1) and
    (2^-11 + d 2^-24) * max_j sum_c |q_c k_jc| / sqrt(d) + 4.9e-4 over the keys of the WINDOW; rows without a key
    exactly O = 0, l = 0, m = bytes 0xFA.  Returns the worst |error| / allowance of O, l and m."""
    O64, L64, M64, ha = window_ref.forward_f64(Q, K, V, kv_lens, window, g)
    o, l, m = (t.cpu().numpy() for t in got)
    b, d, nq = Q.shape
    cap = K.shape[2]
    rtol, atol = TOL[np.float16]["fwd"]
    rg._check_empty(got, ~ha)
    live = ha[:, None, :] & np.ones_like(O64, bool)
    assert np.isfinite(o.astype(np.float64)).all()
    parity._close("O", np.where(live, o, 0.0), O64, rtol, atol)
    res = {"O": float((np.abs(np.where(live, o, 0.0) - O64) / gate.plain_bound(O64, rtol, atol)).max())}
    if not ha.any():
        return res
    m_f, M = m.astype(np.float64)[ha], M64[ha]
    rowdot = np.zeros((b, nq))
    for bi in range(b):
        mask = window_ref.window_mask(nq, cap, kv_lens[bi // g], window)
        rowdot[bi] = gate.max_abs_dot(Q[bi][None], K[bi // g][None], mask)[0] / math.sqrt(d)
    ulp = np.abs(np.spacing(np.abs(M).astype(np.float16))).astype(np.float64)
    m_tol = 2 * ulp + np.maximum(1e-3 * np.maximum(np.abs(M), 1.0), (2.0 ** -11 + d * 2.0 ** -24) * rowdot[ha] + 4.9e-4)
    assert (np.abs(m_f - M) <= m_tol).all(), f"m: max err {np.abs(m_f - M).max():.3e}"
    l_ref = L64[ha] * np.exp(M - m_f)
    parity._close("l", l.astype(np.float64)[ha], l_ref, max(rtol, 1e-6), atol)
    res["m"] = float((np.abs(m_f - M) / m_tol).max())
    res["l"] = float((np.abs(l.astype(np.float64)[ha] - l_ref) / gate.plain_bound(l_ref, max(rtol, 1e-6), atol)).max())
    return res


def _edge_lengths(cap, nq, window, chunk):
    """0, 1, the ends of the query block, of the window, of a 64-key tile and of a chunk, and the capacity"""
    want = [0, 1, nq - 1, nq, window - 1, window, window + 1, window + nq, 191, 193, 1279, 1281, chunk - 1, chunk + 1,
            2 * chunk - 1, 2 * chunk + 1, cap]
    return sorted({min(max(x, 0), cap) for x in want})


def _case(form, g, d, vd, nq, window, page, seed, lens=None):
    """Q, the padded caches, the table, what the form reads, and the lengths (default: _edge_lengths)."""
    max_pages = pg._max_pages(page)
    cap = max_pages * page
    plan = _plan(nq, cap, d, vd, g, window, page if form == "paged" else None)
    assert plan[0] >= 1 and plan[6] == 0 and plan[3] >= 3
    lens = _edge_lengths(cap, nq, window, plan[1]) if lens is None else lens
    Q, K, V, table, _, _ = pg._case(len(lens), g, d, vd, nq, page, seed)
    return Q, K, V, table, lens, plan


# ------------------------------------------------------------------ 5. against the reference
WINDOWS = [1, 2, 63, 64, 65, 511, 512, 513, 1000, None]  # None: the capacity - 1


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "cap-1" if w is None else f"w{w}")
@pytest.mark.parametrize("nq", [1, 4, 33])
@pytest.mark.parametrize("form", FORMS)
def test_windows_and_length_edges_against_the_reference(form, nq, window):
    """d = v_d = 64 (16-byte staging), g = 2, pages of 192 keys: every window x every length edge."""
    g, d, page = 2, 64, 192
    cap = pg._max_pages(page) * page
    window = cap - 1 if window is None else window
    Q, K, V, table, lens, plan = _case(form, g, d, d, nq, window, page, seed=7 * window + nq)
    k, v = _stores(form, K, V, table, page)
    got = _ok(form, g, _dev(Q), _dev(k), _dev(v), table, lens, window)
    res = _check_window(got, Q, K, V, np.repeat(lens, HK), g, window)
    print(f"{form} nq={nq} W={window} plan={plan}: worst error / allowance {res}")


@pytest.mark.parametrize("g,nq", [(1, 1), (8, 1), (2, 4), (8, 4), (1, 33), (2, 33)])
@pytest.mark.parametrize("d,vd", [(64, 64), (128, 128), (96, 40), (8, 8)])
@pytest.mark.parametrize("form", FORMS)
def test_instances_against_the_reference(form, d, vd, g, nq):
    """Every D, both stagings (element-wise at (96, 40) and (8, 8), and on pointers misaligned by one element), every
    pitch and wave class of the fold, chunks of 512 and of 1024 keys, at W = 65 and W = 1000."""
    page = 128
    for window in (65, 1000):
        Q, K, V, table, lens, plan = _case(form, g, d, vd, nq, window, page, seed=1000 * d + 10 * g + nq + window)
        assert plan[5] == g * PITCH[nq] and plan[1] == (512 if plan[5] <= 64 else 1024)
        k, v = _stores(form, K, V, table, page)
        tq = _dev(Q)
        got = _ok(form, g, tq, _dev(k), _dev(v), table, lens, window)
        res = _check_window(got, Q, K, V, np.repeat(lens, HK), g, window)
        print(f"{form} d={d} vd={vd} g={g} nq={nq} W={window}: worst error / allowance {res}")
        mis = _ok(form, g, _dev(Q, True), _dev(k, True), _dev(v, True), table, lens, window)
        if d != vd or d not in (32, 64, 128):
            assert rg._same(got, mis)
        else:
            _check_window(mis, Q, K, V, np.repeat(lens, HK), g, window)


@pytest.mark.parametrize("window", [64, 65, 512, 513])
@pytest.mark.parametrize("nq", [1, 4, 33])
@pytest.mark.parametrize("form", FORMS)
def test_beacon_inputs_pin_both_edges(form, nq, window):
    """window_ref.plant_beacons: for the first and the last query the keys just outside and just inside both window
    edges equal the query and carry V of opposite sign, so an edge that is off by one key fails the gate by a factor
    above 100 (tests/test_window_ref.py).  Lengths put the edges inside a tile, on tile edges and on chunk edges."""
    g, d, page = 2, 64, 192
    cap = pg._max_pages(page) * page
    chunk = 512 if g * PITCH[nq] <= 64 else 1024
    lens = sorted({window + nq + 700, window + nq + chunk - 1, window + nq + chunk, window + chunk + 64, 2 * chunk + nq,
                   cap - 1, cap - 64})
    assert all(window + nq <= x < cap for x in lens)
    Q, K, V, table, lens, plan = _case(form, g, d, d, nq, window, page, seed=window + nq, lens=lens)
    assert plan[1] == chunk
    K, V, rows = window_ref.plant_beacons(Q, K, V, np.repeat(lens, HK), window, g)
    assert len(rows) == len(lens) * HK * len(window_ref.beacon_queries(nq))
    k, v = _stores(form, K, V, table, page)
    got = _ok(form, g, _dev(Q), _dev(k), _dev(v), table, lens, window)
    _check_window(got, Q, K, V, np.repeat(lens, HK), g, window)


# ------------------------------------------------------------------ 6. bitwise invariants
@pytest.mark.parametrize("page", [64, 128, 192])
@pytest.mark.parametrize("nq,window", [(1, 1), (4, 65), (4, 600), (33, 513), (1, 2000)])
def test_paged_is_bitwise_ragged_on_the_gathered_cache(page, nq, window):
    g, d = 2, 64
    Q, K, V, table, lens, _ = _case("paged", g, d, d, nq, window, page, seed=page + nq)
    kp, vp = _stores("paged", K, V, table, page)
    tq = _dev(Q)
    for misalign in (False, True):
        got = _ok("paged", g, tq, _dev(kp, misalign), _dev(vp, misalign), table, lens, window)
        assert rg._same(got, _ok("ragged", g, tq, _dev(K, misalign), _dev(V, misalign), None, lens, window))


def _case8(form, g, d, vd, nq, window, page, seed, lens=None):
    Q, K, V, table, lens, _ = _case(form, g, d, vd, nq, window, page, seed, lens)
    rng = np.random.default_rng(seed + 7)
    K8 = fp8_ref.encode(K.astype(np.float64) * np.exp2(-rng.integers(0, 10, K.shape)))
    V8 = fp8_ref.encode(V.astype(np.float64) * np.exp2(rng.integers(-8, 8, V.shape)))
    return Q, K8, V8, table, lens


def _f16(b8):
    return fp8_ref.decode(b8).astype(np.float16)


@pytest.mark.parametrize("d,vd", [(64, 64), (128, 128), (96, 40), (8, 8)])
@pytest.mark.parametrize("g,nq,window", [(8, 1, 64), (2, 4, 513), (1, 33, 1000)])
@pytest.mark.parametrize("form", FORMS)
def test_fp8_with_unit_scales_is_bitwise_the_fp16_call_on_the_converted_cache(form, g, nq, window, d, vd):
    """scales null, and 1.0 read from a device array; aligned (8-byte staging where d == v_d) and offset by one byte"""
    page = 192
    Q, K8, V8, table, lens = _case8(form, g, d, vd, nq, window, page, seed=d + nq)
    k8, v8 = _stores(form, K8, V8, table, page, 0x7F)
    tq, ones = _dev(Q), _scale_dev(np.ones(HK))
    for misalign in (False, True):
        ref = _ok(form, g, tq, _dev(_f16(k8), misalign), _dev(_f16(v8), misalign), table, lens, window)
        tk, tv = _dev(k8, misalign), _dev(v8, misalign)
        for ks, vs in ((None, None), (ones, ones)):
            assert rg._same(_ok(form, g, tq, tk, tv, table, lens, window, fp8=True, ks=ks, vs=vs), ref), (misalign, ks is None)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("nq", [1, 4, 33])
@pytest.mark.parametrize("form", FORMS)
def test_a_window_that_reaches_the_capacity_is_bitwise_the_tail_call(form, nq, fp8):
    """window = capacity, capacity + 1 and INT32_MAX: the un-windowed twin with tail_causal = 1 (its plan, its kernels)"""
    g, d, page = 2, 64, 192
    Q, K8, V8, table, lens = _case8(form, g, d, d, nq, 100, page, seed=nq)
    cap = K8.shape[2]
    K, V = (K8, V8) if fp8 else (_f16(K8), _f16(V8))
    k, v = _stores(form, K, V, table, page, 0x7F if fp8 else np.nan)
    tq, tk, tv = _dev(Q), _dev(k), _dev(v)
    ks, vs = (_scale_dev([0.3, 1.7]), _scale_dev([2.5, 0.04])) if fp8 else (None, None)
    L = _lib.lib()
    prob = rg._problem(nq, cap, d, d, Q.shape[0])
    O_, l, m = (torch.empty_like(t) for t in _ok(form, g, tq, tk, tv, table, lens, 100, fp8=fp8, ks=ks, vs=vs))
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
    tt = torch.tensor(table, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    sc = [ks.data_ptr(), vs.data_ptr()] if fp8 else []
    if form == "ragged":
        need = int(L.fa_forward_ragged_workspace_bytes(prob, g))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        fn = L.fa_forward_ragged_fp8 if fp8 else L.fa_forward_ragged
        st = fn(stream, prob, g, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), *sc, tl.data_ptr(), HK, 1, O_.data_ptr(),
                l.data_ptr(), m.data_ptr(), ws.data_ptr(), need)
    else:
        need = int(L.fa_forward_paged_workspace_bytes(prob, g, page))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        fn = L.fa_forward_paged_fp8 if fp8 else L.fa_forward_paged
        st = fn(stream, prob, g, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), *sc, tt.data_ptr(), table.shape[1], page,
                k.shape[0], tl.data_ptr(), HK, 1, O_.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == 0
    for window in (cap, cap + 1, 2 ** 31 - 1):
        assert _plan(nq, cap, d, d, g, window, page if form == "paged" else None)[6] == 1
        assert rg._same(_ok(form, g, tq, tk, tv, table, lens, window, fp8=fp8, ks=ks, vs=vs), (O_, l, m)), window


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", FORMS)
def test_two_calls_are_equal_a_sequence_does_not_depend_on_the_batch_and_the_wrapper_is_the_abi(form, fp8):
    g, nq, d, vd, page, window = 2, 5, 96, 40, 192, 300
    lens = [2 * page + 9, 2688, 40, 1100]
    Q, K8, V8, table, lens = _case8(form, g, d, vd, nq, window, page, seed=51, lens=lens)
    cap = K8.shape[2]
    K, V = (K8, V8) if fp8 else (_f16(K8), _f16(V8))
    k, v = _stores(form, K, V, table, page, 0x7F if fp8 else np.nan)
    tq, tk, tv = _dev(Q), _dev(k), _dev(v)
    ks, vs = (_scale_dev([0.3, 1.7]), _scale_dev([2.5, 0.04])) if fp8 else (None, None)
    a = _ok(form, g, tq, tk, tv, table, lens, window, fp8=fp8, ks=ks, vs=vs)
    assert rg._same(a, _ok(form, g, tq, tk, tv, table, lens, window, fp8=fp8, ks=ks, vs=vs, ws_fill=0xFF))
    for s in range(4):  # each sequence alone, and beside other lengths
        q1 = slice(s * HK * g, (s + 1) * HK * g)
        one_k, one_v = (tk, tv) if form == "paged" else (tk[s * HK:(s + 1) * HK].contiguous(), tv[s * HK:(s + 1) * HK].contiguous())
        alone = _ok(form, g, tq[q1].contiguous(), one_k, one_v, table[s:s + 1], lens[s:s + 1], window, fp8=fp8, ks=ks, vs=vs)
        assert rg._same([t[q1] for t in a], alone), s
    other = _ok(form, g, tq, tk, tv, table, [lens[0], 7, cap, 0], window, fp8=fp8, ks=ks, vs=vs)
    assert rg._same([t[:HK * g] for t in a], [t[:HK * g] for t in other])
    # the wrapper is the ABI call
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
    tt = torch.tensor(table, dtype=torch.int32, device="cuda:0")
    Qw = tq.reshape(4, HK * g, d, nq)
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    kw = dict(tail_causal=True, returning_l_m=True, window_size=window, **(dict(k_scale=ks, v_scale=vs) if fp8 else {}))
    if form == "ragged":
        got = fa.ragged_1d(Qw, view(tk).reshape(4, HK, d, cap), view(tv).reshape(4, HK, vd, cap), tl, **kw)
    else:
        got = fa.paged_1d(Qw, view(tk), view(tv), tt, tl, **kw)
    torch.cuda.synchronize()
    assert rg._same([t.reshape(r.shape) for t, r in zip(got, a)], a)


# ------------------------------------------------------------------ 7. never read
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("misalign", [False, True], ids=["fast", "elementwise"])
@pytest.mark.parametrize("nq,window", [(4, 300), (1, 64), (33, 513)])
@pytest.mark.parametrize("form", FORMS)
def test_what_lies_outside_the_window_tiles_does_not_reach_the_result(form, nq, window, misalign, fp8):
    """Every key below floor(lo / 64) * 64 and at or past L, and every pool page that no sequence owns, hold NaN, Inf
    or 65504 (FP8: 0x7F, 0xFF, 0x7E); the workspace 0xFF bytes; the table entries of pages wholly below the window's
    first tile and past the last live page INT32_MIN, -1 or INT32_MAX: bitwise the clean call (zeros and valid
    entries there)."""
    g, d, page = 2, 64, 128
    Q, K8, V8, table, lens = _case8(form, g, d, d, nq, window, page, seed=41 + nq)
    cap, max_pages = K8.shape[2], table.shape[1]
    K, V = (K8, V8) if fp8 else (_f16(K8), _f16(V8))
    lo64 = np.array([window_ref.window_lo(x, nq, window, cap) // 64 * 64 for x in lens])
    j = np.arange(cap)[None, :]
    dead = np.repeat((j < lo64[:, None]) | (j >= np.asarray(lens)[:, None]), HK, axis=0)[:, None, :]
    assert dead[:, 0, :].sum() > cap and (lo64 > 0).any()
    pages = np.arange(max_pages)[None, :]
    dead_page = ((pages + 1) * page <= lo64[:, None]) | (pages * page >= np.asarray(lens)[:, None])
    ks, vs = (_scale_dev([0.5, 3.0]), _scale_dev([1.25, 0.01])) if fp8 else (None, None)
    tq = _dev(Q)

    def run(poison, entry):
        zero = np.uint8(poison) if fp8 else np.float16(poison)
        k, v = _stores(form, np.where(dead, zero, K), np.where(dead, zero, V), table, page, poison)
        tbl = table if entry is None else np.where(dead_page, entry, table).astype(np.int32)
        return _ok(form, g, tq, _dev(k, misalign), _dev(v, misalign), tbl, lens, window, fp8=fp8, ks=ks, vs=vs, fill=0x5A,
                   ws_fill=0xFF)

    ref = run(0, None)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    poisons = (0x7F, 0xFF, 0x7E) if fp8 else (np.nan, np.inf, 65504.0)
    for poison, entry in zip(poisons, (pg.INT32_MIN, -1, pg.INT32_MAX)):
        assert rg._same(run(poison, entry), ref), (poison, entry)


# ------------------------------------------------------------------ 8. non-unit FP8 scales
K_SCALES = ([0.037, 2.0 ** -12 * 1.37], [200.0, 0.037])
V_SCALE = [300.0, 0.0123]


@pytest.mark.parametrize("k_scale", K_SCALES, ids=["small", "large"])
@pytest.mark.parametrize("g,nq,window", [(4, 4, 300), (1, 1, 1000)])
@pytest.mark.parametrize("d", [64, 128, 40])
@pytest.mark.parametrize("form", FORMS)
def test_real_fp8_scales_against_the_reference_on_the_dequantized_cache(form, d, g, nq, window, k_scale):
    """The FP8 tests' scales (0.037: e = -5; 2^-12 * 1.37: clamped to e = -8; 200: clamped to e = 7) under the same gate"""
    page = 192
    Q, K, V, table, lens, _ = _case(form, g, d, d, nq, window, page, seed=300 + d + g)
    cap = K.shape[2]
    byhead = lambda x: x.reshape(len(lens), HK, d, cap)  # noqa: E731
    K8 = fp8_ref.quantize(byhead(K), k_scale, 1).reshape(K.shape)
    V8 = fp8_ref.quantize(byhead(V), V_SCALE, 1).reshape(V.shape)
    Kd = fp8_ref.dequantize(byhead(K8), k_scale, 1).reshape(K.shape)
    Vd = fp8_ref.dequantize(byhead(V8), V_SCALE, 1).reshape(V.shape)
    k8, v8 = _stores(form, K8, V8, table, page, 0x7F)
    got = _ok(form, g, _dev(Q), _dev(k8), _dev(v8), table, lens, window, fp8=True, ks=_scale_dev(k_scale), vs=_scale_dev(V_SCALE))
    res = _check_window(got, Q, Kd, Vd, np.repeat(lens, HK), g, window)
    print(f"{form} d={d} g={g} nq={nq} W={window}: worst error / allowance {res}")


# ------------------------------------------------------------------ 9. graph replay
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_a_captured_windowed_call_follows_lengths_table_pools_and_scales_on_the_device(fp8):
    """One windowed paged_1d call captured in a graph.  Between replays k_lens, block_table, the pools and the scales
    are overwritten in place; the lengths move lo from chunk 0 to chunk 1, onto the chunk edge (lo = 512), one key
    below it and to chunk 4: every replay is bitwise the eager call on the same state."""
    g, nq, d, page, window = 4, 4, 64, 192, 300
    Q, K8, V8, table, _ = _case8("paged", g, d, d, nq, window, page, seed=81, lens=[0, 0, 0])
    num_pages, cap = table.size + SPARE, K8.shape[2]
    assert _plan(nq, cap, d, d, g, window, page)[:2] == (2, 512)
    conv = (lambda x: x) if fp8 else _f16
    fill = 0x7F if fp8 else np.nan

    def pools(tbl):
        k, v = conv(K8), conv(V8)
        scatter = (lambda x: _stores("paged", x, x, tbl, page, fill)[0])
        return scatter(k), scatter(v)

    kp, vp = pools(table)
    tq = _dev(Q).reshape(3, HK * g, d, nq)
    tk, tv = _dev(kp), _dev(vp)
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    tt = torch.tensor(table, dtype=torch.int32, device="cuda:0")
    lens = torch.tensor([cap, 1, 700], dtype=torch.int32, device="cuda:0")
    ks, vs = (_scale_dev([1.0, 1.0]), _scale_dev([1.0, 1.0])) if fp8 else (None, None)
    kw = dict(tail_causal=True, returning_l_m=True, window_size=window, **(dict(k_scale=ks, v_scale=vs) if fp8 else {}))
    fa.paged_1d(tq, view(tk), view(tv), tt, lens, **kw)  # (first launches raise the LDS limit)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fa.paged_1d(tq, view(tk), view(tv), tt, lens, **kw)
    # lo = L - nq - W + 1 = L - 303
    for i, (now, k_now, v_now) in enumerate((([5, cap, 0], [0.037, 3.0], [300.0, 0.5]),
                                             ([815, 814, 816], [1.0, 1.0], [1.0, 1.0]),
                                             ([303, 2351, 1327], [2.0 ** -12 * 1.37, 200.0], [0.0123, 7.0]))):
        lens.copy_(torch.tensor(now, dtype=torch.int32))
        if fp8:
            ks.copy_(torch.tensor(k_now))
            vs.copy_(torch.tensor(v_now))
        new = np.random.default_rng(90 + i).permutation(num_pages)[:table.size].reshape(table.shape).astype(np.int32)
        tt.copy_(torch.from_numpy(new))
        kp, vp = pools(new)
        tk.copy_(torch.from_numpy(kp))
        tv.copy_(torch.from_numpy(vp))
        graph.replay()
        torch.cuda.synchronize()
        kw2 = dict(kw, **(dict(k_scale=ks.clone(), v_scale=vs.clone()) if fp8 else {}))
        eager = fa.paged_1d(tq, view(tk.clone()), view(tv.clone()), tt.clone(), lens.clone(), **kw2)
        torch.cuda.synchronize()
        assert rg._same(out, eager), now
        st, *abi = _win("paged", g, tq.reshape(-1, d, nq), tk, tv, tt, lens, window, fp8=fp8, ks=ks, vs=vs)
        assert st == 0 and rg._same([t.reshape(r.shape) for t, r in zip(out, abi)], abi)
    del graph


# ------------------------------------------------------------------ 10. refusals
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", FORMS)
def test_a_short_workspace_and_an_out_of_envelope_problem_write_nothing(form, fp8):
    g, nq, d, page, window = 4, 8, 64, 64, 300
    Q, K8, V8, table, _ = _case8(form, g, d, d, nq, window, page, seed=71, lens=[2600, 100])
    K, V = (K8, V8) if fp8 else (_f16(K8), _f16(V8))
    k, v = _stores(form, K, V, table, page, 0x7F if fp8 else np.nan)
    tq, tk, tv = _dev(Q), _dev(k), _dev(v)
    st, *out = _win(form, g, tq, tk, tv, table, [2600, 100], window, fp8=fp8, ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL and "workspace_bytes" in _lib.last_error()
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())
    st, *out = _win(form, g, tq, tk, tv, table, [2600, 100], 0, fp8=fp8, fill=0x5A)
    assert st == _lib.FA_ERR_INVALID_ARGUMENT and "window" in _lib.last_error()
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())
    if form == "paged":  # a page of 32 keys: outside the envelope, windowed and delegated alike
        table32 = np.stack([2 * table, 2 * table + 1], axis=-1).reshape(2, -1).astype(np.int32)
        for w in (window, 10 ** 6):
            st, *out = _win(form, g, tq, tk, tv, table32, [2600, 100], w, fp8=fp8, fill=0x5A, page=32)
            assert st == _lib.FA_ERR_UNSUPPORTED and "page % 64" in _lib.last_error()
            for t in out:
                assert bool((t.view(torch.uint8) == 0x5A).all())
    else:  # 33 queries x 4 heads: above 128 folded rows
        Q33 = rg._np_inputs(2 * HK, g, d, d, 33, 8, seed=1)[0]
        for w in (window, 10 ** 6):
            st, *out = _win(form, g, _dev(Q33), tk, tv, table, [2600, 100], w, fp8=fp8, fill=0x5A)
            assert st == _lib.FA_ERR_UNSUPPORTED and "envelope" in _lib.last_error()
            for t in out:
                assert bool((t.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_batch_is_ok(form):
    L = _lib.lib()
    prob = rg._problem(4, 2560, 64, 64, 0)
    ws = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    if form == "ragged":
        st = L.fa_forward_ragged_window(None, prob, 4, None, None, None, None, HK, 300, None, None, None, ws.data_ptr(), 0)
    else:
        st = L.fa_forward_paged_window(None, prob, 4, None, None, None, None, 40, 64, 8, None, HK, 300, None, None, None,
                                       ws.data_ptr(), 0)
    assert st == _lib.FA_OK
