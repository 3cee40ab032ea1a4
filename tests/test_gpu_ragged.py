"""GPU tests of the ragged few-query forward (csrc/fa_fwd_f16_decode.hip over RaggedCache, fa_forward_ragged,
flash_attention.ragged_1d): K and V are laid out for a capacity, K/V slice bkv attends its first
k_lens[bkv / kv_per_len] keys, and the lengths are device data.

The full form of a slice of length L is the full rule on K / V truncated to L, so it goes through
tests.test_gpu_parity.run_case (its fp16 forward tolerances TOL[float16]["fwd"] for O and l, its fp16 rule for m,
rows without a key exactly O = 0, l = 0, m = bytes 0xFA): one run_case call per distinct length, handed the
truncated K / V as inputs= and the slices of that length, and reaching the ONE ragged call of the test through its
module-level _call hook.  The tail-causal form is no existing rule; it is compared with tests/ragged_ref.py (checked
against the oracle by tests/test_ragged_ref.py) under the same tolerances, restated in _check_ref.  The poison,
clamp, batch-independence, grouped-equality, wrapper and graph tests are bitwise."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gate
from tests import ragged_ref
from tests import test_gpu_parity as parity
from tests.gate import TOL
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu


def _problem(nq, cap, d, vd, b, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, vd)


def _plan(nq, cap, d, vd, g):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_ragged_plan(_problem(nq, cap, d, vd, g), g, out) == 0
    return tuple(out)


def _np_inputs(bkv, g, d, vd, nq, cap, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(bkv * g, d, nq), mk(bkv, d, cap), mk(bkv, vd, cap)


def _dev(x, misalign=False):
    return parity._to_dev(x, torch.device("cuda:0"), False, misalign)


def _abi(g, Q, K, V, lens, kv_per_len=1, tail=False, ws_short=0, fill=None, ws_fill=None, prob=None):
    """fa_forward_ragged on device tensors (lens: a device int32 tensor or a list); returns (status, O, l, m)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    vd, cap = V.shape[1], V.shape[2]
    prob = _problem(nq, cap, d, vd, b) if prob is None else prob
    if not isinstance(lens, torch.Tensor):
        lens = torch.tensor(list(lens), dtype=torch.int32, device=Q.device)
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O_, l, m):
            t.view(torch.uint8).fill_(fill)
    need = int(L.fa_forward_ragged_workspace_bytes(prob, g))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    st = L.fa_forward_ragged(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                             lens.data_ptr(), kv_per_len, int(tail), O_.data_ptr(), l.data_ptr(), m.data_ptr(),
                             ws.data_ptr(), max(need - ws_short, 0))
    torch.cuda.synchronize()
    return st, O_, l, m


def _same(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def _check_empty(got, rows):
    """rows: bool [b, nq] of the rows that see no key: exactly O = 0, l = 0, m = bytes 0xFA."""
    o, l, m = (t.cpu().numpy() for t in got)
    if rows.any():
        assert (np.moveaxis(o, 1, 2)[rows] == 0).all()
        assert (l[rows] == 0).all()
        assert m[rows].tobytes() == b"\xfa" * (2 * int(rows.sum()))


def _check_full_by_run_case(monkeypatch, got, Q, K, V, kv_lens, g):
    """The full form against the oracle on truncated K / V: run_case per distinct length over the slices that have
    it, with the ragged result of those slices handed in through run_case's _call hook."""
    cap, nq, d, vd = K.shape[2], Q.shape[2], Q.shape[1], V.shape[1]
    lens_q = np.clip(np.repeat(np.asarray(kv_lens), g), 0, cap)
    _check_empty(got, np.broadcast_to((lens_q == 0)[:, None], (Q.shape[0], nq)))
    for L in sorted(set(lens_q.tolist()) - {0}):
        sub = np.nonzero(lens_q == L)[0]
        part = tuple(t[torch.from_numpy(sub).to(t.device)] for t in got)
        monkeypatch.setattr(parity, "_call", lambda *a, part=part: part)
        res = parity.run_case(np.float16, "full", 1, "none_front", (len(sub),), d, vd, (nq,), (L,), bwd=False,
                              inputs=(Q[sub], K[:, :, :L][sub // g], V[:, :, :L][sub // g],
                                      np.zeros((len(sub), vd, nq), np.float16)), slices=range(len(sub)))
        print(f"L = {L}: {len(sub)} slices, O max err / scale {res['O']:.3e}")


def _check_ref(got, Q, K, V, kv_lens, g, tail, m_bound=None):
    """Against tests/ragged_ref.py under run_case's fp16 forward rule: O and l within TOL[float16]['fwd'] (l
    relative to the stored m), m within 2 ulp plus the larger of 1e-3 * max(|m|, 1) and the rounding a score can
    carry from the fp16 pre-scaled Q, (2^-11 + d 2^-24) * max_j sum_c |q_c k_jc| / sqrt(d) + 4.9e-4.  m_bound
    (optional, [b, nq]) replaces that dot-product term only, as run_case(m_bound=...) does (gate.m_tol_bounded).
    Returns the worst |error| / allowance of O, l and m (for the records of a sweep; every check is an assertion)."""
    O64, L64, M64, ha = ragged_ref.forward_f64(Q, K, V, kv_lens, g, tail)
    o, l, m = (t.cpu().numpy() for t in got)
    b, d, nq = Q.shape
    cap = K.shape[2]
    rtol, atol = TOL[np.float16]["fwd"]
    _check_empty(got, ~ha)
    live = ha[:, None, :] & np.ones_like(O64, bool)
    parity._close("O", np.where(live, o, 0.0), O64, rtol, atol)
    assert np.isfinite(o.astype(np.float64)).all()
    res = {"O": float((np.abs(np.where(live, o, 0.0) - O64) / gate.plain_bound(O64, rtol, atol)).max())}
    if not ha.any():
        return res
    m_f, M = m.astype(np.float64)[ha], M64[ha]
    if m_bound is None:
        rowdot = np.zeros((b, nq))
        for bi in range(b):
            mask = ragged_ref.ragged_mask(nq, cap, kv_lens[bi // g], tail)
            rowdot[bi] = gate.max_abs_dot(Q[bi][None], K[bi // g][None], mask)[0] / math.sqrt(d)
        ulp = np.abs(np.spacing(np.abs(M).astype(np.float16))).astype(np.float64)
        m_tol = 2 * ulp + np.maximum(1e-3 * np.maximum(np.abs(M), 1.0), (2.0 ** -11 + d * 2.0 ** -24) * rowdot[ha] + 4.9e-4)
    else:
        m_tol = gate.m_tol_bounded(M, np.float16, np.asarray(m_bound, dtype=np.float64)[ha])
    assert (np.abs(m_f - M) <= m_tol).all(), f"m: max err {np.abs(m_f - M).max():.3e}"
    l_ref = L64[ha] * np.exp(M - m_f)
    parity._close("l", l.astype(np.float64)[ha], l_ref, max(rtol, 1e-6), atol)
    res["m"] = float((np.abs(m_f - M) / m_tol).max())
    res["l"] = float((np.abs(l.astype(np.float64)[ha] - l_ref) / gate.plain_bound(l_ref, max(rtol, 1e-6), atol)).max())
    return res


# ------------------------------------------------------------------ tile, chunk and 16-byte edges
def _edge_lengths(cap):
    return [0, 1, 63, 64, 65, 72, 77, 511, 512, 513, 2599, cap]


@pytest.mark.parametrize("cap", [2600, 2601], ids=["fast", "elementwise"])
def test_tile_chunk_and_chunk8_edges(monkeypatch, cap):
    """d = v_d = 64, g = 4, nq = 4, Hk = 2 heads per sequence sharing its length (kv_per_len = 2): lengths at the
    ends of a 64-key tile, a 512-key chunk and a 16-byte run of 8 keys, through ragged_1d."""
    g, nq, hk, d = 4, 4, 2, 64
    chunks, chunk = _plan(nq, cap, d, d, g)[:2]
    assert chunk == 512 and chunks >= 3
    lens = _edge_lengths(cap)
    Q, K, V = _np_inputs(len(lens) * hk, g, d, d, nq, cap, seed=cap)
    shape = lambda x, h: _dev(x.reshape((len(lens), h) + x.shape[1:]))  # noqa: E731
    got = fa.ragged_1d(shape(Q, hk * g), shape(K, hk), shape(V, hk), torch.tensor(lens, dtype=torch.int32, device="cuda:0"),
                       returning_l_m=True)
    torch.cuda.synchronize()
    assert got[0].shape == (len(lens), hk * g, d, nq) and got[1].shape == got[2].shape == (len(lens), hk * g, nq)
    got = tuple(t.reshape((-1,) + t.shape[2:]) for t in got)
    _check_full_by_run_case(monkeypatch, got, Q, K, V, np.repeat(lens, hk), g)


# ------------------------------------------------------------------ instances
@pytest.mark.parametrize("g,nq", [(1, 1), (1, 33), (8, 1), (128, 1), (3, 3), (2, 33), (2, 64)])
@pytest.mark.parametrize("d,vd", [(8, 8), (96, 40), (128, 128)])
def test_instances(monkeypatch, d, vd, g, nq):
    """D = 32 / 128 (element-wise staging) and D = 128 with 16-byte staging, every pitch and wave class of the fold,
    one group and ungrouped decode; then the same call on pointers misaligned by one element (bitwise equal where
    the staging is element-wise on both sides, and checked against the oracle either way)."""
    cap = 1096
    lens = [77, 0, cap, 600]
    Q, K, V = _np_inputs(len(lens), g, d, vd, nq, cap, seed=1000 * d + 10 * g + nq)
    st, *got = _abi(g, _dev(Q), _dev(K), _dev(V), lens)
    assert st == 0
    _check_full_by_run_case(monkeypatch, got, Q, K, V, lens, g)
    st, *mis = _abi(g, _dev(Q, True), _dev(K, True), _dev(V, True), lens)
    assert st == 0
    if d != vd or d not in (32, 64, 128):
        assert _same(got, mis)
    else:
        _check_full_by_run_case(monkeypatch, mis, Q, K, V, lens, g)


# ------------------------------------------------------------------ tail-causal
@pytest.mark.parametrize("cap", [1096, 1101], ids=["fast", "elementwise"])
@pytest.mark.parametrize("nq", [1, 4, 16, 33])
def test_tail_causal(nq, cap):
    """Query i sees keys j <= L - nq + i.  L = 66 and 514 put the window of the last nq keys across the tile edge at
    64 and the chunk edge at 512; L = nq - 1 leaves query 0 without a key, L = 0 all of them."""
    g, d = (1 if nq == 33 else 2), 64
    chunks, chunk = _plan(nq, cap, d, d, g)[:2]
    assert chunk == 512 and chunks == 3
    lens = [0, nq - 1, nq, 66, 514, cap]
    Q, K, V = _np_inputs(len(lens), g, d, d, nq, cap, seed=nq + cap)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    st, *got = _abi(g, tq, tk, tv, lens, tail=True)
    assert st == 0
    _check_ref(got, Q, K, V, lens, g, True)
    if nq == 1:
        st, *full = _abi(g, tq, tk, tv, lens, tail=False)
        assert st == 0 and _same(got, full)


# ------------------------------------------------------------------ poison past the lengths
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("cap", [2600, 2601], ids=["fast", "elementwise"])
def test_values_past_the_length_do_not_reach_the_result(cap, tail):
    """K and V past every length filled with NaN, Inf and 65504, and the workspace with 0xFF bytes (NaN): (O, l, m)
    are bitwise those of the same call with zeros there."""
    g, nq, d = 4, 4, 64
    lens = _edge_lengths(cap)
    Q, K, V = _np_inputs(len(lens), g, d, d, nq, cap, seed=5)
    past = np.arange(cap)[None, None, :] >= np.asarray(lens)[:, None, None]
    tq = _dev(Q)
    st, *ref = _abi(g, tq, _dev(np.where(past, np.float16(0), K)), _dev(np.where(past, np.float16(0), V)), lens, tail=tail)
    assert st == 0
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    for poison in (np.nan, np.inf, 65504.0):
        st, *got = _abi(g, tq, _dev(np.where(past, np.float16(poison), K)), _dev(np.where(past, np.float16(poison), V)),
                        lens, tail=tail, ws_fill=0xFF)
        assert st == 0
        assert _same(got, ref), f"poison {poison}"


# ------------------------------------------------------------------ clamp
def test_lengths_are_clamped_to_the_capacity():
    """An over-capacity length acts as the capacity and a negative one as 0, on slices that are not the last of
    K / V: without the clamp the first would read its neighbour's keys and fail the comparison."""
    g, nq, d, cap = 4, 4, 64, 1096
    Q, K, V = _np_inputs(4, g, d, d, nq, cap, seed=6)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    for tail in (False, True):
        st0, *got = _abi(g, tq, tk, tv, [cap + 1, -1, 2 ** 31 - 1, 300], tail=tail)
        st1, *ref = _abi(g, tq, tk, tv, [cap, 0, cap, 300], tail=tail)
        assert st0 == 0 and st1 == 0
        assert _same(got, ref)
        _check_ref(got, Q, K, V, [cap, 0, cap, 300], g, tail)
        _check_empty(got, np.repeat(np.array([False, True, False, False]), g)[:, None] & np.ones((1, nq), bool))


# ------------------------------------------------------------------ bitwise properties
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_two_calls_are_equal_and_a_sequence_does_not_depend_on_the_batch(tail):
    g, nq, d, vd, cap, hk = 2, 5, 96, 40, 1101, 2
    Q, K, V = _np_inputs(3 * hk, g, d, vd, nq, cap, seed=7)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    st0, *a = _abi(g, tq, tk, tv, [1101, 333, 40], kv_per_len=hk, tail=tail)
    st1, *b = _abi(g, tq, tk, tv, [1101, 333, 40], kv_per_len=hk, tail=tail)
    assert st0 == 0 and st1 == 0 and _same(a, b)
    q1, k1 = slice(hk * g, 2 * hk * g), slice(hk, 2 * hk)
    st2, *alone = _abi(g, tq[q1].contiguous(), tk[k1].contiguous(), tv[k1].contiguous(), [333], kv_per_len=hk, tail=tail)
    st3, *others = _abi(g, tq, tk, tv, [0, 333, 1000], kv_per_len=hk, tail=tail)
    assert st2 == 0 and st3 == 0
    assert _same([t[q1] for t in a], alone)
    assert _same([t[q1] for t in others], alone)


@pytest.mark.parametrize("g,nq,d,cap", [(4, 8, 64, 2600), (4, 8, 64, 2601), (2, 33, 128, 1096), (8, 1, 32, 640)])
def test_full_lengths_are_bitwise_the_grouped_forward(g, nq, d, cap):
    """Every length equal to the capacity, g >= 2: the plan and the key loop are fa_forward_grouped's under FA_FULL."""
    L = _lib.lib()
    Q, K, V = (_dev(x) for x in _np_inputs(2, g, d, d, nq, cap, seed=8))
    prob = _problem(nq, cap, d, d, 2 * g)
    st, *got = _abi(g, Q, K, V, [cap, cap])
    assert st == 0
    ref = [torch.empty_like(t) for t in got]
    need = int(L.fa_forward_grouped_workspace_bytes(prob, g))
    assert need == int(L.fa_forward_ragged_workspace_bytes(prob, g))
    ws = torch.empty(need, dtype=torch.uint8, device=Q.device)
    st = L.fa_forward_grouped(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                              ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == 0
    assert _same(got, ref)


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
def test_python_wrapper_is_the_abi_call(tail):
    """Leading batch axes [2, 3] with Hk = 2: kv_per_len = 2 and one length per sequence; and tensors without a
    batch axis with a 0-d k_lens."""
    g, nq, d, cap, hk = 4, 4, 64, 1096, 2
    lens = [[1096, 5, 513], [0, 700, 64]]
    Q, K, V = (_dev(x) for x in _np_inputs(6 * hk, g, d, d, nq, cap, seed=9))
    tl = torch.tensor(lens, dtype=torch.int32, device=Q.device)
    st, *direct = _abi(g, Q, K, V, tl.reshape(-1), kv_per_len=hk, tail=tail)
    assert st == 0
    got = fa.ragged_1d(Q.reshape(2, 3, hk * g, d, nq), K.reshape(2, 3, hk, d, cap), V.reshape(2, 3, hk, d, cap), tl,
                       tail_causal=tail, returning_l_m=True)
    torch.cuda.synchronize()
    assert got[0].shape == (2, 3, hk * g, d, nq)
    assert _same([t.reshape(r.shape) for t, r in zip(got, direct)], direct)
    one = fa.ragged_1d(Q[hk * g:2 * hk * g], K[hk:2 * hk], V[hk:2 * hk], tl[0, 1], tail_causal=tail, returning_l_m=True)
    torch.cuda.synchronize()
    assert _same(one, [t[hk * g:2 * hk * g] for t in direct])
    assert torch.equal(fa.ragged_1d(Q[hk * g:2 * hk * g], K[hk:2 * hk], V[hk:2 * hk], tl[0, 1], tail_causal=tail), one[0])


# ------------------------------------------------------------------ ABI statuses
def test_short_workspace_is_rejected_and_nothing_is_written():
    Q, K, V = (_dev(x) for x in _np_inputs(2, 4, 64, 64, 8, 2600, seed=2))
    st, *out = _abi(4, Q, K, V, [2600, 100], ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


def test_outside_the_envelope_the_abi_reports_unsupported_and_writes_nothing():
    Q, K, V = (_dev(x) for x in _np_inputs(2, 2, 64, 64, 200, 300, seed=6))
    st, *out = _abi(2, Q, K, V, [300, 100], fill=0x5A)
    assert st == _lib.FA_ERR_UNSUPPORTED
    for t in out:
        assert bool((t.view(torch.uint8) == 0x5A).all())


# ------------------------------------------------------------------ graph replay
def test_a_captured_call_follows_the_lengths_on_the_device():
    """One ragged_1d call captured in a (linear, one-stream) graph and replayed with k_lens overwritten in place:
    every replay is bitwise the eager call at those lengths."""
    g, nq, d, cap, hk = 4, 4, 64, 2600, 2
    Q, K, V = (_dev(x.reshape((3, -1) + x.shape[1:])) for x in _np_inputs(3 * hk, g, d, d, nq, cap, seed=11))
    lens = torch.tensor([2600, 1, 700], dtype=torch.int32, device=Q.device)
    for tail in (False, True):
        fa.ragged_1d(Q, K, V, lens, tail_causal=tail)  # (first launches raise the kernels' LDS limit: not capturable)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fa.ragged_1d(Q, K, V, lens, tail_causal=tail, returning_l_m=True)
        for now in ([5, 2600, 0], [513, 64, 2599], [77, 77, 1024]):
            lens.copy_(torch.tensor(now, dtype=torch.int32))
            graph.replay()
            torch.cuda.synchronize()
            eager = fa.ragged_1d(Q, K, V, torch.tensor(now, dtype=torch.int32, device=Q.device), tail_causal=tail,
                                 returning_l_m=True)
            torch.cuda.synchronize()
            assert _same(out, eager), now
        del graph
