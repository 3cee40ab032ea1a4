"""GPU tests of the sliding-window prefill forwards (csrc/fa_fwd_f16_window_prefill.h / .hip,
fa_forward_ragged_window_prefill / fa_forward_paged_window_prefill and their _fp8 forms,
flash_attention.ragged_window_prefill_1d / paged_window_prefill_1d): the nq queries are the last nq
positions of a sequence of L keys, query i at pos = L - nq + i sees the W keys [max(0, pos - W + 1), pos], for any nq,
worked in blocks of P_b queries with one workgroup per (K/V slice, query block, launched chunk).

Parity is against tests/window_ref.py under the rule that tests/test_gpu_window.py applies (_check_window: O and l
within TOL[float16]['fwd'], test_gpu_ragged._check_ref's allowance on m, empty rows exact; an FP8 cache on the
dequantized cache), at test_gpu_prefill's smallest shapes, a capacity of 2560 keys, every window of test_gpu_window, and
lengths that put a block's key end L_b at 0, at 1 and either side of a tile and a chunk edge and a block's window
start lo_b either side of a tile and a chunk edge.  The trap shapes also run tests/window_prefill_beacons.py's
inputs, on which either window edge moved by one key is a gross error (tests/test_window_prefill_beacons.py).
Everything else is bitwise: paged = ragged on the gathered cache, FP8 with unit scales = fp16 on the converted cache,
W >= capacity = the query-blocked tail call, one block = the windowed twin, a full block = the windowed twin on a copy
of its queries, the wrapper = the ABI call, poison, and a captured graph."""

import ctypes

import numpy as np
import pytest
import torch

from tests import prefill_beacons as B
from tests import score_ramp as R
from tests import test_gpu_prefill as P
from tests import test_gpu_ragged as rg
from tests import test_gpu_window as tw
from tests import window_prefill_beacons as WB
from tests import window_ref
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = P.INT32_MIN, P.INT32_MAX
FORMS = P.FORMS
SHAPES = [(1, 129), (1, 256), (8, 17), (8, 37), (16, 20), (128, 2), (4, 33)]
CHANNELS = [(64, 64), (128, 128), (40, 72), (8, 8)]
CAP = 2560
WINDOWS = [1, 2, 63, 64, 65, 511, 512, 513, 1000, CAP - 1]
_dev, _same, _scatter, _table, _quantize, _inputs = P._dev, P._same, P._scatter, P._table, P._quantize, P._inputs


# ------------------------------------------------------------------ calls
def _plan(nq, cap, d, vd, g, window, page=None, kind="_window_prefill"):
    out = (ctypes.c_int32 * 8)()
    L = _lib.lib()
    p = P._problem(nq, cap, d, vd, g)
    own = (p, g) + (() if page is None else (page,)) + ((window,) if "window" in kind else ())
    assert getattr(L, "fa_forward_" + ("ragged" if page is None else "paged") + kind + "_plan")(*own, out) == 0
    return tuple(out)


def _abi(form, g, Q, K, V, lens, window, hk=1, table=None, scales=(None, None), fill=None, ws_fill=None, ws_short=0,
         kind="_window_prefill", page=None):
    """One of the four forwards of the form (kind "_window": the windowed twin's entry point; "_prefill": the
    query-blocked one's with tail_causal = 1) on device tensors.  K / V: the padded cache [bkv, c, cap] or, for a paged
    form, the pools [num_pages, hk, c, page] with ``table`` [sequences, max_pages].  Returns (status, O, l, m,
    workspace, workspace bytes)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    paged, fp8 = form.startswith("paged"), form.endswith("fp8")
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    lens = as_dev(lens)
    if paged:
        table = as_dev(table)
        num_pages, vd = V.shape[0], V.shape[2]
        page = V.shape[3] if page is None else page
        max_pages = table.shape[-1]
        cap = max_pages * page
    else:
        vd, cap = V.shape[1], V.shape[2]
    prob = P._problem(nq, cap, d, vd, b)
    out = (torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device),
           torch.empty((b, nq), dtype=torch.float32, device=Q.device),
           torch.empty((b, nq), dtype=torch.float16, device=Q.device))
    if fill is not None:
        for t in out:
            t.view(torch.uint8).fill_(fill)
    stem = "fa_forward_" + ("paged" if paged else "ragged") + kind
    own = (prob, g) + ((page,) if paged else ()) + ((window,) if "window" in kind else ())
    need = int(getattr(L, stem + "_workspace_bytes")(*own))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    sc = [None if s is None else s.data_ptr() for s in scales] if fp8 else []
    where = [table.data_ptr(), max_pages, page, num_pages] if paged else []
    st = getattr(L, stem + ("_fp8" if fp8 else ""))(
        torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), *sc, *where,
        lens.data_ptr(), hk, window if "window" in kind else 1, *(t.data_ptr() for t in out), ws.data_ptr(),
        max(need - ws_short, 0))
    torch.cuda.synchronize()
    return (st,) + out + (ws, need)


def _run(form, g, Q, K, V, lens, window, **kw):
    st, *got = _abi(form, g, Q, K, V, lens, window, **kw)
    assert st == 0, _lib.last_error()
    return got[:3]


def _stores(form, K, V, table, page, hk=1):
    """what the form reads: the padded caches, or the pools scattered through the table"""
    if not form.startswith("paged"):
        return _dev(K), _dev(V)
    fill = 0x7F if K.dtype == np.uint8 else np.nan
    return _dev(_scatter(K, table, page, hk, fill)), _dev(_scatter(V, table, page, hk, fill))


def _blocks(g, nq, lens, cap, window):
    """(L_b, lo_b) [sequences, nqb] from include/fa_api.h's text"""
    pb, nqb = B.block_shape(g, nq)
    L = np.clip(np.asarray(lens), 0, cap)
    ends, los = [], []
    for qb in range(nqb):
        nq_b = min(pb, nq - qb * pb)
        lb = np.clip(L - nq + qb * pb + nq_b, 0, L)
        ends.append(lb)
        los.append(np.maximum(lb - nq_b - window + 1, 0))
    return np.stack(ends, axis=1), np.stack(los, axis=1)


def _lengths(g, nq, cap, chunk, window):
    """0; 1; nq - 1; nq; nq + 1; what puts block 0's and the last block's key end L_b at 0, at 1 and on either side of
    a tile edge and of a chunk edge; what puts their window start lo_b on either side of a tile edge and of a chunk
    edge; the capacity; the capacity + 5 (clamped)."""
    pb, nqb = B.block_shape(g, nq)
    cand = {0, 1, nq - 1, nq, nq + 1, cap, cap + 5}
    for behind, nq_b in ((nq - min(pb, nq), min(pb, nq)), (0, nq - (nqb - 1) * pb)):  # L_b = L - behind
        for edge in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1):
            cand.add(edge + behind)
        for edge in (63, 64, 65, chunk - 1, chunk, chunk + 1):  # lo_b = L_b - nq_b - W + 1
            cand.add(edge + nq_b + window - 1 + behind)
    return sorted(x for x in cand if 0 <= x <= cap + 5)


# ------------------------------------------------------------------ parity: every window x the shapes x the four forms
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("g,nq", SHAPES)
def test_parity(g, nq, window):
    """The fp16 and the FP8 cache (non-unit scales) against the reference, and the paged forms bitwise against the
    ragged ones through a random table.  Channels and pages rotate over the cases."""
    i = SHAPES.index((g, nq)) + WINDOWS.index(window)
    d, vd = CHANNELS[i % 4]
    page = (64, 128)[i % 2]
    plan = _plan(nq, CAP, d, vd, g, window)
    launched, chunk, span_w, cap_chunks, pb, rows, nqb, delegated = plan
    assert delegated == 0 and (pb, nqb) == B.block_shape(g, nq) and rows == g * pb and nqb >= 2
    assert plan == _plan(nq, CAP, d, vd, g, window, page)
    lens = _lengths(g, nq, CAP, chunk, window)
    ends, los = _blocks(g, nq, lens, CAP, window)
    assert {0, 1, 63, 64, 65} <= set(ends.ravel().tolist())
    assert {chunk - 1, chunk, chunk + 1} <= set(ends.ravel().tolist())
    if window + pb + 65 <= CAP:
        assert {63, 64, 65} <= set(los.ravel().tolist())
    if window + pb + chunk + 1 <= CAP:
        assert {chunk - 1, chunk, chunk + 1} <= set(los.ravel().tolist())
    Q, K, V = _inputs(g, nq, d, vd, CAP, len(lens), seed=CAP + nq + window)
    K8, V8, scales, Kd, Vd = _quantize(K, V, 1)
    table = _table(len(lens), CAP // page, seed=window)
    tq = _dev(Q)
    got = _run("ragged", g, tq, _dev(K), _dev(V), lens, window)
    res = tw._check_window(got, Q, K, V, lens, g, window)
    got8 = _run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, window, scales=scales)
    res8 = tw._check_window(got8, Q, Kd, Vd, lens, g, window)
    print(f"g={g} nq={nq} W={window} d={d} vd={vd} plan={plan}: f16 {res}  fp8 {res8}")
    assert _same(_run("paged", g, tq, *_stores("paged", K, V, table, page), lens, window, table=table), got)
    assert _same(_run("paged_fp8", g, tq, *_stores("paged", K8, V8, table, page), lens, window, table=table, scales=scales), got8)


@pytest.mark.parametrize("g,nq,window", [(8, 37, 65), (1, 129, 1000), (3, 40, 513)])
def test_parity_at_a_capacity_that_is_no_multiple_of_eight(g, nq, window):
    """cap = 2601: element-wise staging at d = v_d = 64, and a last chunk of 41 keys"""
    cap, d = 2601, 64
    chunk = _plan(nq, cap, d, d, g, window)[1]
    lens = _lengths(g, nq, cap, chunk, window)
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=nq + window)
    tw._check_window(_run("ragged", g, _dev(Q), _dev(K), _dev(V), lens, window), Q, K, V, lens, g, window)


# ------------------------------------------------------------------ beacons
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("window", [2, 64, 513])
@pytest.mark.parametrize("g,nq,d,vd", [(8, 37, 32, 40), (16, 20, 64, 64), (1, 129, 64, 64), (1, 256, 128, 128)])
def test_beacons(g, nq, d, vd, window, form):
    """Four towering keys around both window edges of queries 0, nq - 1 and the queries on both sides of the block
    edges, with V of opposite sign inside and outside: an edge that is one key off fails the gate
    (tests/test_window_prefill_beacons.py).  The lengths put the edges inside a tile, on tile and chunk edges."""
    page = 64
    chunk = _plan(nq, CAP, d, vd, g, window)[1]
    pb = B.block_shape(g, nq)[0]
    lens = sorted({window + nq + 700, window + nq, window + nq + 64, window + nq + chunk - 1, window + nq + chunk,
                   window + chunk + 64, 2 * chunk + nq, CAP - 1, CAP - 64})
    assert all(window + nq <= x < CAP for x in lens)
    Q, K, V = _inputs(g, nq, d, vd, CAP, len(lens), seed=7 * nq + d + window)
    Q, K, V, planted = WB.plant(Q, K, V, lens, window, g)
    assert len(planted) == len(lens) * len(WB.beacon_queries(g, nq))  # no planted row is skipped
    assert {q for _, q, _ in planted} >= {0, pb - 1, pb, nq - 1}
    scales, Kref, Vref = (None, None), K, V
    if form.endswith("fp8"):
        # (the cache rounds the beacons like every other value: the reference is the dequantized cache.  Unit scales: a
        # k_scale's mantissa would enter the pre-scale of Q, for which the beacons' query value was chosen)
        K, V, scales, Kref, Vref = _quantize(K, V, 1, unit=True)
    table = _table(len(lens), CAP // page, seed=nq)
    got = _run(form, g, _dev(Q), *_stores(form, K, V, table, page), lens, window, table=table, scales=scales)
    res = tw._check_window(got, Q, Kref, Vref, lens, g, window)
    print(f"beacons g={g} nq={nq} d={d} W={window} {form}: {res}")
    if form == "ragged":
        o = got[0].cpu().numpy().astype(np.float64)
        for s, q, vch in planted:  # every beaconed query answers (x + y) / 2 on its channels
            x, y = WB.values(len(vch))
            assert np.abs(o[s * g:(s + 1) * g][:, vch, q] - (x.astype(np.float64) + y) / 2).max() < 0.03, (s, q)
        # the semantic control: the un-windowed query-blocked call on the same inputs also sees the key below the
        # window, and misses the reference grossly on every planted row
        tail = _run(form, g, _dev(Q), _dev(K), _dev(V), lens, window, kind="_prefill")[0].cpu().numpy().astype(np.float64)
        ref = window_ref.forward_f64(Q, K, V, lens, window, g)[0]
        for s, q, vch in planted:
            assert np.abs(tail[s * g, :, q] - ref[s * g, :, q]).max() >= window_ref.BEACON_V / 4, (s, q)


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("page,max_pages", [(64, 40), (128, 20), (192, 14)])
@pytest.mark.parametrize("g,nq,window", [(1, 129, 1), (8, 37, 65), (16, 20, 600), (4, 33, 513), (1, 256, 2000)])
def test_paged_is_ragged_on_the_gathered_cache(g, nq, window, page, max_pages):
    cap, d = page * max_pages, 64
    chunk = _plan(nq, cap, d, d, g, window, page)[1]
    lens = _lengths(g, nq, cap, chunk, window)
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=page + nq)
    K8, V8, scales, _, _ = _quantize(K, V, 1)
    table = _table(len(lens), max_pages, seed=page)
    tq = _dev(Q)
    assert _same(_run("paged", g, tq, *_stores("paged", K, V, table, page), lens, window, table=table),
                 _run("ragged", g, tq, _dev(K), _dev(V), lens, window))
    assert _same(_run("paged_fp8", g, tq, *_stores("paged", K8, V8, table, page), lens, window, table=table, scales=scales),
                 _run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, window, scales=scales))


@pytest.mark.parametrize("g,nq,window", [(1, 129, 64), (8, 37, 513), (128, 2, 1000)])
@pytest.mark.parametrize("d,vd", [(64, 64), (40, 72)])
def test_fp8_with_unit_scales_is_the_fp16_forward_on_the_converted_cache(g, nq, window, d, vd):
    cap, page, max_pages = 2560, 128, 20
    lens = [0, nq - 1, nq + 70, window + nq + 70, 1030, cap]
    Q, K, V = _inputs(g, nq, d, vd, cap, len(lens), seed=nq)
    K8, V8, unit, Kd, Vd = _quantize(K, V, 1, unit=True)
    K16, V16 = Kd.astype(np.float16), Vd.astype(np.float16)
    assert np.array_equal(K16.astype(np.float64), Kd)
    table = _table(len(lens), max_pages, seed=3)
    tq = _dev(Q)
    ref = _run("ragged", g, tq, _dev(K16), _dev(V16), lens, window)
    assert _same(_run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, window, scales=unit), ref)
    assert _same(_run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, window), ref)  # null scales
    assert _same(_run("paged_fp8", g, tq, *_stores("paged", K8, V8, table, page), lens, window, table=table, scales=unit), ref)


def _form_case(form, g, nq, d, cap, page, lens, seed):
    """Q, what the form reads (device), and the keywords of _run"""
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=seed)
    kw = dict(scales=(None, None))
    if form.endswith("fp8"):
        K, V, kw["scales"], _, _ = _quantize(K, V, 1)
    if form.startswith("paged"):
        kw["table"] = _table(len(lens), cap // page, seed=seed + 1)
    tk, tv = _stores(form, K, V, kw.get("table"), page)
    return _dev(Q), tk, tv, kw


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("g,nq", [(1, 129), (8, 37), (4, 7)])
def test_a_window_that_reaches_the_capacity_is_the_query_blocked_tail_call(g, nq, form):
    """window = capacity, capacity + 1 and INT32_MAX: fa_forward_*_prefill with tail_causal = 1, with its plan and its
    workspace size ((4, 7): one block, which that call hands to the un-blocked twin in turn)"""
    cap, page, d = CAP, 64, 64
    lens = [0, nq - 1, 700, 1030, cap]
    tq, tk, tv, kw = _form_case(form, g, nq, d, cap, page, lens, seed=nq + g)
    st, *ref = _abi(form, g, tq, tk, tv, lens, 0, kind="_prefill", **kw)
    assert st == 0
    parent = _plan(nq, cap, d, d, g, 0, kind="_prefill")
    for window in (cap, cap + 1, 2 ** 31 - 1):
        plan = _plan(nq, cap, d, d, g, window)
        assert plan[7] == 1 and plan[:2] == parent[:2] and plan[4:7] == parent[2:5]
        st, *got = _abi(form, g, tq, tk, tv, lens, window, **kw)
        assert st == 0 and got[4] == ref[4] and _same(got[:3], ref[:3]), window


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("g,nq", [(1, 128), (8, 16), (4, 7), (128, 1), (3, 32)])
def test_one_block_is_the_windowed_twin(g, nq, form):
    """kv_group * next_pow2(nq) <= 128 under a window below the capacity: the plan says delegated = 2, with the
    windowed twin's chunks and workspace size, and the bits are the twin's."""
    cap, page, d = CAP, 64, 64
    lens = [0, nq - 1, 700, 1030, cap]
    tq, tk, tv, kw = _form_case(form, g, nq, d, cap, page, lens, seed=nq + g)
    for window in (1, 65, 600, cap - 1):
        plan, twin = _plan(nq, cap, d, d, g, window), _plan(nq, cap, d, d, g, window, kind="_window")
        assert plan[7] == 2 and plan[6] == 1 and plan[:4] == twin[:4]
        st, *ref = _abi(form, g, tq, tk, tv, lens, window, kind="_window", **kw)
        st2, *got = _abi(form, g, tq, tk, tv, lens, window, **kw)
        assert st == 0 and st2 == 0 and got[4] == ref[4] and _same(got[:3], ref[:3]), window


@pytest.mark.parametrize("form", ["ragged", "paged_fp8"])
@pytest.mark.parametrize("g,nq", [(1, 256), (8, 32), (1, 384)])
def test_a_full_block_is_the_windowed_twin_on_a_copy_of_its_queries(g, nq, form):
    """What a caller ran before: fa_forward_*_window on a contiguous copy of Q[..., q0:q0 + P_b] with the lengths
    shifted by the queries behind the block.  Both plans cut the capacity into the same chunks here (rows = 128, and
    the twins' min_chunk of 1024 decides both), which the test asserts first, so the bits agree."""
    cap, page, d = CAP, 128, 64
    pb, nqb = B.block_shape(g, nq)
    assert nq == nqb * pb
    lens = np.array([0, pb - 1, nq - 1, nq + 3, 600 + nq, 1024 + pb, 1025, 1700, cap])
    tq, tk, tv, kw = _form_case(form, g, nq, d, cap, page, lens, seed=nq)
    for window in (2, 65, 600):
        plan, twin = _plan(nq, cap, d, d, g, window), _plan(pb, cap, d, d, g, window, kind="_window")
        assert plan[7] == 0 and twin[6] == 0 and plan[1] == twin[1] == 1024
        got = _run(form, g, tq, tk, tv, lens, window, **kw)
        for qb in range(nqb):
            q0 = qb * pb
            ref = _run(form, g, tq[:, :, q0:q0 + pb].contiguous(), tk, tv, lens - (nq - q0 - pb), window, kind="_window", **kw)
            assert _same([got[0][:, :, q0:q0 + pb], got[1][:, q0:q0 + pb], got[2][:, q0:q0 + pb]], ref), (window, qb)


@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_two_calls_are_equal_and_a_sequence_does_not_depend_on_the_batch(form):
    g, nq, d, vd, hk, page, max_pages, window = 8, 37, 40, 72, 2, 192, 14, 300
    cap = page * max_pages
    Q, K, V = _inputs(g, nq, d, vd, cap, 3 * hk, seed=17)
    kw = {}
    if form == "paged":
        kw["table"] = _table(3, max_pages, seed=4)
    tq = _dev(Q)
    tk, tv = _stores(form, K, V, kw.get("table"), page, hk)
    a = _run(form, g, tq, tk, tv, [1101, 333, 40], window, hk=hk, **kw)
    assert _same(a, _run(form, g, tq, tk, tv, [1101, 333, 40], window, hk=hk, ws_fill=0xFF, **kw))
    q1 = slice(hk * g, 2 * hk * g)
    others = _run(form, g, tq, tk, tv, [0, 333, cap], window, hk=hk, **kw)
    assert _same([t[q1] for t in others], [t[q1] for t in a])
    if form == "paged":
        alone = _run(form, g, tq[q1].contiguous(), tk, tv, [333], window, hk=hk, table=kw["table"][1:2])
    else:
        alone = _run(form, g, tq[q1].contiguous(), tk[hk:2 * hk].contiguous(), tv[hk:2 * hk].contiguous(), [333], window, hk=hk)
    assert _same([t[q1] for t in a], alone)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_python_wrapper_is_the_abi_call(form, fp8):
    """Leading batch axes [2, 3] with Hk = 2 (kv_per_len = 2, one length per sequence), and no batch axis; a window
    below the capacity, one that reaches it (delegated) and one above 2^31 (clamped)."""
    g, nq, d, hk, page, max_pages = 4, 33, 64, 2, 64, 18
    cap = page * max_pages
    lens = [[cap, 5, 513], [0, 700, 64]]
    Q, K, V = _inputs(g, nq, d, d, cap, 6 * hk, seed=9)
    scales, kws = (None, None), {}
    if fp8:
        K, V, scales, _, _ = _quantize(K, V, hk)
        kws = dict(k_scale=scales[0], v_scale=scales[1])
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
    tq = _dev(Q)
    table = _table(6, max_pages, seed=5)
    tk, tv = _stores(form, K, V, table, page, hk)
    tt = _dev(table)
    name = form + ("_fp8" if fp8 else "")
    for window, sent in ((300, 300), (cap, cap), (2 ** 40, 2 ** 31 - 1)):
        if form == "paged":
            direct = _run(name, g, tq, tk, tv, tl.reshape(-1), sent, hk=hk, table=tt, scales=scales)
            got = fa.paged_window_prefill_1d(tq.reshape(2, 3, hk * g, d, nq), tk, tv, tt.reshape(2, 3, max_pages), tl, window,
                                             returning_l_m=True, **kws)
            one = fa.paged_window_prefill_1d(tq[hk * g:2 * hk * g], tk, tv, tt[1], tl[0, 1], window, returning_l_m=True, **kws)
        else:
            direct = _run(name, g, tq, tk, tv, tl.reshape(-1), sent, hk=hk, scales=scales)
            got = fa.ragged_window_prefill_1d(tq.reshape(2, 3, hk * g, d, nq), tk.reshape(2, 3, hk, d, cap),
                                              tv.reshape(2, 3, hk, d, cap), tl, window, returning_l_m=True, **kws)
            one = fa.ragged_window_prefill_1d(tq[hk * g:2 * hk * g], tk[hk:2 * hk], tv[hk:2 * hk], tl[0, 1], window,
                                              returning_l_m=True, **kws)
        torch.cuda.synchronize()
        assert got[0].shape == (2, 3, hk * g, d, nq) and got[1].shape == got[2].shape == (2, 3, hk * g, nq)
        assert _same([t.reshape(r.shape) for t, r in zip(got, direct)], direct)
        assert _same(one, [t[hk * g:2 * hk * g] for t in direct])


# ------------------------------------------------------------------ isolation
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("g,nq,window,d", [(8, 37, 300, 64), (1, 129, 64, 64), (16, 20, 513, 40)])
def test_what_lies_outside_the_calls_window_tiles_does_not_reach_the_result(form, g, nq, window, d):
    """Every key at or past L and every key of a tile wholly below the call's lowest window start
    lo = max(0, L - nq - W + 1), and every pool page that no sequence owns, hold NaN, Inf or 65504 (FP8: 0x7F, 0xFF,
    0x7E); the workspace 0xFF bytes; the table entries of pages wholly below floor(lo / 64) * 64 and past the last
    live page INT32_MIN, -1 or INT32_MAX: bitwise the clean call (zeros and valid entries there)."""
    paged, fp8 = form.startswith("paged"), form.endswith("fp8")
    page, max_pages = 128, 20
    cap = page * max_pages
    chunk = _plan(nq, cap, d, d, g, window)[1]
    lens = _lengths(g, nq, cap, chunk, window)
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=41 + nq)
    scales = (None, None)
    if fp8:
        K, V, scales, _, _ = _quantize(K, V, 1)
    Lc = np.clip(np.asarray(lens), 0, cap)
    lo64 = np.array([window_ref.window_lo(x, nq, window, cap) // 64 * 64 for x in lens])
    j = np.arange(cap)[None, :]
    dead = ((j < lo64[:, None]) | (j >= Lc[:, None]))[:, None, :]
    assert dead[:, 0, :].sum() > cap and (lo64 > 0).any()
    pages = np.arange(max_pages)[None, :]
    dead_page = ((pages + 1) * page <= lo64[:, None]) | (pages * page >= Lc[:, None])
    assert ((pages + 1) * page <= lo64[:, None]).any()
    table = _table(len(lens), max_pages, seed=6)
    tq = _dev(Q)

    def call(fill, entry=None, ws_fill=None):
        k, v = np.where(dead, fill, K).astype(K.dtype), np.where(dead, fill, V).astype(V.dtype)
        if not paged:
            return _run(form, g, tq, _dev(k), _dev(v), lens, window, scales=scales, ws_fill=ws_fill, fill=0x5A)
        t = table if entry is None else np.where(dead_page, entry, table).astype(np.int32)
        return _run(form, g, tq, _dev(_scatter(k, table, page, 1, fill)), _dev(_scatter(v, table, page, 1, fill)), lens, window,
                    table=t, scales=scales, ws_fill=ws_fill, fill=0x5A)

    ref = call(np.uint8(0) if fp8 else np.float16(0))
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    poisons = [np.uint8(0x7F), np.uint8(0xFF), np.uint8(0x7E)] if fp8 else [np.float16(np.nan), np.float16(np.inf), np.float16(65504)]
    for poison, entry in zip(poisons, (INT32_MIN, -1, INT32_MAX)):
        assert _same(call(poison, entry, ws_fill=0xFF), ref), (poison, entry)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", FORMS)
def test_refusals_write_nothing(form):
    """A workspace one byte short, a window of 0 and a shape outside the envelope (136 channels), un-delegated and under
    both delegations: the status, and the 0xA5-filled outputs and workspace are untouched."""
    page, max_pages = 64, 4
    cap = page * max_pages
    for g, nq in ((8, 37), (4, 7)):
        for window in (100, cap):
            for d, short, w, want in ((64, 1, window, _lib.FA_ERR_WORKSPACE_TOO_SMALL), (64, 0, 0, _lib.FA_ERR_INVALID_ARGUMENT),
                                      (136, 0, window, _lib.FA_ERR_UNSUPPORTED)):
                Q, K, V = _inputs(g, nq, d, d, cap, 2, seed=d)
                kw = {}
                if form.endswith("fp8"):
                    K, V = K.view(np.uint8)[:, :, :cap].copy(), V.view(np.uint8)[:, :, :cap].copy()
                if form.startswith("paged"):
                    kw["table"] = _table(2, max_pages, seed=8)
                    K, V = _scatter(K, kw["table"], page, 1, 0), _scatter(V, kw["table"], page, 1, 0)
                st, o, l, m, ws, need = _abi(form, g, _dev(Q), _dev(K), _dev(V), [cap, 100], w, fill=0xA5, ws_fill=0xA5,
                                             ws_short=short, **kw)
                assert st == want and (need > 0) == (d == 64 and w > 0), (g, nq, window, d, w, _lib.last_error())
                for t in (o, l, m, ws):
                    assert bool((t.view(torch.uint8) == 0xA5).all())


@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_an_empty_batch_is_ok(form):
    L = _lib.lib()
    prob = P._problem(200, 2560, 64, 64, 0)
    ws = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    if form == "ragged":
        st = L.fa_forward_ragged_window_prefill(None, prob, 4, None, None, None, None, 2, 300, None, None, None, ws.data_ptr(), 0)
    else:
        st = L.fa_forward_paged_window_prefill(None, prob, 4, None, None, None, None, 40, 64, 8, None, 2, 300, None, None,
                                               None, ws.data_ptr(), 0)
    assert st == _lib.FA_OK


# ------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_a_captured_call_follows_the_lengths_the_table_the_pools_and_the_scales(fp8):
    """paged_window_prefill_1d captured in a (linear, one-stream) graph; between replays k_lens, the table, the pools
    and the scales are overwritten in place, so that a block's window start crosses a chunk edge, a block's key end
    crosses one and a block turns empty.  Every replay is bitwise the eager call on the same values."""
    g, nq, d, hk, page, max_pages, seqs, window = 8, 37, 64, 2, 64, 40, 3, 300
    cap = page * max_pages
    launched, chunk, span_w, cap_chunks, pb, rows, nqb = _plan(nq, cap, d, d, g, window, page)[:7]
    assert (launched, chunk, pb, nqb) == (2, 1024, 16, 3)
    Q, K, V = _inputs(g, nq, d, d, cap, seqs * hk, seed=31)
    scales = (None, None)
    if fp8:
        K, V, scales, _, _ = _quantize(K, V, hk)
    fill = 0x7F if fp8 else np.nan
    tables = [_table(seqs, max_pages, seed=s) for s in (10, 11)]
    pools = [(_scatter(K, t, page, hk, fill), _scatter(V, t, page, hk, fill)) for t in tables]
    # block 0 (behind = 21, nq_b = 16): L_b = L - 21, lo_b = L_b - 315.  1360 -> lo_b = 1024 (chunk 1's first key),
    # 1359 -> 1023 (chunk 0's last); 1045 -> L_b = 1024, 1046 -> 1025; 21 -> L_b = 0 (empty)
    steps = [([1360, 2560, 40], 0, 1.0), ([1359, 21, 2559], 1, 0.5), ([1045, 1024, 1046], 0, 3.0), ([20, 1361, 5], 1, 1.0)]
    ends, los = zip(*(_blocks(g, nq, L, cap, window) for L, _, _ in steps))
    assert los[0][0, 0] == 1024 and los[1][0, 0] == 1023 and ends[2][0, 0] == 1024 and ends[2][2, 0] == 1025
    assert ends[1][1, 0] == 0 and ends[1][1, 1] > 0
    tq = _dev(Q.reshape(seqs, hk * g, d, nq))
    kp, vp = _dev(pools[0][0]), _dev(pools[0][1])
    tt, tl = _dev(tables[0]), torch.tensor(steps[0][0], dtype=torch.int32, device="cuda:0")
    live = dict(k_scale=scales[0].clone(), v_scale=scales[1].clone()) if fp8 else {}
    with torch.no_grad():
        fa.paged_window_prefill_1d(tq, kp, vp, tt, tl, window, **live)  # (first launches raise the LDS limit)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fa.paged_window_prefill_1d(tq, kp, vp, tt, tl, window, returning_l_m=True, **live)
        for L, which, mul in steps:
            tl.copy_(torch.tensor(L, dtype=torch.int32))
            tt.copy_(torch.from_numpy(tables[which]))
            kp.copy_(torch.from_numpy(pools[which][0]))
            vp.copy_(torch.from_numpy(pools[which][1]))
            now = {}
            if fp8:
                live["k_scale"].copy_(scales[0] * mul)
                live["v_scale"].copy_(scales[1] / mul)
                now = dict(k_scale=scales[0] * mul, v_scale=scales[1] / mul)
            graph.replay()
            torch.cuda.synchronize()
            eager = fa.paged_window_prefill_1d(_dev(Q.reshape(seqs, hk * g, d, nq)), _dev(pools[which][0]), _dev(pools[which][1]),
                                               _dev(tables[which]), torch.tensor(L, dtype=torch.int32, device="cuda:0"),
                                               window, returning_l_m=True, **now)
            torch.cuda.synchronize()
            assert _same(out, eager), L
        del graph


# ------------------------------------------------------------------ staircase scores
def test_staircase_scores():
    """tests/score_ramp.py's staircase inputs of test_gpu_prefill.STAIRS' tail case through the ragged and the paged
    form at W = capacity - 1: every length lies below the capacity, so the window cuts nothing, the mask is the tail
    mask the inputs were built for, and the call is not delegated.  The lazy rebase runs in a block with q0 > 0
    (asserted from the rebase model over this plan's chunks), and the merge weighs chunks that underflow."""
    case = P.STAIRS[0]
    assert case.tail and max(case.lens) < case.cap
    made = R.decode_inputs(case)
    g, nq, d, cap, window = case.g, case.nq, case.d, case.cap, case.cap - 1
    launched, chunk, span_w, cap_chunks, pb, rows, nqb, delegated = _plan(nq, cap, d, case.vd, g, window)
    assert (launched, chunk, delegated) == (3, 1024, 0)
    later = 0
    for bi, info in enumerate(made["infos"]):
        L = made["lens"][bi // g]
        if info is None:
            continue
        scores = R.kernel_scores(made["Q"][bi][None], made["K"][bi // g][None, :, :L], d, True)
        for c in range(launched):  # lo_b = 0: relative chunk c is absolute chunk c
            k0, k1 = c * chunk, min((c + 1) * chunk, L)
            if k0 < L:
                later += int(R.rebase_tiles(scores[pb:, k0:k1], info["mask"][pb:, k0:k1], 64, 8.0)[0].sum())
    assert later > 0
    tq = _dev(made["Q"])
    got = _run("ragged", g, tq, _dev(made["K"]), _dev(made["V"]), made["lens"], window)
    res = rg._check_ref(got, made["Q"], made["K"], made["V"], made["lens"], g, True, m_bound=made["bound"])
    print(case.id, {k: round(v, 3) for k, v in res.items()}, "rebases in blocks behind the first:", later)
    page = case.pages[0]
    table = _table(len(made["lens"]), cap // page, seed=12)
    paged = _run("paged", g, tq, *_stores("paged", made["K"], made["V"], table, page), made["lens"], window, table=table)
    assert _same(paged, got)


# ------------------------------------------------------------------ seeded sweep
SWEEP_SEED, SWEEP_N = 20241021, 60


def _draw(rng):
    g = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32, 128]))
    pb = B.block_shape(g, 1)[0]
    nq = int(rng.integers(pb + 1, min(300, 6 * pb) + 1))
    d, vd = CHANNELS[int(rng.integers(4))] if rng.random() < 0.7 else (int(rng.integers(1, 129)), int(rng.integers(1, 129)))
    form = FORMS[int(rng.integers(4))]
    page = int(rng.choice([64, 128, 192]))
    cap = page * int(rng.integers(1, 2700 // page + 1)) if form.startswith("paged") else int(rng.integers(2, 2701))
    window = int(rng.choice([1, 2, 63, 64, 65, 512, int(rng.integers(1, cap)), cap - 1]))
    window = min(max(window, 1), cap - 1)
    nseq = int(rng.integers(1, 4))
    lens = [int(rng.choice([0, 1, nq - 1, nq, nq + window, cap, cap + 5, int(rng.integers(0, cap + 1))])) for _ in range(nseq)]
    return dict(g=g, nq=nq, d=d, vd=vd, form=form, page=page, cap=cap, window=window, lens=lens)


def test_seeded_sweep():
    """SWEEP_N = 60 draws from seed SWEEP_SEED over (form, g, nq <= 300, W, d, v_d, cap <= 2700, page, lengths), each
    undelegated and checked against the reference, none skipped."""
    rng = np.random.default_rng(SWEEP_SEED)
    worst, most_blocks, empty_block = {}, 0, False
    for i in range(SWEEP_N):
        c = _draw(rng)
        g, nq, d, vd, cap, lens, form, window = c["g"], c["nq"], c["d"], c["vd"], c["cap"], c["lens"], c["form"], c["window"]
        plan = _plan(nq, cap, d, vd, g, window)
        assert plan[7] == 0 and plan[0] >= 1, c
        most_blocks = max(most_blocks, plan[6])
        empty_block |= bool((_blocks(g, nq, lens, cap, window)[0] == 0).any())
        mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
        Q, K, V = mk(len(lens) * g, d, nq), mk(len(lens), d, cap), mk(len(lens), vd, cap)
        scales, Kref, Vref = (None, None), K, V
        if form.endswith("fp8"):
            K, V, scales, Kref, Vref = _quantize(K, V, 1)
        table = _table(len(lens), max(cap // c["page"], 1), seed=i) if form.startswith("paged") else None
        got = _run(form, g, _dev(Q), *_stores(form, K, V, table, c["page"]), lens, window, table=table, scales=scales)
        try:
            res = tw._check_window(got, Q, Kref, Vref, lens, g, window)
        except AssertionError as e:
            raise AssertionError(f"draw {i}: {c}: {e}") from e
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert most_blocks >= 3 and empty_block
    print(f"{SWEEP_N} draws from seed {SWEEP_SEED}, worst error / allowance {worst}")
