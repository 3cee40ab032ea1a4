"""GPU tests of the query-blocked forwards (csrc/fa_fwd_f16_prefill.h and the four fa_fwd_f16_prefill_*.hip,
fa_forward_ragged_prefill / fa_forward_paged_prefill and their _fp8 forms, flash_attention.ragged_prefill_1d /
paged_prefill_1d): the ragged and paged forwards for any number of queries, worked in blocks of
P_b queries, one workgroup per (K/V slice, query block, key chunk).

Parity is against tests/ragged_ref.py under test_gpu_ragged._check_ref's rule (an FP8 cache: on the dequantized
cache), at the smallest shapes where each piece can go wrong (SHAPES) and at lengths that put a block's key end L_b at
0, at 1 and on either side of a tile and a chunk edge.  The trap shapes and (1, 256) also run the beacon inputs of
tests/prefill_beacons.py, which turn a key bound that is off by one into a gross error
(tests/test_prefill_ref.py).  (A build whose core takes a wave's last lane from the whole call's query count fails
test_parity_ragged at (8, 17) and (16, 20) and test_beacons at (16, 20).)  Everything else is bitwise: paged = ragged on the gathered cache, FP8 with unit scales
= fp16 on the converted cache, one block = the twin, a block = the twin on a contiguous copy of its Q slice with
shifted lengths, the wrapper = the ABI call, poison, and a captured graph."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import paged_ref
from tests import prefill_beacons as B
from tests import ragged_ref
from tests import score_ramp as R
from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SPARE = 3  # pool pages that no sequence owns
FORMS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]

# (g, nq): P_b and what the shape exercises
SHAPES = [(1, 129),    # 128: the second block has one query
          (1, 256),    # 128: two full blocks
          (4, 33),     # 32: a second block
          (8, 17),     # 16: a second block; lane nq - 1 - wq0 of the WHOLE call's nq is query 0 of the second head
          (8, 37),     # 16: a short last block behind two full ones
          (16, 20),    # 8: the lane trap: lane nq - 1 - wq0 of the whole call's nq is query 3 of a block of 8
          (3, 40),     # 32: 96 rows
          (5, 40),     # 16: 80 rows
          (128, 2)]    # 1: one query per block
CHANNELS = [(32, 32), (64, 64), (128, 128), (40, 72)]
K_SCALE, V_SCALE = 0.37, 2.75  # non-unit, not powers of two


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _problem(nq, cap, d, vd, b):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, vd)


def _plan(nq, cap, d, vd, g, page=None):
    out = (ctypes.c_int32 * 8)()
    L = _lib.lib()
    p = _problem(nq, cap, d, vd, g)
    assert (L.fa_forward_ragged_prefill_plan(p, g, out) if page is None else L.fa_forward_paged_prefill_plan(p, g, page, out)) == 0
    return tuple(out)


def _same(a, b):
    return rg._same(a, b)


def _abi(form, g, Q, K, V, lens, tail, hk=1, table=None, scales=(None, None), fill=None, ws_fill=None, ws_short=0,
         twin=False, page=None, cap=None):
    """One of the four forwards (twin: the un-blocked entry point of the same form) on device tensors.  K / V: the
    padded cache [bkv, c, cap] or, for a paged form, the pools [num_pages, hk, c, page] with ``table``
    [sequences, max_pages].  Returns (status, O, l, m, workspace, workspace bytes)."""
    L = _lib.lib()
    b, d, nq = Q.shape
    paged, fp8 = form.startswith("paged"), form.endswith("fp8")
    as_dev = lambda x: x if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), dtype=torch.int32, device=Q.device)  # noqa: E731
    lens = as_dev(lens)
    if paged:
        table = as_dev(table)
        num_pages, vd, pg = V.shape[0], V.shape[2], V.shape[3]
        page = pg if page is None else page
        max_pages = table.shape[-1]
        cap = max_pages * page if cap is None else cap
    else:
        vd, cap = V.shape[1], V.shape[2]
    prob = _problem(nq, cap, d, vd, b)
    out = (torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device),
           torch.empty((b, nq), dtype=torch.float32, device=Q.device),
           torch.empty((b, nq), dtype=torch.float16, device=Q.device))
    if fill is not None:
        for t in out:
            t.view(torch.uint8).fill_(fill)
    mid = "" if twin else "_prefill"
    wsfn = getattr(L, f"fa_forward_{'paged' if paged else 'ragged'}{mid}_workspace_bytes")
    need = int(wsfn(prob, g, page) if paged else wsfn(prob, g))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    fn = getattr(L, f"fa_forward_{'paged' if paged else 'ragged'}{mid}{'_fp8' if fp8 else ''}")
    sc = [None if s is None else s.data_ptr() for s in scales] if fp8 else []
    where = [table.data_ptr(), max_pages, page, num_pages] if paged else []
    st = fn(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), *sc, *where,
            lens.data_ptr(), hk, int(tail), *(t.data_ptr() for t in out), ws.data_ptr(), max(need - ws_short, 0))
    torch.cuda.synchronize()
    return (st,) + out + (ws, need)


def _run(form, g, Q, K, V, lens, tail, **kw):
    st, *got = _abi(form, g, Q, K, V, lens, tail, **kw)
    assert st == 0, _lib.last_error()
    return got[:3]


def _scatter(cache, table, page, hk, fill):
    """The padded cache [seqs * hk, c, cap] as a pool [num_pages, hk, c, page] through ``table``; the SPARE pages
    that the table does not name hold ``fill``."""
    seqs, max_pages = table.shape
    c = cache.shape[1]
    pool = np.full((seqs * max_pages + SPARE, hk, c, page), fill, cache.dtype)
    pool[table] = cache.reshape(seqs, hk, c, max_pages, page).transpose(0, 3, 1, 2, 4)
    return pool


def _table(seqs, max_pages, seed):
    n = seqs * max_pages + SPARE
    return np.random.default_rng(seed).permutation(n)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)


def _quantize(K, V, hk, unit=False):
    """(K8, V8, scales as device tensors, the dequantized float64 K and V) with one scale pair per K/V head."""
    ks = np.full(hk, 1.0 if unit else K_SCALE, np.float32) * (1 + np.arange(hk, dtype=np.float32))
    vs = np.full(hk, 1.0 if unit else V_SCALE, np.float32) / (1 + np.arange(hk, dtype=np.float32))
    if unit:
        ks[:], vs[:] = 1.0, 1.0
    byhead = lambda x: x.reshape((-1, hk) + x.shape[1:])  # noqa: E731
    K8, V8 = fp8_ref.quantize(byhead(K), ks, 1).reshape(K.shape), fp8_ref.quantize(byhead(V), vs, 1).reshape(V.shape)
    Kd, Vd = fp8_ref.dequantize(byhead(K8), ks, 1).reshape(K.shape), fp8_ref.dequantize(byhead(V8), vs, 1).reshape(V.shape)
    return K8, V8, (_dev(ks), _dev(vs)), Kd, Vd


def _lengths(g, nq, cap, chunk):
    """0; 1; nq - 1; nq; nq + 1; what puts block 0's and the last block's key end at 0, at 1, and on either side of
    a tile edge and of a chunk edge; the capacity; the capacity + 5 (clamped)."""
    pb, nqb = B.block_shape(g, nq)
    first = nq - min(pb, nq)  # L_b of block 0 is L - first
    cand = {0, 1, nq - 1, nq, nq + 1, cap, cap + 5}
    for edge in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1):
        cand |= {edge, edge + first}
    return sorted(x for x in cand if 0 <= x <= cap + 5)


@functools.lru_cache(maxsize=None)
def _inputs(g, nq, d, vd, cap, nseq, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(nseq * g, d, nq), mk(nseq, d, cap), mk(nseq, vd, cap)


def _block_ends(g, nq, lens, cap, tail):
    pb, nqb = B.block_shape(g, nq)
    L = np.clip(np.asarray(lens), 0, cap)
    ends = np.stack([np.clip(L - nq + min(nq, (qb + 1) * pb), 0, L) if tail else L for qb in range(nqb)], axis=1)
    return ends  # [sequences, nqb]


# ------------------------------------------------------------------ parity, the ragged forms
@pytest.mark.parametrize("cap", [192, 1100, 2560])
@pytest.mark.parametrize("g,nq", SHAPES)
def test_parity_ragged(g, nq, cap):
    """Both rules, the fp16 and the FP8 cache (non-unit scales).  cap = 1100 is no multiple of 8 (element-wise
    staging), 2560 is three chunks of 1024 where there are two or three blocks."""
    d, vd = CHANNELS[(SHAPES.index((g, nq)) + [192, 1100, 2560].index(cap)) % 4]
    chunks, chunk, pb, rows, nqb, delegated = _plan(nq, cap, d, vd, g)[:6]
    assert delegated == 0 and (pb, nqb) == B.block_shape(g, nq) and rows == g * pb
    if cap == 2560 and nqb <= 21:
        assert (chunks, chunk) == (3, 1024)
    lens = _lengths(g, nq, cap, chunk)
    Q, K, V = _inputs(g, nq, d, vd, cap, len(lens), seed=cap + nq)
    K8, V8, scales, Kd, Vd = _quantize(K, V, 1)
    tq = _dev(Q)
    for tail in (False, True):
        ends = _block_ends(g, nq, lens, cap, tail)
        if tail:  # the lengths do what _lengths says
            assert {0, 1} <= set(ends[:, 0].tolist()) and {0, 1} <= set(ends[:, -1].tolist())
            assert {63, 64, 65} <= set(ends[:, 0].tolist()) or cap < nq - pb + 65
            assert cap < chunk + nq or {chunk, chunk + 1} <= set(ends[:, 0].tolist())
        res = rg._check_ref(_run("ragged", g, tq, _dev(K), _dev(V), lens, tail), Q, K, V, lens, g, tail)
        res8 = rg._check_ref(_run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, tail, scales=scales), Q, Kd, Vd, lens, g, tail)
        print(f"g={g} nq={nq} cap={cap} d={d} vd={vd} tail={tail}: f16 {res}  fp8 {res8}")


# ------------------------------------------------------------------ parity, the paged forms
@pytest.mark.parametrize("page,max_pages", [(64, 40), (128, 9), (192, 3)])
@pytest.mark.parametrize("g,nq", SHAPES)
def test_parity_paged(g, nq, page, max_pages):
    """Through a random table: bitwise the ragged form on the gathered cache, and against the reference."""
    cap = page * max_pages
    d, vd = CHANNELS[(SHAPES.index((g, nq)) + [64, 128, 192].index(page) + 1) % 4]
    chunks, chunk = _plan(nq, cap, d, vd, g, page)[:2]
    assert _plan(nq, cap, d, vd, g, page) == _plan(nq, cap, d, vd, g)
    lens = _lengths(g, nq, cap, chunk)
    Q, K, V = _inputs(g, nq, d, vd, cap, len(lens), seed=page + nq)
    K8, V8, scales, Kd, Vd = _quantize(K, V, 1)
    table = _table(len(lens), max_pages, seed=page)
    tq = _dev(Q)
    for tail in (False, True):
        got = _run("paged", g, tq, _dev(_scatter(K, table, page, 1, np.nan)), _dev(_scatter(V, table, page, 1, np.nan)), lens,
                   tail, table=table)
        assert _same(got, _run("ragged", g, tq, _dev(K), _dev(V), lens, tail))
        rg._check_ref(got, Q, K, V, lens, g, tail)
        got8 = _run("paged_fp8", g, tq, _dev(_scatter(K8, table, page, 1, 0x7F)), _dev(_scatter(V8, table, page, 1, 0x7F)), lens,
                    tail, table=table, scales=scales)
        assert _same(got8, _run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, tail, scales=scales))
        rg._check_ref(got8, Q, Kd, Vd, lens, g, tail)


# ------------------------------------------------------------------ beacons
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("g,nq,d,vd", [(8, 37, 32, 40), (16, 20, 64, 64), (1, 256, 32, 32), (1, 256, 128, 128)])
def test_beacons(g, nq, d, vd, form):
    """A tower of a score at every block's first and last query's own key and at the key after it, with V of
    opposite sign: a bound that is one key off fails the gate (tests/test_prefill_ref.py)."""
    page, max_pages = 64, 18
    cap = page * max_pages if form.startswith("paged") else 1100
    chunk = _plan(nq, cap, d, vd, g)[1]
    pb = B.block_shape(g, nq)[0]
    # the last two put the newest key of block 0's and of block 1's last query on the first key of a tile (key 128),
    # which no other query of the block sees: a wave bound taken from a lower lane skips that tile
    lens = [nq + 9, nq, 70 + nq, chunk + 3, chunk + nq - 1, cap - 1, nq - 3, 128 + nq - (pb - 1), 128 + nq - (min(nq, 2 * pb) - 1)]
    Q, K, V = _inputs(g, nq, d, vd, cap, len(lens), seed=7 * nq + d)
    Q, K, V, planted = B.plant(Q, K, V, lens, g)
    assert len(planted) >= (len(lens) - 2) * len(B.beacon_queries(g, nq))
    scales, Kref, Vref = (None, None), K, V
    if form.endswith("fp8"):
        # (the beacons' amplitudes are rounded by the cache like every other value: the reference is the dequantized
        # cache, in which the tower is a few percent lower and V's +-A a few percent off)
        K, V, scales, Kref, Vref = _quantize(K, V, 1)
    if form.startswith("paged"):
        table = _table(len(lens), max_pages, seed=nq)
        fill = 0x7F if form.endswith("fp8") else np.nan
        got = _run(form, g, _dev(Q), _dev(_scatter(K, table, page, 1, fill)), _dev(_scatter(V, table, page, 1, fill)), lens, True,
                   table=table, scales=scales)
    else:
        got = _run(form, g, _dev(Q), _dev(K), _dev(V), lens, True, scales=scales)
    res = rg._check_ref(got, Q, Kref, Vref, lens, g, True)
    print(f"beacons g={g} nq={nq} d={d} {form}: {res}")
    if not form.endswith("fp8"):  # every beaconed query answers +A on its channels
        o = got[0].cpu().numpy().astype(np.float64)
        for s, q, pos, vch in planted:
            assert np.abs(o[s * g:(s + 1) * g][:, vch, q] - B.A).max() < 0.02, (s, q, pos)


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("g,nq", [(1, 129), (8, 37), (128, 2)])
def test_fp8_with_unit_scales_is_the_fp16_forward_on_the_converted_cache(g, nq):
    cap, page, max_pages = 1152, 128, 9
    lens = [0, nq - 1, nq + 70, 1030, cap]
    Q, K, V = _inputs(g, nq, 64, 64, cap, len(lens), seed=nq)
    K8, V8, unit, Kd, Vd = _quantize(K, V, 1, unit=True)
    K16, V16 = Kd.astype(np.float16), Vd.astype(np.float16)
    assert np.array_equal(K16.astype(np.float64), Kd)
    table = _table(len(lens), max_pages, seed=3)
    tq = _dev(Q)
    for tail in (False, True):
        ref = _run("ragged", g, tq, _dev(K16), _dev(V16), lens, tail)
        assert _same(_run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, tail, scales=unit), ref)
        assert _same(_run("ragged_fp8", g, tq, _dev(K8), _dev(V8), lens, tail), ref)  # null scales
        assert _same(_run("paged_fp8", g, tq, _dev(_scatter(K8, table, page, 1, 0x7F)), _dev(_scatter(V8, table, page, 1, 0x7F)),
                          lens, tail, table=table, scales=unit), ref)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("g,nq", [(1, 128), (8, 16), (4, 7), (128, 1), (3, 32)])
def test_one_block_is_the_twin(g, nq, form):
    """kv_group * next_pow2(nq) <= 128: the plan says delegated, with the twin's chunks, and the bits are the twin's."""
    cap, page, max_pages, d = 2560, 64, 40, 64
    plan = _plan(nq, cap, d, d, g)
    assert plan[4:6] == (1, 1) and plan[:2] == rg._plan(nq, cap, d, d, g)[:2]
    lens = [0, nq - 1, 700, cap]
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=nq + g)
    scales = (None, None)
    if form.endswith("fp8"):
        K, V, scales, _, _ = _quantize(K, V, 1)
    kw = dict(scales=scales)
    if form.startswith("paged"):
        kw["table"] = _table(len(lens), max_pages, seed=1)
        fill = 0x7F if form.endswith("fp8") else np.nan
        K, V = _scatter(K, kw["table"], page, 1, fill), _scatter(V, kw["table"], page, 1, fill)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    for tail in (False, True):
        assert _same(_run(form, g, tq, tk, tv, lens, tail, **kw), _run(form, g, tq, tk, tv, lens, tail, twin=True, **kw))


@pytest.mark.parametrize("form", ["ragged", "paged_fp8"])
@pytest.mark.parametrize("g,nq", [(1, 256), (8, 32)])
def test_a_block_is_the_twin_on_a_copy_of_its_queries(g, nq, form):
    """What a caller ran before: the twin on a contiguous copy of Q[..., q0:q0 + P_b] with the lengths shifted by the
    queries behind the block (tail) or unchanged (full).  The two plans cut the capacity into the same chunks here,
    which the test asserts first, so the bits agree."""
    cap, page, max_pages, d = 2560, 128, 20, 64
    chunks, chunk, pb, rows, nqb = _plan(nq, cap, d, d, g)[:5]
    assert nq == nqb * pb and (chunks, chunk) == rg._plan(pb, cap, d, d, g)[:2]
    lens = np.array([0, pb - 1, nq - 1, nq + 3, 1024 + pb, 1025, cap])
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=nq)
    kw = dict(scales=(None, None))
    if form.endswith("fp8"):
        K, V, kw["scales"], _, _ = _quantize(K, V, 1)
    if form.startswith("paged"):
        kw["table"] = _table(len(lens), max_pages, seed=2)
        K, V = _scatter(K, kw["table"], page, 1, 0x7F), _scatter(V, kw["table"], page, 1, 0x7F)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    for tail in (False, True):
        got = _run(form, g, tq, tk, tv, lens, tail, **kw)
        for qb in range(nqb):
            q0 = qb * pb
            shifted = lens - (nq - q0 - pb) if tail else lens
            twin = _run(form, g, tq[:, :, q0:q0 + pb].contiguous(), tk, tv, shifted, tail, twin=True, **kw)
            assert _same([got[0][:, :, q0:q0 + pb], got[1][:, q0:q0 + pb], got[2][:, q0:q0 + pb]], twin), (tail, qb)


@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_two_calls_are_equal_and_a_sequence_does_not_depend_on_the_batch(form, tail):
    g, nq, d, vd, hk, page, max_pages = 8, 37, 40, 72, 2, 192, 6
    cap = page * max_pages
    Q, K, V = _inputs(g, nq, d, vd, cap, 3 * hk, seed=17)
    kw = {}
    if form == "paged":
        kw["table"] = _table(3, max_pages, seed=4)
        K, V = _scatter(K, kw["table"], page, hk, np.nan), _scatter(V, kw["table"], page, hk, np.nan)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    a = _run(form, g, tq, tk, tv, [1101, 333, 40], tail, hk=hk, **kw)
    assert _same(a, _run(form, g, tq, tk, tv, [1101, 333, 40], tail, hk=hk, **kw))
    q1 = slice(hk * g, 2 * hk * g)
    others = _run(form, g, tq, tk, tv, [0, 333, 1000], tail, hk=hk, **kw)
    assert _same([t[q1] for t in others], [t[q1] for t in a])
    if form == "paged":
        alone = _run(form, g, tq[q1].contiguous(), tk, tv, [333], tail, hk=hk, table=kw["table"][1:2])
    else:
        alone = _run(form, g, tq[q1].contiguous(), tk[hk:2 * hk].contiguous(), tv[hk:2 * hk].contiguous(), [333], tail, hk=hk)
    assert _same([t[q1] for t in a], alone)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_python_wrapper_is_the_abi_call(form, fp8):
    """Leading batch axes [2, 3] with Hk = 2 (kv_per_len = 2, one length per sequence), and no batch axis."""
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
    if form == "paged":
        table = _table(6, max_pages, seed=5)
        fill = 0x7F if fp8 else np.nan
        tk, tv, tt = _dev(_scatter(K, table, page, hk, fill)), _dev(_scatter(V, table, page, hk, fill)), _dev(table)
    else:
        tk, tv = _dev(K), _dev(V)
    for tail in (False, True):
        if form == "paged":
            direct = _run("paged_fp8" if fp8 else "paged", g, tq, tk, tv, tl.reshape(-1), tail, hk=hk, table=tt, scales=scales)
            got = fa.paged_prefill_1d(tq.reshape(2, 3, hk * g, d, nq), tk, tv, tt.reshape(2, 3, max_pages), tl, tail_causal=tail,
                                      returning_l_m=True, **kws)
            one = fa.paged_prefill_1d(tq[hk * g:2 * hk * g], tk, tv, tt[1], tl[0, 1], tail_causal=tail, returning_l_m=True, **kws)
        else:
            direct = _run("ragged_fp8" if fp8 else "ragged", g, tq, tk, tv, tl.reshape(-1), tail, hk=hk, scales=scales)
            got = fa.ragged_prefill_1d(tq.reshape(2, 3, hk * g, d, nq), tk.reshape(2, 3, hk, d, cap), tv.reshape(2, 3, hk, d, cap),
                                       tl, tail_causal=tail, returning_l_m=True, **kws)
            one = fa.ragged_prefill_1d(tq[hk * g:2 * hk * g], tk[hk:2 * hk], tv[hk:2 * hk], tl[0, 1], tail_causal=tail,
                                       returning_l_m=True, **kws)
        torch.cuda.synchronize()
        assert got[0].shape == (2, 3, hk * g, d, nq) and got[1].shape == got[2].shape == (2, 3, hk * g, nq)
        assert _same([t.reshape(r.shape) for t, r in zip(got, direct)], direct)
        assert _same(one, [t[hk * g:2 * hk * g] for t in direct])


# ------------------------------------------------------------------ poison
@pytest.mark.parametrize("tail", [False, True], ids=["full", "tail"])
@pytest.mark.parametrize("form", FORMS)
def test_nothing_past_a_length_and_no_dead_table_entry_reaches_a_result(form, tail):
    """NaN, Inf and 65504 (an FP8 cache: the codes 0x7F, 0xFF, 0x7E) in every key at or past the length and in the
    pages that no sequence owns, 0xFF bytes in the workspace, and INT32_MIN / -1 / INT32_MAX in the table entries of
    pages without a live key: the bits are those of the call with zeros there and a valid table."""
    g, nq, d, page, max_pages = 8, 37, 64, 64, 18
    paged, fp8 = form.startswith("paged"), form.endswith("fp8")
    cap = page * max_pages if paged else 1100
    chunk = _plan(nq, cap, d, d, g)[1]
    lens = _lengths(g, nq, cap, chunk)
    Q, K, V = _inputs(g, nq, d, d, cap, len(lens), seed=21)
    scales = (None, None)
    if fp8:
        K, V, scales, _, _ = _quantize(K, V, 1)
    past = np.arange(cap)[None, None, :] >= np.clip(np.asarray(lens), 0, cap)[:, None, None]
    table = _table(len(lens), max_pages, seed=6) if paged else None
    tq = _dev(Q)

    def call(fill, bad_entry=None, ws_fill=None):
        k, v = np.where(past, fill, K).astype(K.dtype), np.where(past, fill, V).astype(V.dtype)
        if not paged:
            return _run(form, g, tq, _dev(k), _dev(v), lens, tail, scales=scales, ws_fill=ws_fill)
        t = table.copy()
        if bad_entry is not None:
            dead = np.arange(max_pages)[None, :] * page >= np.clip(np.asarray(lens), 0, cap)[:, None]
            t[dead] = bad_entry
        return _run(form, g, tq, _dev(_scatter(k, table, page, 1, fill)), _dev(_scatter(v, table, page, 1, fill)), lens, tail,
                    table=t, scales=scales, ws_fill=ws_fill)

    zero = np.uint8(0) if fp8 else np.float16(0)
    ref = call(zero)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ref[:2])
    poisons = [np.uint8(0x7F), np.uint8(0xFF), np.uint8(0x7E)] if fp8 else [np.float16(np.nan), np.float16(np.inf), np.float16(65504)]
    for poison, entry in zip(poisons, (INT32_MIN, -1, INT32_MAX)):
        assert _same(call(poison, entry, ws_fill=0xFF), ref), (poison, entry)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", FORMS)
def test_refusals_write_nothing(form):
    """A workspace one byte short, and a shape outside the envelope (136 channels): the status, and the 0xA5-filled
    outputs and workspace are untouched."""
    g, nq, page, max_pages = 8, 37, 64, 4
    cap = page * max_pages
    for d, short, want in ((64, 1, _lib.FA_ERR_WORKSPACE_TOO_SMALL), (136, 0, _lib.FA_ERR_UNSUPPORTED)):
        Q, K, V = _inputs(g, nq, d, d, cap, 2, seed=d)
        kw = {}
        if form.endswith("fp8"):
            K, V = K.view(np.uint8)[:, :, :cap].copy(), V.view(np.uint8)[:, :, :cap].copy()
        if form.startswith("paged"):
            kw["table"] = _table(2, max_pages, seed=8)
            K, V = _scatter(K, kw["table"], page, 1, 0), _scatter(V, kw["table"], page, 1, 0)
        st, o, l, m, ws, need = _abi(form, g, _dev(Q), _dev(K), _dev(V), [cap, 100], True, fill=0xA5, ws_fill=0xA5, ws_short=short,
                                     **kw)
        assert st == want and (need > 0) == (d == 64)
        for t in (o, l, m, ws):
            assert bool((t.view(torch.uint8) == 0xA5).all())


# ------------------------------------------------------------------ graph replay
def test_a_captured_call_follows_the_lengths_the_table_the_pools_and_the_scales():
    """paged_prefill_1d over FP8 pools captured in a (linear, one-stream) graph; between replays k_lens, the table,
    the pools and the scales are overwritten in place, so that one block's key end crosses a chunk edge and another
    block turns empty.  Every replay is bitwise the eager call on the same values."""
    g, nq, d, hk, page, max_pages, seqs = 8, 37, 64, 2, 64, 40, 3
    cap = page * max_pages
    chunks, chunk, pb, rows, nqb = _plan(nq, cap, d, d, g, page)[:5]
    assert (chunks, chunk, pb, nqb) == (3, 1024, 16, 3)
    Q, K, V = _inputs(g, nq, d, d, cap, seqs * hk, seed=31)
    K8, V8, scales, _, _ = _quantize(K, V, hk)
    tables = [_table(seqs, max_pages, seed=s) for s in (10, 11)]
    pools = [(_scatter(K8, t, page, hk, 0x7F), _scatter(V8, t, page, hk, 0x7F)) for t in tables]
    # block 0's key end is L - 21: 1045 -> 1024 (inside chunk 0) and 1046 -> 1025 (into chunk 1); 21 -> 0 (empty)
    steps = [([1045, 2560, 40], 0, 1.0), ([1046, 21, 2559], 1, 0.5), ([20, 1024, 1046], 0, 3.0)]
    for L, _, _ in steps[:2]:
        ends = _block_ends(g, nq, L, cap, True)
        assert (ends[0, 0] <= chunk) != (L[0] == 1046)
    assert _block_ends(g, nq, steps[1][0], cap, True)[1, 0] == 0 and _block_ends(g, nq, steps[1][0], cap, True)[1, 1] > 0
    tq = _dev(Q.reshape(seqs, hk * g, d, nq))
    kp, vp = _dev(pools[0][0]), _dev(pools[0][1])
    tt, tl = _dev(tables[0]), torch.tensor(steps[0][0], dtype=torch.int32, device="cuda:0")
    ks, vs = scales[0].clone(), scales[1].clone()
    with torch.no_grad():
        fa.paged_prefill_1d(tq, kp, vp, tt, tl, tail_causal=True, k_scale=ks, v_scale=vs)  # (first launches raise the LDS limit)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fa.paged_prefill_1d(tq, kp, vp, tt, tl, tail_causal=True, returning_l_m=True, k_scale=ks, v_scale=vs)
        for L, which, mul in steps:
            tl.copy_(torch.tensor(L, dtype=torch.int32))
            tt.copy_(torch.from_numpy(tables[which]))
            kp.copy_(torch.from_numpy(pools[which][0]))
            vp.copy_(torch.from_numpy(pools[which][1]))
            ks.copy_(scales[0] * mul)
            vs.copy_(scales[1] / mul)
            graph.replay()
            torch.cuda.synchronize()
            eager = fa.paged_prefill_1d(_dev(Q.reshape(seqs, hk * g, d, nq)), _dev(pools[which][0]), _dev(pools[which][1]),
                                        _dev(tables[which]), torch.tensor(L, dtype=torch.int32, device="cuda:0"),
                                        tail_causal=True, returning_l_m=True, k_scale=scales[0] * mul, v_scale=scales[1] / mul)
            torch.cuda.synchronize()
            assert _same(out, eager), L
        del graph


# ------------------------------------------------------------------ staircase scores
STAIRS = [R.DecodeCase("prefill-d64-g8q37-tail", "ragged", 64, 64, 8, 37, 2560, (2048 + 148, 2048, 2049, 40, 0, 36, 2048 + 132), True,
                       pages=(64,)),
          R.DecodeCase("prefill-d128-g1q129-full", "ragged", 128, 128, 1, 129, 2560, (2048 + 148, 2048, 2049, 40, 0), False,
                       pages=(128,))]


@pytest.mark.parametrize("case", STAIRS, ids=lambda c: c.id)
def test_staircase_scores(case):
    """tests/score_ramp.py's staircase inputs through the ragged and the paged form: the lazy rebase runs in a block
    with q0 > 0 (asserted from the rebase model over this plan's chunks), and the merge weighs chunks that underflow."""
    made = R.decode_inputs(case)
    g, nq, d, cap = case.g, case.nq, case.d, case.cap
    chunks, chunk, pb = _plan(nq, cap, d, case.vd, g)[:3]
    assert (chunks, chunk) == (3, 1024)
    later = 0
    for bi, info in enumerate(made["infos"]):
        L = made["lens"][bi // g]
        if info is None:
            continue
        scores = R.kernel_scores(made["Q"][bi][None], made["K"][bi // g][None, :, :L], d, True)
        for c in range(chunks):
            k0, k1 = c * chunk, min((c + 1) * chunk, L)
            if k0 < L:
                later += int(R.rebase_tiles(scores[pb:, k0:k1], info["mask"][pb:, k0:k1], 64, 8.0)[0].sum())
    assert later > 0
    tq = _dev(made["Q"])
    got = _run("ragged", g, tq, _dev(made["K"]), _dev(made["V"]), made["lens"], case.tail)
    res = rg._check_ref(got, made["Q"], made["K"], made["V"], made["lens"], g, case.tail, m_bound=made["bound"])
    print(case.id, {k: round(v, 3) for k, v in res.items()}, "rebases in blocks behind the first:", later)
    page = case.pages[0]
    table = _table(len(made["lens"]), cap // page, seed=12)
    paged = _run("paged", g, tq, _dev(_scatter(made["K"], table, page, 1, np.nan)), _dev(_scatter(made["V"], table, page, 1, np.nan)),
                 made["lens"], case.tail, table=table)
    assert _same(paged, got)
    assert np.array_equal(paged_ref.gather(_scatter(made["K"], table, page, 1, np.nan), table, page), made["K"])


# ------------------------------------------------------------------ seeded sweep
def _draw(rng):
    g = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32, 128]))
    pb = B.block_shape(g, 1)[0]
    nq = int(rng.integers(pb + 1, min(300, 6 * pb) + 1))
    d, vd = CHANNELS[int(rng.integers(4))] if rng.random() < 0.7 else (int(rng.integers(1, 129)), int(rng.integers(1, 129)))
    form = FORMS[int(rng.integers(4))]
    page = int(rng.choice([64, 128, 192]))
    cap = page * int(rng.integers(1, 3000 // page + 1)) if form.startswith("paged") else int(rng.integers(1, 3001))
    nseq = int(rng.integers(1, 4))
    lens = [int(rng.choice([0, 1, nq - 1, nq, cap, cap + 5, int(rng.integers(0, cap + 1))])) for _ in range(nseq)]
    return dict(g=g, nq=nq, d=d, vd=vd, form=form, page=page, cap=cap, lens=lens, tail=bool(rng.integers(2)))


def test_seeded_sweep():
    """FA_PREFILL_FUZZ_N (default 100) seeded draws over (g, nq <= 300, d, v_d, cap <= 3000, page, lengths, rule,
    form), each checked against the reference."""
    import os
    n = int(os.environ.get("FA_PREFILL_FUZZ_N", "100"))
    rng = np.random.default_rng(20240607)
    worst = {}
    for i in range(n):
        c = _draw(rng)
        g, nq, d, vd, cap, lens, form = c["g"], c["nq"], c["d"], c["vd"], c["cap"], c["lens"], c["form"]
        assert _plan(nq, cap, d, vd, g)[5] == 0
        mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
        Q, K, V = mk(len(lens) * g, d, nq), mk(len(lens), d, cap), mk(len(lens), vd, cap)
        scales, Kref, Vref = (None, None), K, V
        if form.endswith("fp8"):
            K, V, scales, Kref, Vref = _quantize(K, V, 1)
        kw = dict(scales=scales)
        if form.startswith("paged"):
            kw["table"] = _table(len(lens), cap // c["page"], seed=i)
            fill = 0x7F if form.endswith("fp8") else np.nan
            K, V = _scatter(K, kw["table"], c["page"], 1, fill), _scatter(V, kw["table"], c["page"], 1, fill)
        got = _run(form, g, _dev(Q), _dev(K), _dev(V), lens, c["tail"], **kw)
        try:
            res = rg._check_ref(got, Q, Kref, Vref, lens, g, c["tail"])
        except AssertionError as e:
            raise AssertionError(f"draw {i}: {c}: {e}") from e
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{n} draws, worst error / allowance {worst}")
