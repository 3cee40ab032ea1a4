"""GPU tests of the batch-slab launch loops of csrc/fa_api.hip: fewq_slabs behind fa_forward_ws,
fa_forward_grouped, fa_forward_ragged[_fp8] and fa_forward_paged[_fp8], bwd_slabs behind both forms of
fa_backward_split, and the loops of fa_merge_partials and fa_accumulate_parts.  Their real limits (about 2^31 blocks;
65535 slices, which tests/test_gpu_merge.py reaches) are out of reach, so the DIAGNOSTIC library lowers them to
FA_SLAB_MAX slices (for fa_accumulate_parts: units of 2048 elements) and counts the slab launches in
fa_diag_slab_count().

Every case checks
  (a) the capped call against the same call through the same library without a cap, bit for bit: a slice's bits do
      not depend on how the batch is cut;
  (b) the uncapped call against the float64 reference that the path's own test uses, under that test's tolerances
      (run_case's oracle and bounds; test_gpu_ragged._check_ref on tests/ragged_ref.py, on the cache gathered by
      tests/paged_ref.py, on the cache dequantized by tests/fp8_ref.py; test_gpu_merge.check_merge; the float64 sum);
  (c) the counter: it rose by exactly ceil(slices / cap), so a cap that did nothing fails;
  (d) where the test hands over the workspace itself: the bytes behind the reported size are untouched.
The inputs make a wrong offset a gross error: every sequence has its own length (0, one inside a 64-key tile, the
capacity), every K/V head its own scales, several-fold apart, every sequence its own pages, and Q, K, V are
independent random numbers per slice."""

import ctypes

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import paged_ref
from tests import test_gpu_merge as mg
from tests import test_gpu_parity as parity
from tests import test_gpu_ragged as rg
from tests.gate import U_ROUND
from tests.test_gpu_parity import diag_lib  # noqa: F401  (a fixture)
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}
GUARD = 4096          # bytes behind a workspace
GUARD_BYTE = 0xA5     # what they (and the workspace, before the call) hold


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def _run(monkeypatch, lib, cap, slices, fn):
    """fn() with FA_SLAB_MAX = cap (None: unset) through the diagnostic library ``lib``; the slab counter must rise
    by ceil(slices / cap), by 1 without a cap."""
    if cap is None:
        monkeypatch.delenv("FA_SLAB_MAX", raising=False)
    else:
        monkeypatch.setenv("FA_SLAB_MAX", str(cap))
    before = lib.fa_diag_slab_count()
    out = fn()
    torch.cuda.synchronize()
    rose = lib.fa_diag_slab_count() - before
    assert rose == (1 if cap is None else -(-slices // cap)), (cap, slices, rose)
    return out


def _check_caps(caps, slices, control=()):
    """What the issue asks of a case's caps: at least two slabs each (but for the controls), one short last slab."""
    assert all(-(-slices // c) >= 2 for c in caps if c not in control) and all(c >= slices for c in control)
    assert any(slices % c for c in caps if c < slices)


class Workspace:
    """``nbytes`` of workspace with GUARD bytes behind them, all holding GUARD_BYTE (no kernel may depend on what a
    workspace holds); intact(): the guard is untouched."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.nbytes:] == GUARD_BYTE).all())


def _problem(policy, mode, nq, nk, d, vd, b):
    return _lib.make_problem(_lib.F16, POL[policy], 1, SYNC[mode], b, (nq,), (nk,), d, vd)


def _plan4(fn, prob):
    out = (ctypes.c_int32 * 4)()
    assert fn(prob, out) == _lib.FA_OK
    return tuple(out)


def _np_qkv(b, bkv, d, vd, nq, nk, seed):
    rng = np.random.default_rng(seed)
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    return mk(b, d, nq), mk(bkv, d, nk), mk(bkv, vd, nk), mk(b, vd, nq)


def _fwd_outputs(b, vd, nq):
    return (torch.empty((b, vd, nq), dtype=torch.float16, device="cuda:0"),
            torch.empty((b, nq), dtype=torch.float32, device="cuda:0"),
            torch.empty((b, nq), dtype=torch.float16, device="cuda:0"))


def _oracle_forward(monkeypatch, got, policy, mode, Q, K, V):
    """run_case's forward checks of ``got`` = (O, l, m) of a [b, ...] call, handed in through its _call hook."""
    b, d, nq = Q.shape
    monkeypatch.setattr(parity, "_call", lambda *a: got)
    parity.run_case(np.float16, policy, 1, mode, (b,), d, V.shape[1], (nq,), (K.shape[2],), bwd=False,
                    inputs=(Q, K, V, np.zeros((b, V.shape[1], nq), np.float16)))


# ------------------------------------------------------------------ fa_forward_ws
@pytest.mark.parametrize("policy,mode", [("full", "none_front"), ("causal", "scale_end")])
def test_forward_ws(monkeypatch, diag_lib, policy, mode):  # noqa: F811
    """5 queries against 2100 keys (under causal scale_end query i sits at key 420 i + 419, so the range is all
    2100 keys): 5 chunks of 512 keys, the last one short; 5 slices in slabs of 1, 2, 3 and (the control) 7."""
    b, nq, nk, d = 5, 5, 2100, 64
    caps = (1, 2, 3, 7)
    _check_caps(caps, b, control=(7,))
    prob = _problem(policy, mode, nq, nk, d, d, b)
    chunks, chunk, kb, ke = _plan4(diag_lib.fa_forward_split_plan, prob)
    assert chunks >= 2 and (ke - kb) >= 2048 and (ke - kb) % chunk != 0
    Q, K, V, _ = _np_qkv(b, b, d, d, nq, nk, seed=11)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    need = int(diag_lib.fa_forward_workspace_bytes(prob))
    assert need > 0

    def call():
        out, ws = _fwd_outputs(b, d, nq), Workspace(need)
        st = diag_lib.fa_forward_ws(_stream(), prob, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(),
                                    *(t.data_ptr() for t in out), ws.ptr(), need)
        assert st == _lib.FA_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert ws.intact()
        return out

    ref = _run(monkeypatch, diag_lib, None, b, call)
    _oracle_forward(monkeypatch, ref, policy, mode, Q, K, V)
    for cap in caps:
        assert _same(_run(monkeypatch, diag_lib, cap, b, call), ref), cap


# ------------------------------------------------------------------ fa_forward_grouped
def test_forward_grouped(monkeypatch, diag_lib):  # noqa: F811
    """g = 4 query slices of 3 queries per K/V slice, 203 keys, 5 K/V slices: the slab advances Q, O, l and m by
    g slices and K, V by one."""
    g, nq, nk, d, bkv = 4, 3, 203, 64, 5
    caps = (1, 2, 3)
    _check_caps(caps, bkv)
    b = bkv * g
    prob = _problem("full", "none_front", nq, nk, d, d, b)
    plan = (ctypes.c_int32 * 6)()
    assert diag_lib.fa_forward_grouped_plan(prob, g, plan) == _lib.FA_OK and plan[0] >= 1
    Q, K, V, _ = _np_qkv(b, bkv, d, d, nq, nk, seed=12)
    tq, tk, tv = _dev(Q), _dev(K), _dev(V)
    need = int(diag_lib.fa_forward_grouped_workspace_bytes(prob, g))
    assert need > 0

    def call():
        out, ws = _fwd_outputs(b, d, nq), Workspace(need)
        st = diag_lib.fa_forward_grouped(_stream(), prob, g, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(),
                                         *(t.data_ptr() for t in out), ws.ptr(), need)
        assert st == _lib.FA_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert ws.intact()
        return out

    ref = _run(monkeypatch, diag_lib, None, bkv, call)
    _oracle_forward(monkeypatch, ref, "full", "none_front", Q, np.repeat(K, g, axis=0), np.repeat(V, g, axis=0))
    for cap in caps:
        assert _same(_run(monkeypatch, diag_lib, cap, bkv, call), ref), cap


# ------------------------------------------------------------------ ragged_1d and paged_1d, fp16 and FP8 caches
SEQS, HK, G = 3, 3, 2                   # kv_per_len = 3, 9 K/V slices, 18 query slices
PAGE, MAX_PAGES = 64, 4                 # capacity 256
LENS = (77, 0, PAGE * MAX_PAGES)        # inside the second tile, empty, the capacity
K_SCALE, V_SCALE = (0.5, 1.0, 3.0), (2.0, 0.25, 1.5)
DECODE_CAPS = (1, 2, 4, 5, 7)           # slabs start at (len0, rem0) = (0, 2), (1, 1), (1, 2), (2, 1), ...
DECODE_SHAPES = [(64, 64, 1, False), (64, 64, 1, True), (64, 64, 4, False), (64, 64, 4, True), (128, 128, 4, True),
                 (96, 40, 4, False)]    # (the last one: element-wise staging, of the FP8 cache too)


def _pairwise_distinct(rows):
    rows = [tuple(np.asarray(r).reshape(-1).tolist()) for r in rows]
    return len(set(rows)) == len(rows)


def _scatter(cache, table, num_pages, fill):
    """The padded cache [SEQS * HK, c, cap] as a pool [num_pages, HK, c, PAGE] through ``table``."""
    c = cache.shape[1]
    pool = np.full((num_pages, HK, c, PAGE), fill, cache.dtype)
    pool[table] = cache.reshape(SEQS, HK, c, MAX_PAGES, PAGE).transpose(0, 3, 1, 2, 4)
    return pool


def _decode_case(form, fp8, d, vd, nq, seed):
    """The wrapper's arguments (device tensors) and what the float64 reference needs (Q, K, V as the kernel
    is to see them, one length per K/V slice)."""
    cap = PAGE * MAX_PAGES
    Q, K, V, _ = _np_qkv(SEQS * HK * G, SEQS * HK, d, vd, nq, cap, seed)
    num_pages = SEQS * MAX_PAGES + 3
    table = np.random.default_rng(seed + 1).permutation(num_pages)[:SEQS * MAX_PAGES].reshape(SEQS, MAX_PAGES)
    table = table.astype(np.int32)
    assert _pairwise_distinct(LENS) and set(LENS) >= {0, cap} and any(0 < x % 64 and x < cap for x in LENS)
    assert _pairwise_distinct(K_SCALE) and _pairwise_distinct(V_SCALE)
    assert _pairwise_distinct(table) and len(set(table.reshape(-1).tolist())) == table.size   # no shared page
    byhead = lambda x: x.reshape(SEQS, HK, x.shape[1], cap)  # noqa: E731
    scales = {}
    if fp8:
        K8 = fp8_ref.quantize(byhead(K), K_SCALE, 1).reshape(K.shape)
        V8 = fp8_ref.quantize(byhead(V), V_SCALE, 1).reshape(V.shape)
        Kref = fp8_ref.dequantize(byhead(K8), K_SCALE, 1).reshape(K.shape)
        Vref = fp8_ref.dequantize(byhead(V8), V_SCALE, 1).reshape(V.shape)
        Kin, Vin, fill = K8, V8, 0x7F
        scales = dict(k_scale=_dev(np.asarray(K_SCALE, np.float32)), v_scale=_dev(np.asarray(V_SCALE, np.float32)))
    else:
        Kin, Vin, Kref, Vref, fill = K, V, K, V, np.nan
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda:0")
    tq = _dev(Q.reshape(SEQS, HK * G, d, nq))
    if form == "ragged":
        args = (tq, _dev(byhead(Kin)), _dev(byhead(Vin)), lens)
    else:
        Kp, Vp = _scatter(Kin, table, num_pages, fill), _scatter(Vin, table, num_pages, fill)
        args = (tq, _dev(Kp), _dev(Vp), _dev(table), lens)
        gathered = paged_ref.gather(Kp, table, PAGE), paged_ref.gather(Vp, table, PAGE)
        assert gathered[0].tobytes() == Kin.tobytes() and gathered[1].tobytes() == Vin.tobytes()
    return args, scales, (Q, Kref, Vref, np.repeat(LENS, HK))


@pytest.mark.parametrize("d,vd,nq,tail", DECODE_SHAPES)
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_decode_wrappers(monkeypatch, diag_lib, form, fp8, d, vd, nq, tail):  # noqa: F811
    """3 sequences of 3 K/V heads, g = 2, capacity 256 in pages of 64, through ragged_1d / paged_1d: every cap but
    1 makes a slab straddle two sequences, so len0 and rem0 pick the length, the table row and the head's scales."""
    bkv = SEQS * HK
    _check_caps(DECODE_CAPS, bkv)
    args, scales, (Q, Kref, Vref, kv_lens) = _decode_case(form, fp8, d, vd, nq, seed=1000 * d + 10 * nq + tail)
    wrapper = fa.ragged_1d if form == "ragged" else fa.paged_1d

    def call():
        with torch.no_grad():
            out = wrapper(*args, tail_causal=tail, returning_l_m=True, **scales)
        return tuple(t.reshape((-1,) + t.shape[2:]) for t in out)

    ref = _run(monkeypatch, diag_lib, None, bkv, call)
    res = rg._check_ref(ref, Q, Kref, Vref, kv_lens, G, tail)
    print(f"{form} fp8={fp8} d={d} vd={vd} nq={nq} tail={tail}: worst error / allowance {res}")
    for cap in DECODE_CAPS:
        assert _same(_run(monkeypatch, diag_lib, cap, bkv, call), ref), cap


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_decode_workspace_guard(monkeypatch, diag_lib, form, fp8):  # noqa: F811
    """The wrappers allocate their own workspace; here the entry points get one with a guard behind the reported
    size, and must give the wrapper's bits."""
    d, nq, tail, bkv = 64, 4, True, SEQS * HK
    b = bkv * G
    args, scales, _ = _decode_case(form, fp8, d, d, nq, seed=77)
    with torch.no_grad():
        monkeypatch.delenv("FA_SLAB_MAX", raising=False)
        ref = (fa.ragged_1d if form == "ragged" else fa.paged_1d)(*args, tail_causal=tail, returning_l_m=True, **scales)
    ref = tuple(t.reshape((-1,) + t.shape[2:]) for t in ref)
    prob = _problem("full", "none_front", nq, PAGE * MAX_PAGES, d, d, b)
    sc = [scales[k].data_ptr() for k in ("k_scale", "v_scale")] if fp8 else []
    if form == "ragged":
        need = int(diag_lib.fa_forward_ragged_workspace_bytes(prob, G))
        fn = diag_lib.fa_forward_ragged_fp8 if fp8 else diag_lib.fa_forward_ragged
        mid = sc + [args[3].data_ptr(), HK, int(tail)]
    else:
        need = int(diag_lib.fa_forward_paged_workspace_bytes(prob, G, PAGE))
        fn = diag_lib.fa_forward_paged_fp8 if fp8 else diag_lib.fa_forward_paged
        mid = sc + [args[3].data_ptr(), MAX_PAGES, PAGE, int(args[1].shape[0]), args[4].data_ptr(), HK, int(tail)]
    assert need > 0

    def call():
        out, ws = _fwd_outputs(b, d, nq), Workspace(need)
        st = fn(_stream(), prob, G, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), *mid,
                *(t.data_ptr() for t in out), ws.ptr(), need)
        assert st == _lib.FA_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert ws.intact()
        return out

    for cap in (None, 2, 4, 7):
        assert _same(_run(monkeypatch, diag_lib, cap, bkv, call), ref), cap


# ------------------------------------------------------------------ fa_backward_split, both forms
class _Replay(torch.autograd.Function):
    """O with the given gradients: hands an entry point's results to run_case, which calls .backward()."""

    @staticmethod
    def forward(ctx, q, k, v, o, dq, dk, dv):
        ctx.save_for_backward(dq, dk, dv)
        return o.clone()

    @staticmethod
    def backward(ctx, d_o):
        return (*ctx.saved_tensors, None, None, None, None)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("form,nq,nk", [("key_split", 5, 2100), ("query_split", 2100, 77)])
def test_backward_split(monkeypatch, diag_lib, form, nq, nk, d):  # noqa: F811
    """key_split: 5 queries against 2100 keys, the dQ pass in 5 key chunks with partials in the workspace;
    query_split: 2100 queries against 77 keys, the dK/dV pass in 3 query chunks.  dQ, dK and dV of 5 slices in
    slabs of 1, 2 and 3."""
    b, caps = 5, (1, 2, 3)
    _check_caps(caps, b)
    prob = _problem("full", "none_front", nq, nk, d, d, b)
    kplan = _plan4(diag_lib.fa_backward_split_plan, prob)
    qplan = _plan4(diag_lib.fa_backward_split_q_plan, prob)
    assert (kplan[0] >= 2 and qplan[0] == 0) if form == "key_split" else (qplan[0] >= 2 and kplan[0] == 0)
    Q, K, V, dO = _np_qkv(b, b, d, d, nq, nk, seed=13 + d)
    tq, tk, tv, tdo = _dev(Q), _dev(K), _dev(V), _dev(dO)
    monkeypatch.delenv("FA_SLAB_MAX", raising=False)
    o, l, m = fa.attention_forward("full", 1, tq, tk, tv, "none_front")
    need = int(diag_lib.fa_backward_split_workspace_bytes(prob))
    assert need > int(diag_lib.fa_backward_workspace_bytes(prob))

    def call():
        grads, ws = (torch.empty_like(tq), torch.empty_like(tk), torch.empty_like(tv)), Workspace(need)
        st = diag_lib.fa_backward_split(_stream(), prob, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), o.data_ptr(),
                                        l.data_ptr(), m.data_ptr(), tdo.data_ptr(), *(t.data_ptr() for t in grads),
                                        ws.ptr(), need)
        assert st == _lib.FA_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert ws.intact()
        return grads

    ref = _run(monkeypatch, diag_lib, None, b, call)
    monkeypatch.setattr(parity, "_call", lambda pol, sd, q, k, v, *a: (_Replay.apply(q, k, v, o, *ref), l, m))
    parity.run_case(np.float16, "full", 1, "none_front", (b,), d, d, (nq,), (nk,), inputs=(Q, K, V, dO))
    for cap in caps:
        assert _same(_run(monkeypatch, diag_lib, cap, b, call), ref), cap


# ------------------------------------------------------------------ fa_merge_partials and fa_accumulate_parts
@pytest.mark.parametrize("nq", [7, 8], ids=["scalar", "vector"])
@pytest.mark.parametrize("dtype", mg.DTYPES, ids=mg._id)
def test_merge_partials(monkeypatch, diag_lib, dtype, nq):  # noqa: F811
    b, caps = 5, (1, 2, 3)
    _check_caps(caps, b)
    Os, ls, ms = mg.synthetic_partials(dtype, 3, b, 9, nq, seed=14 + nq)
    ref = _run(monkeypatch, diag_lib, None, b, lambda: mg.call_merge(dtype, Os, ls, ms))
    mg.check_merge(dtype, Os, ls, ms, ref, f"slabs nq={nq}")
    for cap in caps:
        got = _run(monkeypatch, diag_lib, cap, b, lambda: mg.call_merge(dtype, Os, ls, ms))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, ref)), cap


@pytest.mark.parametrize("dtype", mg.DTYPES, ids=mg._id)
def test_accumulate_parts(monkeypatch, diag_lib, dtype):  # noqa: F811
    """5 * 2048 + 3 elements in slabs of 2048 (five and a tail of 3 elements) and of 4096 (two and a tail of 2051);
    the bound is test_gpu_merge.test_accumulate_parts's."""
    count, n, caps = 5 * 2048 + 3, 3, (1, 2)
    units = -(-count // 2048)
    assert all(units >= 2 * c and count % (2048 * c) for c in caps)   # several slabs, the last one short
    rng = np.random.default_rng(15)
    parts = [rng.uniform(-2, 2, count).astype(dtype) for _ in range(n)]
    dparts = [_dev(x) for x in parts]

    def call():
        out = torch.empty_like(dparts[0])
        st = diag_lib.fa_accumulate_parts(_stream(), mg.DT_ID[dtype], count, n,
                                          _lib.pointer_array([t.data_ptr() for t in dparts]), out.data_ptr())
        assert st == _lib.FA_OK, _lib.last_error()
        torch.cuda.synchronize()
        return (out,)

    ref = _run(monkeypatch, diag_lib, None, units, call)
    u_t, u_acc = U_ROUND[dtype]
    exact = np.sum([x.astype(np.float64) for x in parts], axis=0)
    mag = np.sum([np.abs(x.astype(np.float64)) for x in parts], axis=0)
    err = np.abs(ref[0].cpu().numpy().astype(np.float64) - exact)
    tiny = float(np.finfo(dtype).smallest_subnormal) / 2
    assert (err <= u_t * np.abs(exact) + tiny + (1 + u_t) * (n - 1) * u_acc * mag).all()
    for cap in caps:
        assert _same(_run(monkeypatch, diag_lib, cap, units, call), ref), cap
