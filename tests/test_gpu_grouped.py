"""GPU tests of grouped-query attention (csrc/fa_fwd_f16_gqa.hip, flash_attention.grouped_1d / grouped_2d;
DESIGN.md §3.8): g query heads share one K/V head, and inside the fused envelope the g heads are folded into
the 128 query rows of one workgroup.

Reference: oracle.forward_f64 on K / V repeated per group with np.repeat.  Every forward case goes through
tests.test_gpu_parity.run_case (its fp16 forward tolerances and its l / m checks, rows that attend nothing
exactly O = 0, l = 0, m = bytes 0xFA): run_case is handed the expanded K / V as its inputs and reaches the
grouped wrapper, with the grouped K / V, through its module-level _call hook.  The gradient cases compare
grouped_1d's dQ, dK, dV with oracle.backward_f64 on the expanded problem, dK / dV summed over each group in
float64, under gate.grad_ok with the root-sum-square of the members' rounding scales.  The remaining tests call
the C ABI directly: workspace check, determinism, independence of the batch, kv_group = 1."""

import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from oracle import fa_oracle as O
from tests import gate
from tests import score_ramp as R
from tests import test_gpu_parity as parity
from tests.gate import U_ROUND
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}
DT = {np.float16: _lib.F16, np.float32: _lib.F32, np.float64: _lib.F64}


def _problem(policy, mode, qs, ks, d, vd, b, ws=1, ls=0, causal=False, dtype=_lib.F16):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], b, qs, ks, d, vd, ws, ls, causal)


def _plan(policy, mode, qs, ks, d, vd, g, ws=1, ls=0, causal=False, dtype=_lib.F16):
    out = (ctypes.c_int32 * 6)()
    p = _problem(policy, mode, qs, ks, d, vd, g, ws, ls, causal, dtype)
    assert _lib.lib().fa_forward_grouped_plan(p, g, out) == 0
    return tuple(out)


def _uniform(rng, dtype, *shape):
    return rng.uniform(-2, 2, shape).astype(dtype)


def _grouped_case(monkeypatch, policy, mode, g, qs, ks, d, vd, bkv=2, ws=1, ls=0, causal=False, seed=0, dtype=np.float16,
                  fused=True, misalign=False, inputs=None, m_bound=None):
    """Forward parity of the grouped wrapper for Q [bkv * g, d, *qs] against K / V [bkv, ., *ks]."""
    qs, ks = tuple(qs), tuple(ks)
    chunks = _plan(policy, mode, qs, ks, d, vd, g, ws, ls, causal, DT[dtype])[0]
    assert (chunks > 0) == fused, chunks
    rng = np.random.default_rng(seed)
    if inputs is None:
        Q, dO = _uniform(rng, dtype, bkv * g, d, *qs), _uniform(rng, dtype, bkv * g, vd, *qs)
        K, V = _uniform(rng, dtype, bkv, d, *ks), _uniform(rng, dtype, bkv, vd, *ks)
    else:
        Q, K, V, dO = inputs
    dev = torch.device("cuda:0")
    tk, tv = (parity._to_dev(x, dev, False, misalign) for x in (K, V))
    f = fa.grouped_1d if len(qs) == 1 else fa.grouped_2d

    def call(policy_, seq_dims, tq, tk_expanded, tv_expanded, mode_, ws_, ls_, causal_):
        assert tuple(tk_expanded.shape) == (bkv * g, d) + ks  # (run_case's reference inputs; not used here)
        return f(tq, tk, tv, policy_, mode_, ws_, ls_, causal_, returning_l_m=True)

    monkeypatch.setattr(parity, "_call", call)
    return parity.run_case(dtype, policy, len(qs), mode, (bkv * g,), d, vd, qs, ks, ws=ws, ls=ls, causal=causal, bwd=False,
                           inputs=(Q, np.repeat(K, g, axis=0), np.repeat(V, g, axis=0), dO), misalign=misalign,
                           m_bound=m_bound)


# ------------------------------------------------------------------ the fused path against the oracle
@pytest.mark.parametrize("g,nq", [(2, 1), (8, 1), (128, 1), (3, 3), (5, 5), (8, 16), (4, 32), (2, 33), (2, 64)])
def test_pitch_and_wave_classes(monkeypatch, g, nq):
    """Full rule, d = v_d = 64, nk = 2601: several chunks with a ragged last tile, element-wise staging."""
    chunks, chunk, kb, ke, pitch, rows = _plan("full", "none_front", (nq,), (2601,), 64, 64, g)
    assert chunks >= 3 and (kb, ke) == (0, 2601) and 2601 % chunk % 64 != 0
    _grouped_case(monkeypatch, "full", "none_front", g, (nq,), (2601,), 64, 64, seed=100 * g + nq)


@pytest.mark.parametrize("d,vd", [(8, 8), (64, 64), (96, 40), (33, 100), (128, 128)])
def test_channel_instances(monkeypatch, d, vd):
    """D = 32 / 64 / 128 with both stagings (nk % 8 == 0: the 16-byte one where d == v_d == D)."""
    _grouped_case(monkeypatch, "full", "none_front", 4, (8,), (2600,), d, vd, seed=d + vd)


@pytest.mark.parametrize("nk", [1, 70, 640])
def test_key_lengths(monkeypatch, nk):
    """One key; one tile and a tail in a second; whole tiles only (a 512-key chunk and one of two tiles: at 32
    folded rows min_chunk is 512).  The plan has no minimum range."""
    chunks, chunk = _plan("full", "none_front", (4,), (nk,), 128, 128, 8)[:2]
    assert (chunks, chunk) == ((1, 512) if nk < 640 else (2, 512))
    _grouped_case(monkeypatch, "full", "none_front", 8, (4,), (nk,), 128, 128, seed=nk)


@pytest.mark.parametrize("policy,mode,nq,nk,ws,causal", [
    ("causal", "scale_end", 1, 4200, 1, False),
    ("causal", "scale_end", 4, 4096, 1, False),
    ("causal", "none_front", 16, 2600, 1, False),     # the keys past the first 16 are masked for every row
    ("local", "scale_front", 8, 8192, 3000, False),
    ("local", "scale_front", 8, 8192, 3000, True),
])
def test_interval_rules(monkeypatch, policy, mode, nq, nk, ws, causal):
    _grouped_case(monkeypatch, policy, mode, 4, (nq,), (nk,), 128, 128, ws=ws, causal=causal, seed=nq + nk)


@pytest.mark.parametrize("policy,ws,ls,causal", [("local", 20, 1, False), ("local", 20, 1, True), ("causal", 1, 0, False)])
def test_2d_rules(monkeypatch, policy, ws, ls, causal):
    """Window 20 at stride 2 under scale_end (the per-element rule check, POL 2), and the 2d causal rule."""
    _grouped_case(monkeypatch, policy, "scale_end", 2, (2, 4), (40, 66), 64, 64, ws=ws, ls=ls, causal=causal, seed=17)


@pytest.mark.parametrize("qs,fused", [((64, 2), False), ((64, 1), True)])
def test_rows_without_any_key(monkeypatch, qs, fused):
    """The shape of test_gpu_splitk.test_rows_without_any_key with g = 2: the query rows past key row 42 attend
    nothing (run_case checks O = 0, l = 0, m = bytes 0xFA for them).  Its 128 queries put g * pitch at 256, past
    the fused envelope, so that shape runs on expanded K / V; with one query column the same rows are empty and
    the group folds into 2 x 64 rows, a pitch at which a wave holds a run of one head's queries."""
    mask = O.rule_mask(qs, (33, 80), "scale_front", "local", 10, 0, False)
    empty = ~np.asarray(mask).reshape(qs[0] * qs[1], -1).any(axis=1)
    assert 0 < empty.sum() < empty.size
    _grouped_case(monkeypatch, "local", "scale_front", 2, qs, (33, 80), 64, 64, ws=10, seed=19, fused=fused)


def test_misaligned_pointers(monkeypatch):
    _grouped_case(monkeypatch, "full", "none_front", 4, (8,), (2600,), 64, 64, seed=23, misalign=True)


# ------------------------------------------------------------------ the lazy rebase inside a folded wave
def test_rebase_in_some_heads_of_a_wave(monkeypatch):
    """Staircase scores (tests/score_ramp.py) at pitch 8, g = 8: a wave holds four heads.  K carries one
    staircase per K/V slice; every head has its own seed, step height q0 and lift, and the odd heads have
    q0 = 0: their scores are flat, so within each wave the even heads' climb rows pass kRescaleThr tile after
    tile while their neighbours never do (checked with the rebase model per key chunk).  Then the gate of
    test_gpu_score_range.py: run_case with m's dot-product term replaced by score_ramp.m_rounding_bound."""
    g, nq, nk, d, bkv = 8, 8, 776, 64, 2
    prob = O.Problem("full", 1, "none_front")
    base = R._ramp(d, 64, np.float16)
    (_, K, V, _), _ = R.ramp_inputs(prob, np.float16, (bkv,), d, d, (nq,), (nk,), base, seed=7)
    heads = [dataclasses.replace(base, q0=(0.0 if j % 2 else (2.0, 1.875)[(j // 2) % 2]), lift=24.0 - j) for j in range(g)]
    Q = np.empty((bkv, g, d, nq), np.float16)
    dO = np.empty((bkv, g, d, nq), np.float16)
    bound = np.empty((bkv, g, nq))
    for j, ramp in enumerate(heads):
        (Qj, Kj, _, dOj), info = R.ramp_inputs(prob, np.float16, (bkv,), d, d, (nq,), (nk,), ramp, seed=100 + j)
        Q[:, j], dO[:, j] = Qj, dOj
        # the special channels of K do not depend on the seed, q0 or the lift: head j's Q pairs with the shared K
        assert np.array_equal(Kj[:, :R.N_SPECIAL], K[:, :R.N_SPECIAL])
        if ramp.q0 == 0.0:  # a flat head: the row max may sit on any key
            info = dict(info, on_top=info["mask"])
        bound[:, j] = R.m_rounding_bound(Qj, K, info, np.float16, d)
    chunks, chunk = _plan("full", "none_front", (nq,), (nk,), d, d, g)[:2]
    assert chunks == 2 and g * 8 == 64
    for s in range(bkv):
        fired = np.zeros((g, chunks), bool)
        for j in range(g):
            scores = R.kernel_scores(Q[s, j][None], K[s][None], d, True)
            for c in range(chunks):  # every chunk seeds afresh, tiles from its first key
                k0, k1 = c * chunk, min((c + 1) * chunk, nk)
                fired[j, c] = R.rebase_tiles(scores[:, k0:k1], info["mask"][:, k0:k1], 64, 8.0)[0].any()
        for wave in (slice(0, 4), slice(4, 8)):
            assert (fired[wave].any(axis=0) & ~fired[wave].all(axis=0)).all(), fired
        assert fired[0::2].all() and not fired[1::2].any()
    flat = lambda x: x.reshape((bkv * g,) + x.shape[2:])  # noqa: E731
    _grouped_case(monkeypatch, "full", "none_front", g, (nq,), (nk,), d, d, bkv=bkv, inputs=(flat(Q), K, V, flat(dO)),
                  m_bound=flat(bound))


# ------------------------------------------------------------------ the expansion outside the envelope
@pytest.mark.parametrize("dtype,g,qs,ks,d,policy,ws", [
    (np.float32, 4, (8,), (300,), 64, "full", 1),
    (np.float64, 4, (8,), (300,), 64, "causal", 1),
    (np.float16, 2, (8,), (300,), 256, "full", 1),
    (np.float16, 2, (200,), (300,), 64, "causal", 1),
    (np.float16, 2, (16, 16), (16, 16), 64, "local", 5),
], ids=["fp32", "fp64", "d256", "nq200", "2d-local"])
def test_outside_the_envelope_k_and_v_are_expanded(monkeypatch, dtype, g, qs, ks, d, policy, ws):
    _grouped_case(monkeypatch, policy, "scale_end", g, qs, ks, d, d, ws=ws, dtype=dtype, fused=False, seed=d + len(qs))


def test_wrapper_accepts_leading_batch_axes_and_one_group_is_the_ungrouped_wrapper():
    rng = np.random.default_rng(3)
    dev = torch.device("cuda:0")
    Q, K, V = (torch.from_numpy(_uniform(rng, np.float16, *s)).to(dev)
               for s in ((3, 8, 64, 8), (3, 2, 64, 2600), (3, 2, 64, 2600)))
    got = fa.grouped_1d(Q, K, V, returning_l_m=True)
    # [3, 8] heads over [3, 2]: flattened, Q slice bi attends K/V slice bi // 4
    ref = fa.grouped_1d(Q.reshape(24, 64, 8), K.reshape(6, 64, 2600), V.reshape(6, 64, 2600), returning_l_m=True)
    assert all(a.shape[:2] == (3, 8) for a in got)
    assert _same([a.reshape(b.shape) for a, b in zip(got, ref)], ref)
    one = fa.grouped_1d(Q[:, :2].contiguous(), K, V, "causal", "scale_end", returning_l_m=True)
    assert _same(one, fa.causal_1d(Q[:, :2].contiguous(), K, V, "scale_end", returning_l_m=True))


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize("dtype,policy,mode,g,nq,nk,d,fused", [
    (np.float16, "full", "none_front", 4, 8, 2600, 64, True),
    (np.float16, "causal", "scale_end", 4, 4, 4096, 128, True),
    (np.float16, "causal", "scale_end", 2, 200, 300, 64, False),
    (np.float32, "full", "none_front", 4, 8, 300, 32, False),
    (np.float64, "local", "scale_front", 3, 8, 300, 32, False),
], ids=["fused-full", "fused-causal", "expanded-nq200", "expanded-fp32", "expanded-fp64"])
def test_gradients(dtype, policy, mode, g, nq, nk, d, fused):
    """dQ per head; dK and dV summed over the group (the reference in float64, the wrapper in fp32 / fp64 with
    one rounding).  The rounding scale of a sum is the root-sum-square of its members' scales."""
    bkv, ws = 2, (100 if policy == "local" else 1)
    assert (_plan(policy, mode, (nq,), (nk,), d, d, g, ws, 0, False, DT[dtype])[0] > 0) == fused
    rng = np.random.default_rng(nq + nk + d)
    Q, dO = _uniform(rng, dtype, bkv * g, d, nq), _uniform(rng, dtype, bkv * g, d, nq)
    K, V = _uniform(rng, dtype, bkv, d, nk), _uniform(rng, dtype, bkv, d, nk)
    dev = torch.device("cuda:0")
    tq, tk, tv = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (Q, K, V))
    o = fa.grouped_1d(tq, tk, tv, policy, mode, ws, 0, False)
    o.backward(torch.from_numpy(dO).to(dev))
    torch.cuda.synchronize()
    assert tk.grad.shape == tk.shape and tv.grad.shape == tv.shape and tk.grad.dtype == tk.dtype
    prob = O.Problem(policy, 1, mode, ws, 0, False)
    Ke, Ve = np.repeat(K, g, axis=0), np.repeat(V, g, axis=0)
    dQ, dKe, dVe = O.backward_f64(Q, Ke, Ve, dO, prob)
    eQ, eKe, eVe = O.backward_rounding_scale_f64(Q, Ke, Ve, dO, prob, *U_ROUND[dtype])
    fold = lambda x: x.reshape((bkv, g) + x.shape[1:]).sum(axis=1)  # noqa: E731
    rss = lambda e: np.sqrt((e.reshape((bkv, g) + e.shape[1:]) ** 2).sum(axis=1))  # noqa: E731
    for name, got, ref, e in (("dQ", tq.grad, dQ, eQ), ("dK", tk.grad, fold(dKe), rss(eKe)),
                              ("dV", tv.grad, fold(dVe), rss(eVe))):
        got = got.cpu().numpy().astype(np.float64)
        worst = float((np.abs(got - ref) / gate.grad_bound(ref, e, dtype)).max())
        print(f"{name}: max err / bound {worst:.3f}, slope {gate.scale_slope(got, ref):.3e}")
        assert gate.grad_ok(got, ref, e, dtype, d, got.shape[1]), f"{name}: max err / bound {worst:.3f}"


# ------------------------------------------------------------------ the C ABI directly
def _inputs(bkv, g, d, vd, nq, nk, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=gen) * 4 - 2).half().cuda()  # noqa: E731
    return mk(bkv * g, d, nq), mk(bkv, d, nk), mk(bkv, vd, nk)


def _abi_grouped(prob, g, Q, K, V, ws_short=0, fill=None):
    """fa_forward_grouped on device tensors; returns (status, O, l, m)."""
    L = _lib.lib()
    b, nq, vd = Q.shape[0], Q.shape[2], V.shape[1]
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O_, l, m):
            t.view(torch.uint8).fill_(fill)
    need = int(L.fa_forward_grouped_workspace_bytes(prob, g))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    st = L.fa_forward_grouped(torch.cuda.current_stream().cuda_stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                              O_.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0))
    torch.cuda.synchronize()
    return st, O_, l, m


def _same(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_short_workspace_is_rejected_and_nothing_is_written():
    prob = _problem("full", "none_front", (8,), (2600,), 64, 64, b=8)
    Q, K, V = _inputs(2, 4, 64, 64, 8, 2600, 2)
    st, O_, l, m = _abi_grouped(prob, 4, Q, K, V, ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in (O_, l, m):
        assert bool((t.view(torch.uint8) == 0x5A).all())


def test_two_calls_are_bitwise_equal():
    prob = _problem("causal", "scale_front", (5,), (4101,), 96, 40, b=3 * 5)
    Q, K, V = _inputs(3, 5, 96, 40, 5, 4101, 4)
    st0, *a = _abi_grouped(prob, 5, Q, K, V)
    st1, *b = _abi_grouped(prob, 5, Q, K, V)
    assert st0 == 0 and st1 == 0
    assert _same(a, b)


@pytest.mark.parametrize("policy,mode,g,nq,nk,d", [("full", "none_front", 4, 8, 2600, 64),
                                                   ("causal", "scale_end", 2, 64, 4200, 128)])
def test_group_is_bitwise_independent_of_the_batch(policy, mode, g, nq, nk, d):
    Q, K, V = _inputs(3, g, d, d, nq, nk, 3)
    run = lambda q, k, v: _abi_grouped(_problem(policy, mode, (nq,), (nk,), d, d, b=q.shape[0]), g, q, k, v)  # noqa: E731
    st3, *all3 = run(Q, K, V)
    st1, *alone = run(Q[g:2 * g].contiguous(), K[1:2].contiguous(), V[1:2].contiguous())
    assert st3 == 0 and st1 == 0
    assert _same([t[g:2 * g] for t in all3], alone)


@pytest.mark.parametrize("nk", [300, 2600])
def test_group_of_one_is_fa_forward_ws(nk):
    """Outside and inside the split-key envelope of the ungrouped forward."""
    L = _lib.lib()
    prob = _problem("causal", "scale_end", (33,), (nk,), 64, 64, b=2)
    assert (L.fa_forward_workspace_bytes(prob) > 0) == (nk == 2600)
    Q, K, V = _inputs(2, 1, 64, 64, 33, nk, 1)
    st0, *got = _abi_grouped(prob, 1, Q, K, V)
    need = int(L.fa_forward_workspace_bytes(prob))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    ref = [torch.empty_like(t) for t in got]
    st1 = L.fa_forward_ws(torch.cuda.current_stream().cuda_stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                          ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st0 == 0 and st1 == 0
    assert _same(got, ref)


def test_outside_the_envelope_the_abi_reports_unsupported_and_writes_nothing():
    prob = _problem("full", "none_front", (200,), (300,), 64, 64, b=4)
    Q, K, V = _inputs(2, 2, 64, 64, 200, 300, 6)
    st, O_, l, m = _abi_grouped(prob, 2, Q, K, V, fill=0x5A)
    assert st == _lib.FA_ERR_UNSUPPORTED
    for t in (O_, l, m):
        assert bool((t.view(torch.uint8) == 0x5A).all())


def test_python_wrapper_takes_the_fused_path():
    """grouped_1d's bits are fa_forward_grouped's, and K / V were not expanded on the way (the ungrouped forward
    on expanded K / V is a different computation: compared against the oracle above, not bitwise)."""
    g, nq, nk = 4, 8, 2600
    assert _plan("full", "none_front", (nq,), (nk,), 64, 64, g)[0] >= 3
    Q, K, V = _inputs(2, g, 64, 64, nq, nk, 5)
    st, *direct = _abi_grouped(_problem("full", "none_front", (nq,), (nk,), 64, 64, b=2 * g), g, Q, K, V)
    assert st == 0
    got = fa.grouped_1d(Q, K, V, returning_l_m=True)
    torch.cuda.synchronize()
    assert _same(direct, got)


@pytest.mark.parametrize("dtype,seq,policy,mode,g,batch,hk,qs,ks,d,vd,ws,fused", [
    (np.float16, 1, "full", "none_front", 4, (), 2, (8,), (700,), 64, 40, 1, True),
    (np.float16, 2, "local", "scale_end", 2, (), 2, (12, 11), (12, 11), 64, 64, 3, False),
    (np.float16, 1, "causal", "scale_end", 8, (), 1, (40,), (300,), 96, 96, 1, False),
    (np.float32, 1, "causal", "scale_front", 2, (2,), 3, (50,), (70,), 32, 24, 1, False),
], ids=["fused-d64-v40", "expanded-2d-local", "mqa-g8", "batch-2x3g"])
def test_gradients_more_shapes(dtype, seq, policy, mode, g, batch, hk, qs, ks, d, vd, ws, fused):
    """d != v_d inside the fused envelope, a 2d window, one K/V head under eight query heads, and Q [2, 3 g] over K / V
    [2, 3]: dQ, dK and dV against tests/union_ref.py's grouped reference (np.repeat, dK / dV folded in float64, the
    root-sum-square of the members' scales) under gate.grad_ok."""
    from tests import union_ref
    assert (_plan(policy, mode, qs, ks, d, vd, g, ws, 0, False, DT[dtype])[0] > 0) == fused
    rng = np.random.default_rng(d + vd + g)
    Q, dO = _uniform(rng, dtype, *batch, hk * g, d, *qs), _uniform(rng, dtype, *batch, hk * g, vd, *qs)
    K, V = _uniform(rng, dtype, *batch, hk, d, *ks), _uniform(rng, dtype, *batch, hk, vd, *ks)
    dev = torch.device("cuda:0")
    tq, tk, tv = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (Q, K, V))
    o = (fa.grouped_1d if seq == 1 else fa.grouped_2d)(tq, tk, tv, policy, mode, ws, 0, False)
    o.backward(torch.from_numpy(dO).to(dev))
    torch.cuda.synchronize()
    assert tq.grad.shape == tq.shape and tk.grad.shape == tk.shape and tv.grad.shape == tv.shape
    lead = len(batch) + 1
    flat = lambda x: x.reshape((int(np.prod(x.shape[:lead])), x.shape[lead], -1))  # noqa: E731
    prob = O.Problem(policy, seq, mode, ws, 0, False)
    ref = union_ref.grouped(flat(Q), flat(K), flat(V), flat(dO), O.problem_mask(prob, qs, ks), g, *U_ROUND[dtype])
    og = flat(o.detach().cpu().numpy()).astype(np.float64)
    rtol, atol = gate.TOL[dtype]["fwd"]
    assert (np.abs(og - ref["O"]) <= gate.plain_bound(ref["O"], rtol, atol)).all()
    for name, got, r, e in (("dQ", tq.grad, ref["dQ"], ref["eQ"]), ("dK", tk.grad, ref["dK"], ref["eK"]),
                            ("dV", tv.grad, ref["dV"], ref["eV"])):
        got = flat(got.cpu().numpy()).astype(np.float64)
        worst = float((np.abs(got - r) / gate.grad_bound(r, e, dtype)).max())
        print(f"{name}: max err / bound {worst:.3f}, slope {gate.scale_slope(got, r):.3e}")
        assert gate.grad_ok(got, r, e, dtype, d, got.shape[1]), f"{name}: max err / bound {worst:.3f}"


@pytest.mark.parametrize("nq,fused", [(8, True), (200, False)])
def test_non_contiguous_inputs(nq, fused):
    """Q, K and V as strided views holding the same values: forward and gradients are bit for bit the contiguous
    call's, on the fused path and on expanded K / V."""
    g, nk, d = 4, 300, 64
    assert (_plan("causal", "scale_end", (nq,), (nk,), d, d, g)[0] > 0) == fused
    rng = np.random.default_rng(nq)
    Q, dO, K, V = (_uniform(rng, np.float16, *s) for s in ((2 * g, d, nq), (2 * g, d, nq), (2, d, nk), (2, d, nk)))
    dev = torch.device("cuda:0")

    def strided(x):
        buf = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=torch.float16, device=dev)
        buf[..., ::2] = torch.from_numpy(x).to(dev)
        view = buf[..., ::2]
        assert not view.is_contiguous()
        return view

    outs = []
    for wrap in (lambda x: torch.from_numpy(x).to(dev), strided):
        tq, tk, tv = (wrap(x).requires_grad_(True) for x in (Q, K, V))
        res = fa.grouped_1d(tq, tk, tv, "causal", "scale_end", returning_l_m=True)
        res[0].backward(wrap(dO))
        torch.cuda.synchronize()
        outs.append([t.detach() for t in res] + [tq.grad, tk.grad, tv.grad])
    assert all(a.shape == b.shape for a, b in zip(*outs)) and _same(*outs)
