"""GPU tests of the split-query dK/dV pass of the fp16 backward (csrc/fa_bwd_f16_fast.hip: the SPLIT forms of
bwd_dkdv_kernel and bwd_dkdv_pc_kernel, and dkdv_split_reduce_kernel): many queries
against one key block (nk <= 128), one workgroup per (slice, query chunk) writing fp32 partials, summed in
chunk order.

Every parity case goes through tests.test_gpu_parity.run_case (float64 oracle, its existing gate, forward
and backward through the Python wrappers, which route to fa_backward_split) after asserting through
fa_backward_split_q_plan that the shape really splits into >= 3 chunks with a shorter last chunk.  The
remaining tests call the C ABI directly.

The twelve split instances, <D, POL, ALN> (D = 64: the one-wave kernel for max(d, v_d) <= 64, D = 128: the
producer / consumer kernel; POL 0 full, 1 interval rules, 2 the per-element check of strided / 2d windows;
ALN: 16-B aligned tensors, nq % 8 == nk % 8 == 0), and a case that reaches each:
  64 0 T  full 2600 x 128, 64/64            128 0 T  full 2600 x 128, 128/128
  64 0 F  full 2600 x 33, 64/64             128 0 F  full 2600 x 33, 96/40
  64 1 T  causal 4200 x 64, 64/64           128 1 T  causal 4200 x 64, 128/128
  64 1 F  causal 2603 x 33, 64/64           128 1 F  causal 2603 x 33, 128/128
  64 2 T  2d strided window, 64/48          128 2 T  2d strided window, 128/128
  64 2 F  the same, misaligned pointers     128 2 F  the same, misaligned pointers"""

import ctypes

import numpy as np
import pytest
import torch

from tests import gate
from tests.test_gpu_parity import run_case
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}


def _problem(policy, mode, qs, ks, d, vd, b=1, ws=1, ls=0, causal=False, dtype=_lib.F16):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], b, qs, ks, d, vd, ws, ls, causal)


def _plan(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False, which="q"):
    out = (ctypes.c_int32 * 4)()
    fn = _lib.lib().fa_backward_split_q_plan if which == "q" else _lib.lib().fa_backward_split_plan
    assert fn(_problem(policy, mode, qs, ks, d, vd, 1, ws, ls, causal), out) == 0
    return tuple(out)


def _assert_splits(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False):
    chunks, chunk, qb, qe = _plan(policy, mode, qs, ks, d, vd, ws, ls, causal)
    assert chunks >= 3, (chunks, chunk, qb, qe)
    assert (qe - qb // 32 * 32) % chunk != 0, "the last chunk should be a partial one"
    return chunks, chunk, qb, qe


def _split_case(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False, batch=(2,), seed=0, misalign=False):
    _assert_splits(policy, mode, qs, ks, d, vd, ws, ls, causal)
    return run_case(np.float16, policy, len(qs), mode, batch, d, vd, qs, ks, ws=ws, ls=ls, causal=causal, seed=seed,
                    misalign=misalign)


# ------------------------------------------------------------------ parity against the oracle
@pytest.mark.parametrize("d,vd", [(64, 64), (128, 128), (96, 40), (33, 100), (8, 8)])
@pytest.mark.parametrize("nk", [1, 33, 128])
def test_full_1d_keys_and_channels(nk, d, vd):
    """2600 queries: 6 chunks of 512 with a 40-query last chunk (two tiles, padded to the producer / consumer
    kernel's group of four), or 3 chunks of 1024 above 64 keys."""
    assert _plan("full", "none_front", (2600,), (nk,), d, vd)[:2] == ((6, 512) if nk <= 64 else (3, 1024))
    _split_case("full", "none_front", (2600,), (nk,), d, vd, seed=300 + nk + d)


def test_causal_1d_scale_front():
    """4101 x 33: nine chunks, the last holds 5 queries; the last key sees nothing in the first seven chunks,
    so whole chunks add exact zeros for some keys."""
    assert _assert_splits("causal", "scale_front", (4101,), (33,), 64, 64)[:2] == (9, 512)
    _split_case("causal", "scale_front", (4101,), (33,), 64, 64, seed=307)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("nk", [64, 128])
def test_causal_scale_end_range_starts_past_zero(nk, d):
    """The first key's first query is past 0 (64 at 64 keys, 31 at 128: there the first chunk starts at a tile
    base below the range)."""
    _, _, qb, _ = _assert_splits("causal", "scale_end", (4200,), (nk,), d, d)
    assert qb == (64 if nk == 64 else 31)
    _split_case("causal", "scale_end", (4200,), (nk,), d, d, seed=300 + d + nk)


@pytest.mark.parametrize("d", [64, 128])
def test_ragged_query_length(d):
    _split_case("causal", "scale_end", (2603,), (33,), d, d, seed=329)


def test_misaligned_pointers():
    _split_case("full", "none_front", (2600,), (33,), 64, 64, seed=323, misalign=True)


@pytest.mark.parametrize("causal,mode", [(False, "none_front"), (True, "scale_front")])
def test_local_1d_window_3000(causal, mode):
    """none_front: the queries past the window attend nothing and the range ends before nq."""
    _, _, _, qe = _assert_splits("local", mode, (4101,), (128,), 64, 64, ws=3000, causal=causal)
    if mode == "none_front":
        assert qe < 4101
    _split_case("local", mode, (4101,), (128,), 64, 64, ws=3000, causal=causal, seed=313)


@pytest.mark.parametrize("causal", [False, True])
def test_local_1d_window_40(causal):
    """Each key's pairs sit in one or two chunks; most (key wave, tile) classes are 'none'."""
    _split_case("local", "scale_end", (4101,), (128,), 64, 64, ws=40, causal=causal, seed=315)


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("d,vd", [(64, 48), (128, 128)])
def test_local_2d_strided(d, vd, misalign):
    """Window 20 at stride 2 under scale_end: the per-element rule check (POL 2) inside split chunks, with
    16-B chunk staging and (misaligned pointers) element-wise staging."""
    _split_case("local", "scale_end", (40, 66), (4, 8), d, vd, ws=20, ls=1, seed=317 + d, misalign=misalign)


def test_keys_without_any_query():
    """33 x 80 queries against 64 x 2 keys, window 10: the key rows past query row 42 or so are attended by
    no query in any chunk.  run_case checks every gradient against the oracle; the dK and dV columns of those
    keys must also be exactly zero (every chunk's partial is an untouched accumulator)."""
    from oracle import fa_oracle as O
    qs, ks = (33, 80), (64, 2)
    mask = O.problem_mask(O.Problem("local", 2, "scale_front", 10, 0, False), qs, ks)
    empty = ~np.asarray(mask).reshape(33 * 80, 128).any(axis=0)
    assert empty.sum() == 44
    _split_case("local", "scale_front", qs, ks, 64, 64, ws=10, seed=319)
    g = torch.Generator(device="cpu").manual_seed(319)
    mk = lambda *s: (torch.rand(s, generator=g) * 4 - 2).half().cuda()  # noqa: E731
    Q, K, V, dO = mk(2, 64, *qs), mk(2, 64, *ks), mk(2, 64, *ks), mk(2, 64, *qs)
    o, l, m = fa.attention_forward("local", 2, Q, K, V, "scale_front", 10, 0, False)
    _, dK, dV = fa.attention_backward("local", 2, Q, K, V, o, l, m, dO, "scale_front", 10, 0, False)
    torch.cuda.synchronize()
    for t in (dK, dV):
        x = t.reshape(2, 64, 128).cpu().numpy()
        assert (x[:, :, empty] == 0).all()
        assert (x[:, :, ~empty] != 0).any()


# ------------------------------------------------------------------ the C ABI directly
def _inputs(b, d, vd, nq, nk, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) * 4 - 2).half().cuda()  # noqa: E731
    return mk(b, d, nq), mk(b, d, nk), mk(b, vd, nk), mk(b, vd, nq)


def _forward(prob, Q, K, V):
    L = _lib.lib()
    b, nq, vd = Q.shape[0], Q.shape[2], V.shape[1]
    O = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    st = L.fa_forward(torch.cuda.current_stream().cuda_stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                      O.data_ptr(), l.data_ptr(), m.data_ptr())
    assert st == 0
    return O, l, m


def _abi_backward(prob, Q, K, V, O, l, m, dO, split, ws_short=0, fill=None):
    """fa_backward (split False) or fa_backward_split on device tensors; returns (status, dQ, dK, dV)."""
    L = _lib.lib()
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    if fill is not None:
        for t in (dQ, dK, dV):
            t.view(torch.uint8).fill_(fill)
    need = int(L.fa_backward_split_workspace_bytes(prob) if split else L.fa_backward_workspace_bytes(prob))
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
    fn = L.fa_backward_split if split else L.fa_backward
    st = fn(torch.cuda.current_stream().cuda_stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(),
            l.data_ptr(), m.data_ptr(), dO.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), ws.data_ptr(),
            need - ws_short)
    torch.cuda.synchronize()
    return st, dQ, dK, dV


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _run_both(policy, mode, nq, nk, d, vd, b, seed):
    prob = _problem(policy, mode, (nq,), (nk,), d, vd, b=b)
    Q, K, V, dO = _inputs(b, d, vd, nq, nk, seed)
    O, l, m = _forward(prob, Q, K, V)
    st0, *plain = _abi_backward(prob, Q, K, V, O, l, m, dO, split=False)
    st1, *split = _abi_backward(prob, Q, K, V, O, l, m, dO, split=True)
    assert st0 == 0 and st1 == 0
    return plain, split


@pytest.mark.parametrize("policy,mode,nq,nk,d,vd", [("full", "none_front", 2600, 33, 64, 64),
                                                    ("causal", "scale_end", 4200, 64, 128, 128),
                                                    ("causal", "scale_front", 4101, 33, 96, 40)])
def test_split_against_fa_backward_inside_the_envelope(policy, mode, nq, nk, d, vd):
    """dQ comes from the same prep and dQ kernels: bitwise equal.  dK and dV are the same sums in another
    order: fa_backward's and fa_backward_split's are each within one plain fp16 backward bound of the oracle
    on these inputs (the parity cases above), so they differ by at most two bounds."""
    _assert_splits(policy, mode, (nq,), (nk,), d, vd)
    plain, split = _run_both(policy, mode, nq, nk, d, vd, 2, 401)
    assert _same(plain[:1], split[:1])
    for name, p, s in (("dK", plain[1], split[1]), ("dV", plain[2], split[2])):
        ref, got = p.double().cpu().numpy(), s.double().cpu().numpy()
        bound = 2.0 * gate.plain_bound(ref, *gate.TOL[np.float16]["bwd"])
        err = np.abs(got - ref)
        print(f"max |{name}_split - {name}_plain| / (2 x plain bound) = {(err / bound).max():.3f}")
        assert np.isfinite(got).all() and (err <= bound).all()


def test_split_entry_point_outside_both_envelopes_is_fa_backward():
    assert _plan("causal", "scale_end", (2000,), (33,), 64, 64)[0] == 0
    assert _plan("causal", "scale_end", (2000,), (33,), 64, 64, which="k")[0] == 0
    plain, split = _run_both("causal", "scale_end", 2000, 33, 64, 64, 2, 402)
    assert _same(plain, split)


def test_short_workspace_is_rejected_and_nothing_is_written():
    prob = _problem("full", "none_front", (2600,), (33,), 64, 64, b=2)
    assert _lib.lib().fa_backward_split_workspace_bytes(prob) > _lib.lib().fa_backward_workspace_bytes(prob)
    Q, K, V, dO = _inputs(2, 64, 64, 2600, 33, 403)
    O, l, m = _forward(prob, Q, K, V)
    st, dQ, dK, dV = _abi_backward(prob, Q, K, V, O, l, m, dO, split=True, ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in (dQ, dK, dV):
        assert bool((t.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("policy,mode,nq,nk,d", [("full", "none_front", 2600, 33, 64),
                                                 ("causal", "scale_end", 4200, 64, 128)])
def test_slice_is_bitwise_independent_of_the_batch(policy, mode, nq, nk, d):
    _assert_splits(policy, mode, (nq,), (nk,), d, d)
    Q, K, V, dO = _inputs(3, d, d, nq, nk, 404)

    def run(*ts):
        ts = [t.contiguous() for t in ts]
        prob = _problem(policy, mode, (nq,), (nk,), d, d, b=ts[0].shape[0])
        O, l, m = _forward(prob, *ts[:3])
        st, *grads = _abi_backward(prob, *ts[:3], O, l, m, ts[3], split=True)
        assert st == 0
        return grads

    all3 = run(Q, K, V, dO)
    alone = run(Q[:1], K[:1], V[:1], dO[:1])
    rev = run(Q.flip(0), K.flip(0), V.flip(0), dO.flip(0))
    assert _same([t[0] for t in all3], [t[0] for t in alone])
    assert _same([t[0] for t in all3], [t[2] for t in rev])


def test_two_calls_are_bitwise_equal():
    prob = _problem("causal", "scale_front", (4101,), (33,), 96, 40, b=3)
    Q, K, V, dO = _inputs(3, 96, 40, 4101, 33, 405)
    O, l, m = _forward(prob, Q, K, V)
    st0, *a = _abi_backward(prob, Q, K, V, O, l, m, dO, split=True)
    st1, *b = _abi_backward(prob, Q, K, V, O, l, m, dO, split=True)
    assert st0 == 0 and st1 == 0
    assert _same(a, b)


def test_python_wrappers_take_the_split_path():
    _assert_splits("full", "none_front", (2600,), (33,), 64, 64)
    prob = _problem("full", "none_front", (2600,), (33,), 64, 64, b=2)
    Q, K, V, dO = _inputs(2, 64, 64, 2600, 33, 406)
    O, l, m = _forward(prob, Q, K, V)
    st, dQ, dK, dV = _abi_backward(prob, Q, K, V, O, l, m, dO, split=True)
    assert st == 0
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    fa.full_1d(q, k, v).backward(dO)
    torch.cuda.synchronize()
    assert _same([dQ, dK, dV], [q.grad, k.grad, v.grad])
