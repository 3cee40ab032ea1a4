"""GPU tests of the split-key fp16 forward (csrc/fa_fwd_f16_splitk.hip): few
queries against a long key range, one workgroup per (slice, key chunk) and a merge kernel.

Every parity case goes through tests.test_gpu_parity.run_case (float64 oracle, its existing
tolerances, forward and backward, rows that attend nothing exactly O = 0, l = 0, m = bytes 0xFA) after
asserting through fa_forward_split_plan that the shape really splits into >= 3 chunks with a shorter
last chunk.  The remaining tests call the C ABI directly: routing, workspace check, bitwise
independence of the batch, determinism."""

import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import run_case
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}


def _problem(policy, mode, qs, ks, d, vd, b=1, ws=1, ls=0, causal=False, dtype=_lib.F16):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], b, qs, ks, d, vd, ws, ls, causal)


def _plan(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False):
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(_problem(policy, mode, qs, ks, d, vd, 1, ws, ls, causal), out) == 0
    return tuple(out)


def _assert_splits(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False):
    chunks, chunk, kb, ke = _plan(policy, mode, qs, ks, d, vd, ws, ls, causal)
    assert chunks >= 3, (chunks, chunk, kb, ke)
    assert (ke - kb // 64 * 64) % chunk != 0, "the last chunk should be a partial one"


def _split_case(policy, mode, qs, ks, d, vd, ws=1, ls=0, causal=False, batch=(2,), seed=0, misalign=False):
    _assert_splits(policy, mode, qs, ks, d, vd, ws, ls, causal)
    return run_case(np.float16, policy, len(qs), mode, batch, d, vd, qs, ks, ws=ws, ls=ls, causal=causal, seed=seed,
                    misalign=misalign)


# ------------------------------------------------------------------ parity against the oracle
@pytest.mark.parametrize("d,vd", [(64, 64), (128, 128), (96, 40), (33, 100), (8, 8)])
@pytest.mark.parametrize("nq", [1, 33, 128])
def test_full_1d_queries_and_channels(nq, d, vd):
    _split_case("full", "none_front", (nq,), (2600,), d, vd, seed=nq + d)


@pytest.mark.parametrize("mode", ["none_front", "scale_front", "scale_end"])
def test_causal_1d_sync_modes(mode):
    """nq << nk: under scale_front the early rows see few keys, so whole chunks are empty for them;
    under none_front the causal range is the first 33 keys and the plan must not split."""
    qs, ks = (33,), (4101,)
    if mode == "none_front":
        assert _plan("causal", mode, qs, ks, 64, 64)[0] == 0
        return
    _split_case("causal", mode, qs, ks, 64, 64, seed=7)


@pytest.mark.parametrize("d", [64, 128])
def test_causal_scale_end_64_queries(d):
    _split_case("causal", "scale_end", (64,), (4200,), d, d, seed=d)


@pytest.mark.parametrize("policy,mode", [("full", "none_front"), ("full", "scale_front"), ("causal", "scale_end")])
def test_2d(policy, mode):
    _split_case(policy, mode, (4, 8), (40, 66), 64, 48, seed=11)


def test_causal_2d_short_ranges_do_not_split():
    for mode in ("none_front", "scale_front"):
        chunks, _, kb, ke = _plan("causal", mode, (4, 8), (40, 66), 64, 48)
        assert ke - kb < 2048 and chunks == 0


@pytest.mark.parametrize("causal,mode", [(False, "none_front"), (True, "scale_front")])
def test_local_1d_window_3000(causal, mode):
    _split_case("local", mode, (128,), (4101,), 64, 64, ws=3000, causal=causal, seed=13)


def test_local_1d_causal_none_front_does_not_split():
    assert _plan("local", "none_front", (128,), (4101,), 64, 64, ws=3000, causal=True)[0] == 0


@pytest.mark.parametrize("causal", [False, True])
def test_local_2d_strided(causal):
    """Window 20 at stride 2 under scale_end: the per-element rule check (POL 2) inside split chunks."""
    _split_case("local", "scale_end", (4, 8), (40, 66), 64, 64, ws=20, ls=1, causal=causal, seed=17)


def test_rows_without_any_key():
    """64 x 2 queries against 33 x 80 keys, window 10: the query rows past key row 42 attend nothing in
    any chunk (run_case checks O = 0, l = 0, m = bytes 0xFA for them), the others merge as usual."""
    from oracle import fa_oracle as O
    mask = O.problem_mask(O.Problem("local", 2, "scale_front", 10, 0, False), (64, 2), (33, 80))
    empty = ~np.asarray(mask).reshape(128, -1).any(axis=1)
    assert 0 < empty.sum() < 128
    _split_case("local", "scale_front", (64, 2), (33, 80), 64, 64, ws=10, seed=19)


def test_misaligned_pointers():
    _split_case("full", "none_front", (33,), (2600,), 64, 64, seed=23, misalign=True)


@pytest.mark.parametrize("d", [64, 128])
def test_ragged_key_length(d):
    _split_case("causal", "scale_end", (33,), (2603,), d, d, seed=29)


# The <D, POL, FAST> instances of splitk_partial_kernel that no case above reaches (the others are
# D 64 / 128 under POL 0 / 1 with both stagings, D 64 POL 2 FAST and D 32 POL 0 element-wise): the
# 32-channel tile under every rule form, and the per-element rule check (POL 2) with element-wise
# staging at D = 64 and with both stagings at D = 128.  FAST needs d == v_d == D and nk % 8 == 0.
@pytest.mark.parametrize("policy,mode,qs,ks,d,vd,ws,ls", [
    ("full", "none_front", (33,), (2600,), 32, 32, 1, 0),       # D 32, POL 0, FAST
    ("causal", "scale_end", (64,), (4200,), 32, 32, 1, 0),      # D 32, POL 1, FAST
    ("causal", "scale_end", (33,), (2603,), 24, 17, 1, 0),      # D 32, POL 1, element-wise
    ("local", "scale_end", (4, 8), (40, 66), 32, 32, 20, 1),    # D 32, POL 2, FAST
    ("local", "scale_end", (4, 8), (40, 66), 24, 17, 20, 1),    # D 32, POL 2, element-wise
    ("local", "scale_end", (4, 8), (40, 66), 64, 48, 20, 1),    # D 64, POL 2, element-wise
    ("local", "scale_end", (4, 8), (40, 66), 128, 128, 20, 1),  # D 128, POL 2, FAST
    ("local", "scale_end", (4, 8), (40, 66), 100, 72, 20, 1),   # D 128, POL 2, element-wise
])
def test_partial_kernel_instances(policy, mode, qs, ks, d, vd, ws, ls):
    _split_case(policy, mode, qs, ks, d, vd, ws=ws, ls=ls, seed=31 + d)


# ------------------------------------------------------------------ the C ABI directly
def _inputs(b, d, vd, nq, nk, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) * 4 - 2).half().cuda()  # noqa: E731
    return mk(b, d, nq), mk(b, d, nk), mk(b, vd, nk)


def _abi_forward(prob, Q, K, V, use_ws, ws_short=0, fill=None):
    """fa_forward (use_ws False) or fa_forward_ws on device tensors; returns (status, O, l, m)."""
    L = _lib.lib()
    b, nq, vd = Q.shape[0], Q.shape[2], V.shape[1]
    O = torch.empty((b, vd, nq), dtype=torch.float16, device=Q.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=Q.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=Q.device)
    if fill is not None:
        for t in (O, l, m):
            t.view(torch.uint8).fill_(fill)
    stream = torch.cuda.current_stream().cuda_stream
    if use_ws:
        need = int(L.fa_forward_workspace_bytes(prob))
        ws = torch.empty(max(need, 64), dtype=torch.uint8, device=Q.device)
        st = L.fa_forward_ws(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), l.data_ptr(),
                             m.data_ptr(), ws.data_ptr(), max(need - ws_short, 0) if need else 64)
    else:
        st = L.fa_forward(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), l.data_ptr(),
                          m.data_ptr())
    torch.cuda.synchronize()
    return st, O, l, m


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_ws_entry_point_outside_the_envelope_is_fa_forward():
    prob = _problem("causal", "scale_end", (33,), (300,), 64, 64, b=2)
    assert _lib.lib().fa_forward_workspace_bytes(prob) == 0
    Q, K, V = _inputs(2, 64, 64, 33, 300, 1)
    st0, *ref = _abi_forward(prob, Q, K, V, use_ws=False)
    st1, *got = _abi_forward(prob, Q, K, V, use_ws=True)
    assert st0 == 0 and st1 == 0
    assert _same(ref, got)


def test_short_workspace_is_rejected_and_nothing_is_written():
    prob = _problem("full", "none_front", (33,), (2600,), 64, 64, b=2)
    assert _lib.lib().fa_forward_workspace_bytes(prob) > 0
    Q, K, V = _inputs(2, 64, 64, 33, 2600, 2)
    st, O, l, m = _abi_forward(prob, Q, K, V, use_ws=True, ws_short=1, fill=0x5A)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    for t in (O, l, m):
        assert bool((t.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("policy,mode,nq,nk,d", [("full", "none_front", 33, 2600, 64),
                                                 ("causal", "scale_end", 64, 4200, 128)])
def test_slice_is_bitwise_independent_of_the_batch(policy, mode, nq, nk, d):
    _assert_splits(policy, mode, (nq,), (nk,), d, d)
    Q, K, V = _inputs(3, d, d, nq, nk, 3)
    run = lambda q, k, v: _abi_forward(_problem(policy, mode, (nq,), (nk,), d, d, b=q.shape[0]), q, k, v,  # noqa: E731
                                       use_ws=True)
    st3, *all3 = run(Q, K, V)
    st1, *alone = run(Q[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous())
    str_, *rev = run(Q.flip(0).contiguous(), K.flip(0).contiguous(), V.flip(0).contiguous())
    assert st3 == 0 and st1 == 0 and str_ == 0
    assert _same([t[0] for t in all3], [t[0] for t in alone])
    assert _same([t[0] for t in all3], [t[2] for t in rev])


def test_two_calls_are_bitwise_equal():
    prob = _problem("causal", "scale_front", (33,), (4101,), 96, 40, b=3)
    Q, K, V = _inputs(3, 96, 40, 33, 4101, 4)
    st0, *a = _abi_forward(prob, Q, K, V, use_ws=True)
    st1, *b = _abi_forward(prob, Q, K, V, use_ws=True)
    assert st0 == 0 and st1 == 0
    assert _same(a, b)


def test_python_wrappers_take_the_split_path():
    _assert_splits("full", "none_front", (33,), (2600,), 64, 64)
    Q, K, V = _inputs(2, 64, 64, 33, 2600, 5)
    st, *direct = _abi_forward(_problem("full", "none_front", (33,), (2600,), 64, 64, b=2), Q, K, V, use_ws=True)
    assert st == 0
    got = fa.full_1d(Q, K, V, returning_l_m=True)
    torch.cuda.synchronize()
    assert _same(direct, got)
