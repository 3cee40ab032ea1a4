"""CPU tests of the sliding-window plans (fa_forward_ragged_window_plan, fa_forward_paged_window_plan and the two
workspace functions): host-only arithmetic, no device.  The launched chunks per K/V slice must
cover, for EVERY length, the chunks the window's keys [lo, L) touch, which is shown by brute force; and the plan is a
pure function of the problem without b."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib


def _prob(nq, nk, d=64, vd=64, b=None, g=1, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, g if b is None else b, (nq,), (nk,), d, vd)


def _plan(p, g, window, page=None):
    out = (ctypes.c_int32 * 8)(*([-7] * 8))
    L = _lib.lib()
    st = L.fa_forward_ragged_window_plan(p, g, window, out) if page is None else \
        L.fa_forward_paged_window_plan(p, g, page, window, out)
    assert st == _lib.FA_OK, _lib.last_error()
    return tuple(out)


def _ws(p, g, window, page=None):
    L = _lib.lib()
    return int(L.fa_forward_ragged_window_workspace_bytes(p, g, window) if page is None else
               L.fa_forward_paged_window_workspace_bytes(p, g, page, window))


def _twin_plan(p, g, page=None):
    out = (ctypes.c_int32 * 6)()
    L = _lib.lib()
    assert (L.fa_forward_ragged_plan(p, g, out) if page is None else L.fa_forward_paged_plan(p, g, page, out)) == 0
    return tuple(out)


GRID = [(nk, nq, w, g)
        for nk in (1, 63, 64, 600, 2600, 2624, 5000, 70000)
        for nq in (1, 4, 33)
        for w in (1, 2, 63, 64, 65, 511, 512, 513, 1000, 4096, 66000)
        for g in (1, 2, 8) if g * (1 if nq == 1 else 4 if nq == 4 else 64) <= 128 and w < nk
        and (nk < 70000 or w >= 4096)]  # (the brute force over a long capacity only where the chunk grows)


@pytest.mark.parametrize("nk,nq,w,g", GRID)
def test_the_launched_chunks_cover_every_length(nk, nq, w, g):
    n_launch, chunk, span_w, cap_chunks, pitch, rows, delegated, reserved = _plan(_prob(nq, nk, g=g), g, w)
    assert (delegated, reserved) == (0, 0)
    assert span_w == min(nk, w + nq - 1)
    assert pitch == (1 if nq == 1 else 4 if nq == 4 else 64) and rows == g * pitch
    min_chunk = 512 if rows <= 64 else 1024
    assert chunk == max(min_chunk, -(-(-(-span_w // 64)) // 64) * 64) and chunk % 64 == 0
    assert cap_chunks == -(-nk // chunk)
    assert n_launch == min(cap_chunks, (span_w + chunk - 2) // chunk + 1) and n_launch >= 1
    worst = 0
    for L in range(0, nk + 1):
        lo = max(0, L - nq - w + 1)
        touched = (L - 1) // chunk - lo // chunk + 1 if L > 0 else 0
        assert touched <= n_launch, (L, lo)
        worst = max(worst, touched)
        # the tiles a launched workgroup runs stay inside its chunk, and the first staged tile holds lo
        first = max(lo // chunk * chunk, lo // 64 * 64)
        assert lo // chunk * chunk <= first <= lo < first + 64 or L == 0
    assert worst == n_launch  # the formula is tight: some length needs every launched chunk


@pytest.mark.parametrize("nk,nq,w,g", [(2600, 4, 512, 2), (16384, 1, 1024, 8), (16384, 4, 4096, 4), (70000, 33, 66000, 2)])
def test_the_workspace_follows_the_launched_chunks_and_b_does_not_enter_the_plan(nk, nq, w, g):
    plans = set()
    for bkv in (1, 3, 32):
        p = _prob(nq, nk, vd=40, b=bkv * g, g=g)
        plan = _plan(p, g, w)
        plans.add(plan)
        n_launch, rows = plan[0], plan[5]
        need = bkv * n_launch * (40 + 3) * rows * 4
        assert _ws(p, g, w) == -(-need // 256) * 256
    assert len(plans) == 1
    twin = _twin_plan(_prob(nq, nk, g=g), g)
    if w + nq - 1 <= nk // 4:
        assert plan[0] < twin[0]  # the point of the feature: fewer workgroups and a smaller workspace


@pytest.mark.parametrize("page", [None, 64, 128])
@pytest.mark.parametrize("w", [2560, 2561, 2 ** 31 - 1])
def test_a_window_that_reaches_the_capacity_is_delegated_with_the_twins_values(page, w):
    nk, nq, g = 2560, 4, 2
    p = _prob(nq, nk, b=6 * g, g=g)
    twin = _twin_plan(p, g, page)
    assert _plan(p, g, w, page) == (twin[0], twin[1], nk, twin[0], twin[4], twin[5], 1, 0)
    L = _lib.lib()
    twin_ws = int(L.fa_forward_ragged_workspace_bytes(p, g) if page is None else L.fa_forward_paged_workspace_bytes(p, g, page))
    assert _ws(p, g, w, page) == twin_ws > 0
    assert _plan(p, g, nk - 1, page)[6] == 0


def test_the_paged_plan_is_the_ragged_plan_inside_the_envelope():
    p = _prob(4, 2560, g=2)
    for w in (1, 64, 513, 2559):
        assert _plan(p, 2, w, 64) == _plan(p, 2, w, 128) == _plan(p, 2, w)
        assert _ws(p, 2, w, 64) == _ws(p, 2, w) > 0


def test_a_window_below_one_is_an_argument_error_with_text():
    p = _prob(4, 2560, g=2)
    out = (ctypes.c_int32 * 8)()
    L = _lib.lib()
    for w in (0, -1, -2 ** 31):
        assert L.fa_forward_ragged_window_plan(p, 2, w, out) == _lib.FA_ERR_INVALID_ARGUMENT
        assert "window" in _lib.last_error() and ">= 1" in _lib.last_error()
        assert L.fa_forward_paged_window_plan(p, 2, 64, w, out) == _lib.FA_ERR_INVALID_ARGUMENT
        assert "window" in _lib.last_error()
        assert _ws(p, 2, w) == 0 and _ws(p, 2, w, 64) == 0
    assert L.fa_forward_ragged_window_plan(p, 2, 8, None) == _lib.FA_ERR_INVALID_ARGUMENT
    # the twins' own argument errors come first
    assert L.fa_forward_ragged_window_plan(_prob(4, 2560, g=2, policy=_lib.CAUSAL), 2, 8, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "FA_FULL" in _lib.last_error()
    assert L.fa_forward_ragged_window_plan(p, 3, 8, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert L.fa_forward_paged_window_plan(p, 2, 100, 8, out) == _lib.FA_ERR_INVALID_ARGUMENT  # 2560 % 100 != 0


@pytest.mark.parametrize("w", [8, 5000])
def test_outside_the_envelope_the_plan_gives_no_chunks_and_no_bytes(w):
    for p, g, page in ((_prob(4, 2560, d=136, vd=136, g=2), 2, None), (_prob(4, 2560, g=2, dtype=_lib.F32), 2, None),
                       (_prob(4, 2560, b=64, g=64), 64, None), (_prob(4, 2560, g=2), 2, 32),
                       (_prob(4, 2560, d=136, vd=136, g=2), 2, 64)):
        plan = _plan(p, g, w, page)
        assert plan[0] == 0 and plan[7] == 0
        assert _ws(p, g, w, page) == 0
