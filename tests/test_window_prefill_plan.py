"""CPU tests of the sliding-window prefill plans (fa_forward_ragged_window_prefill_plan, the paged one and the two
workspace functions): host-only arithmetic, no device.  The plan is checked against a mirror written
here from include/fa_api.h's text; by brute force over every length and block, the absolute chunks that a block's key
interval [lo_b, L_b) touches number at most the launched chunks, and the merge's live-chunk count (restated here from
fa_fwd_f16_window_prefill.h) is the brute-force count."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib


def _prob(nq, nk, d=64, vd=64, b=None, g=1):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, g if b is None else b, (nq,), (nk,), d, vd)


def _call(stem, p, g, page, window, n=8):
    out = (ctypes.c_int32 * n)(*([-7] * n))
    L = _lib.lib()
    own = (p, g) + (() if page is None else (page,)) + (() if window is None else (window,))
    name = "fa_forward_" + ("ragged" if page is None else "paged") + stem
    assert getattr(L, name + "_plan")(*own, out) == _lib.FA_OK, _lib.last_error()
    return tuple(out), int(getattr(L, name + "_workspace_bytes")(*own))


def _plan(p, g, window, page=None):
    return _call("_window_prefill", p, g, page, window)


def _next_pow2(n):
    return 1 << (n - 1).bit_length()


def _model(g, nq, nk, window):
    """(launched, chunk, span_w, cap_chunks, P_b, rows, nqb) of an undelegated call, from the header's text."""
    pb = max(p for p in (1, 2, 4, 8, 16, 32, 64, 128) if g * p <= 128)
    rows, nqb = g * pb, -(-nq // pb)
    span_w = min(nk, window + pb - 1)
    kmax = max(1, 64 // nqb)
    min_chunk = 512 if rows <= 64 else 1024
    chunk = max(min_chunk, -(-(-(-span_w // kmax)) // 64) * 64)
    cap_chunks = -(-nk // chunk)
    return min(cap_chunks, (span_w + chunk - 2) // chunk + 1), chunk, span_w, cap_chunks, pb, rows, nqb


GROUPS = (1, 2, 3, 4, 8, 16, 128)
QUERIES = (1, 2, 3, 4, 8, 9, 16, 17, 20, 32, 33, 37, 64, 65, 128, 129, 256, 300, 512, 2048)
CAPS = (1, 64, 192, 1100, 2560, 16384, 70000, 1 << 20)
WINDOWS = (1, 2, 63, 64, 65, 511, 512, 513, 1000, 4096, 40000)


@pytest.mark.parametrize("g", GROUPS)
def test_the_plan_is_the_headers_formula_and_its_two_delegations(g):
    seen = set()
    for nk in CAPS:
        for nq in QUERIES:
            p = _prob(nq, nk, g=g)
            for window in WINDOWS + (nk - 1, nk, nk + 1, 2 ** 31 - 1):
                if window < 1:
                    continue
                plan, ws = _plan(p, g, window)
                launched, chunk, span_w, cap_chunks, pb, rows, nqb = _model(g, nq, nk, window)
                one_block = g * _next_pow2(nq) <= 128
                assert one_block == (nqb == 1)
                if window >= nk:  # the query-blocked form's tail call
                    parent, parent_ws = _call("_prefill", p, g, None, None)
                    assert plan == (parent[0], parent[1], nk, parent[0], pb, rows, nqb, 1), (g, nq, nk, window)
                    assert ws == parent_ws > 0
                elif one_block:   # the windowed twin
                    parent, parent_ws = _call("_window", p, g, None, window)
                    assert parent[6] == 0
                    assert plan == (parent[0], parent[1], parent[2], parent[3], pb, rows, 1, 2), (g, nq, nk, window)
                    assert ws == parent_ws > 0
                else:
                    assert plan == (launched, chunk, span_w, cap_chunks, pb, rows, nqb, 0), (g, nq, nk, window)
                    assert chunk % 64 == 0 and 1 <= launched <= cap_chunks
                    # b / kv_group * nqb * launched records of rows * (v_d + 3) floats, rounded up to 256 bytes
                    assert ws == -(-(nqb * launched * rows * (64 + 3) * 4) // 256) * 256
                seen.add(plan[7])
                if nk % 64 == 0 and nq in (1, 17, 129, 2048):
                    assert _plan(p, g, window, 64) == (plan, ws)
    assert seen == {0, 1, 2}


def test_the_workspace_counts_the_slices_and_the_plan_does_not():
    p1, p6 = _prob(300, 2560, g=4), _prob(300, 2560, b=24, g=4)
    (plan1, ws1), (plan6, ws6) = _plan(p1, 4, 700), _plan(p6, 4, 700)
    launched, chunk, span_w, cap_chunks, pb, rows, nqb = plan1[:7]
    assert plan1 == plan6 and plan1[7] == 0
    assert ws1 == -(-(nqb * launched * rows * 67 * 4) // 256) * 256
    assert ws6 == -(-(6 * nqb * launched * rows * 67 * 4) // 256) * 256


def test_outside_the_envelope_the_plan_is_zero():
    for p, g, page in ((_prob(200, 2560, d=136, g=4), 4, None), (_prob(200, 2560, g=129), 129, None), (_prob(200, 2560, g=4), 4, 32)):
        for window in (600, 10 ** 6):
            assert _plan(p, g, window, page) == ((0,) * 8, 0)


def _block(g, nq, nk, L, qb, pb, window):
    """(nq_b, L_b, lo_b) of block qb of a sequence of L live keys, from the header's text."""
    q0 = qb * pb
    nq_b = min(pb, nq - q0)
    lb = min(max(L - nq + q0 + nq_b, 0), L)
    return nq_b, lb, max(lb - nq_b - window + 1, 0)


def _live_chunks(launched, chunk, lb, lo):
    """the merge's count (fa_fwd_f16_window_prefill.h: window_block_chunks)"""
    return 0 if lb < 1 else min(launched, (lb - 1) // chunk - lo // chunk + 1)


@pytest.mark.parametrize("g,nq,nk,window", [(1, 129, 2600, 1), (1, 129, 2601, 513), (1, 300, 2600, 1000), (8, 17, 2601, 64),
                                             (8, 37, 2600, 511), (16, 20, 2601, 512), (128, 2, 2600, 2), (4, 1000, 2601, 65),
                                             (1, 256, 2600, 2599), (3, 40, 2601, 1500), (2, 2048, 2600, 63)])
def test_brute_force_over_every_length_and_block(g, nq, nk, window):
    """For every length in [0, nk] and every block: the absolute chunks that hold a key some query of the block sees
    (counted query by query from the definition) are the contiguous run from lo_b / chunk on, number at most the
    launched chunks, and number exactly the merge's live-chunk count, so every one is launched and folded."""
    (launched, chunk, span_w, cap_chunks, pb, rows, nqb, delegated), _ = _plan(_prob(nq, nk, g=g), g, window)
    assert delegated == 0 and nqb == -(-nq // pb) >= 2
    most, empties = 0, 0
    for L in range(0, nk + 1):
        for qb in range(nqb):
            nq_b, lb, lo = _block(g, nq, nk, L, qb, pb, window)
            # from the definition: query q at pos = L - nq + q sees [max(0, pos - W + 1), pos] if pos >= 0; the block's
            # queries are consecutive, so their union is one interval: from the first live query's lower end to the
            # last query's position
            pos_last = L - nq + qb * pb + nq_b - 1
            if pos_last < 0:
                assert lb == 0 and _live_chunks(launched, chunk, lb, lo) == 0
                empties += 1
                continue
            pos_first = max(L - nq + qb * pb, 0)
            first_key, last_key = max(0, pos_first - window + 1), pos_last
            assert (first_key, last_key) == (lo, lb - 1), (L, qb)
            touched = last_key // chunk - first_key // chunk + 1
            assert touched <= launched, (L, qb, touched, launched)
            assert _live_chunks(launched, chunk, lb, lo) == touched
            assert lb - lo <= span_w
            # the tiles the workgroup of relative chunk c stages lie inside [lo & ~63, L_b) and inside its chunk
            for c in range(launched):
                cs = (lo // chunk + c) * chunk
                kt0, end = max(cs, lo & ~63), min(cs + chunk, lb)
                assert (kt0 < end) == (c < touched)
            most = max(most, touched)
    assert most == launched  # no chunk is launched that no length needs
    assert empties > 0
