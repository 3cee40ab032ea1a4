"""CPU tests of the 256-channel paged forward's host side: the exported names, the plan and the
workspace of fa_forward_paged_wide, its refusals, and the routing of flash_attention.paged_1d.  Every error is raised
before any device call, so null pointers and CPU tensors reach all of them."""

import ctypes

import pytest
import torch

from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

NAMES = ("fa_forward_paged_wide_plan", "fa_forward_paged_wide_workspace_bytes", "fa_forward_paged_wide")
OK, INVALID, UNSUPPORTED = _lib.FA_OK, _lib.FA_ERR_INVALID_ARGUMENT, _lib.FA_ERR_UNSUPPORTED


def _problem(g=2, d=256, v=256, nq=1, cap=4096, slices=3, dtype=_lib.F16):
    return _lib.make_problem(dtype, _lib.FULL, 1, _lib.NONE_FRONT, slices * g, (nq,), (cap,), d, v)


def _plan(prob, g, page=64):
    out = (ctypes.c_int32 * 6)()
    return _lib.lib().fa_forward_paged_wide_plan(prob, g, page, out), tuple(out)


def _forward(prob, g, page=64, tail=0, window=0, ptr=0):
    """fa_forward_paged_wide with every pointer ``ptr`` (null: no call here gets as far as a launch)."""
    L = _lib.lib()
    need = int(L.fa_forward_paged_wide_workspace_bytes(prob, g, page))
    return L.fa_forward_paged_wide(None, prob, g, ptr, ptr, ptr, ptr, prob.k_seq[0] // page, page, 9, ptr, 1, tail,
                                   window, ptr, ptr, ptr, 1, need)


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("g,nq,rows", [(2, 1, 2), (5, 2, 10), (16, 8, 128)])
@pytest.mark.parametrize("j", [1, 2, 5])
@pytest.mark.parametrize("off", [-64, 0, 64])
def test_plan_and_workspace_follow_the_chunk_formula_and_do_not_depend_on_b(g, nq, rows, j, off):
    """Spans one tile below, at and one tile above 64 * 64 * j keys: chunk = max(ceil(span / 4096) * 64, 512 up to 64
    rows or 1024 above), chunks = ceil(span / chunk), 64-row blocks of (v_d + 3) * 64 floats a chunk."""
    span = 64 * 64 * j + off
    chunk = max(-(-span // 4096) * 64, 512 if rows <= 64 else 1024)
    want = (-(-span // chunk), chunk, rows // g, rows, -(-rows // 64), 0)
    for slices in (1, 7):
        prob = _problem(g=g, nq=nq, cap=span, slices=slices, v=192)
        assert _plan(prob, g) == (OK, want)
        assert (_lib.lib().fa_forward_paged_wide_workspace_bytes(prob, g, 64)
                == -(-slices * want[4] * want[0] * 64 * 195 * 4 // 256) * 256)


@pytest.mark.parametrize("kw,page", [(dict(d=129), 64), (dict(d=320), 64), (dict(v=136), 64), (dict(d=128, v=128), 64),
                                     (dict(), 32), (dict(g=32, nq=5), 64), (dict(dtype=_lib.F32), 64)], ids=str)
def test_outside_the_envelope(kw, page):
    g = kw.get("g", 2)
    prob = _problem(**kw)
    assert _plan(prob, g, page)[0] == OK and _plan(prob, g, page)[1][0] == 0
    assert _lib.lib().fa_forward_paged_wide_workspace_bytes(prob, g, page) == 0
    assert _forward(prob, g, page) == UNSUPPORTED and "fused envelope" in _lib.last_error()


def test_a_window_requires_the_tail_rule():
    prob = _problem(nq=2)
    assert _forward(prob, 2, window=100) == INVALID and "tail_causal" in _lib.last_error()
    assert _forward(prob, 2, window=-1) == INVALID
    assert _forward(prob, 2, tail=1, window=100) == INVALID and "null" in _lib.last_error()  # (as far as the pointers)
    assert _forward(_problem(slices=0), 2, tail=1, window=100) == OK  # b == 0: nothing launched


@pytest.mark.parametrize("c,cv,kw", [(256, 256, {}), (192, 128, dict(tail_causal=True)),
                                     (128, 256, dict(tail_causal=True, window_size=100))])
def test_paged_1d_routes_wide_heads_and_the_device_check_comes_last(c, cv, kw):
    mk = lambda *s: torch.zeros(s, dtype=torch.float16)  # noqa: E731
    a = [mk(3, 4, c, 2), mk(7, 2, c, 64), mk(7, 2, cv, 64), torch.zeros(3, 2, dtype=torch.int32),
         torch.ones(3, dtype=torch.int32)]
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.paged_1d(*a, **kw)
    with pytest.raises(NotImplementedError, match="fused envelope"):  # a draft mask stays outside
        fa.paged_1d(*a, tail_causal=True, draft_mask=torch.zeros(3, 2, 1, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="fused envelope"):
        fa.paged_prefill_1d(*a)
