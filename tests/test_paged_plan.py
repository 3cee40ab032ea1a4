"""CPU tests of the paged forward's routing rule (include/fa_api.h: fa_forward_paged_plan,
fa_forward_paged_workspace_bytes, the host checks of fa_forward_paged).  Host-only: no device
work."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib


def _prob(nq=4, cap=2048, d=64, vd=None, g=4, b=None, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, 2 * g if b is None else b, (nq,), (cap,), d,
                             d if vd is None else vd)


def _plan(p, g, page):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_paged_plan(p, g, page, out) == _lib.FA_OK
    return tuple(out)


def _ragged_plan(p, g):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_ragged_plan(p, g, out) == _lib.FA_OK
    return tuple(out)


def _bytes(p, g, page):
    return int(_lib.lib().fa_forward_paged_workspace_bytes(p, g, page))


PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _launch(p, g, page, max_pages, num_pages=8, kv_per_len=1, ws_bytes=None, ws=PTR, table=PTR, pools=(PTR, PTR),
            k_lens=PTR):
    """fa_forward_paged with pointers that are never dereferenced: every case here returns before a launch."""
    ws_bytes = _bytes(p, g, page) if ws_bytes is None else ws_bytes
    return _lib.lib().fa_forward_paged(None, p, g, None, pools[0], pools[1], table, max_pages, page, num_pages, k_lens,
                                       kv_per_len, 0, None, None, None, ws, ws_bytes)


@pytest.mark.parametrize("page", [64, 128, 192, 256])
@pytest.mark.parametrize("max_pages", [1, 3, 41, 256])
@pytest.mark.parametrize("nq,g,d", [(1, 1, 64), (33, 1, 128), (1, 8, 32), (3, 3, 96), (64, 2, 64), (4, 4, 128)])
def test_plan_and_workspace_are_the_ragged_ones_over_the_capacity(nq, g, d, page, max_pages):
    p = _prob(nq=nq, cap=max_pages * page, d=d, g=g, b=6 * g)
    plan = _plan(p, g, page)
    assert plan == _ragged_plan(p, g)
    assert plan[0] >= 1 and plan[2:4] == (0, max_pages * page)
    need = _bytes(p, g, page)
    assert need == int(_lib.lib().fa_forward_ragged_workspace_bytes(p, g)) and need > 0


@pytest.mark.parametrize("page", [1, 16, 32, 96])
def test_a_page_that_is_no_multiple_of_64_is_outside_the_envelope(page):
    p = _prob(cap=24 * page)
    assert _ragged_plan(p, 4)[0] >= 1
    assert _plan(p, 4, page)[0] == 0
    assert _bytes(p, 4, page) == 0
    assert _launch(p, 4, page, 24) == _lib.FA_ERR_UNSUPPORTED
    assert "page % 64" in _lib.last_error()


@pytest.mark.parametrize("kw", [dict(d=129), dict(nq=33, g=4), dict(dtype=_lib.F32), dict(nq=0)], ids=str)
def test_outside_the_ragged_envelope(kw):
    p = _prob(**kw)
    g = kw.get("g", 4)
    assert _plan(p, g, 64)[0] == 0 and _bytes(p, g, 64) == 0
    assert _launch(p, g, 64, 32) == _lib.FA_ERR_UNSUPPORTED


def test_plan_does_not_depend_on_batch():
    assert len({_plan(_prob(b=4 * bkv), 4, 128) for bkv in (0, 1, 5, 4096)}) == 1


@pytest.mark.parametrize("page,text", [(0, "page must be >= 1"), (-64, "page must be >= 1"),
                                       (192, "not a multiple of page")])
def test_plan_argument_errors(page, text):
    p = _prob(cap=2048)
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    assert _lib.lib().fa_forward_paged_plan(p, 4, page, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert text in _lib.last_error()
    assert tuple(out) == (-7,) * 6
    assert _bytes(p, 4, page) == 0


def test_null_plan_buffer():
    assert _lib.lib().fa_forward_paged_plan(_prob(), 4, 64, None) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "null plan buffer" in _lib.last_error()


@pytest.mark.parametrize("kw,text", [
    (dict(page=0, max_pages=32), "page must be >= 1"),
    (dict(page=-1, max_pages=32), "page must be >= 1"),
    (dict(page=64, max_pages=0), "max_pages must be >= 1"),
    (dict(page=64, max_pages=-3), "max_pages must be >= 1"),
    (dict(page=64, max_pages=31), "max_pages * page = 1984 is not the capacity"),
    (dict(page=128, max_pages=32), "max_pages * page = 4096 is not the capacity"),
    (dict(page=64, max_pages=32, num_pages=0), "num_pages must be >= 1"),
    (dict(page=64, max_pages=32, num_pages=-5), "num_pages must be >= 1"),
    (dict(page=64, max_pages=32, table=None), "null block_table"),
    (dict(page=64, max_pages=32, pools=(None, PTR)), "null K_pool or V_pool"),
    (dict(page=64, max_pages=32, pools=(PTR, None)), "null K_pool or V_pool"),
    (dict(page=64, max_pages=32, k_lens=None), "null k_lens"),
    (dict(page=64, max_pages=32, kv_per_len=0), "kv_per_len must be >= 1"),
    (dict(page=64, max_pages=32, kv_per_len=4), "multiple of kv_per_len"),
], ids=lambda x: x if isinstance(x, str) else None)
def test_launch_argument_errors(kw, text):
    p = _prob(cap=2048, b=24)  # 6 K/V slices
    kw = dict(kw)
    page, max_pages = kw.pop("page"), kw.pop("max_pages")
    assert _launch(p, 4, page, max_pages, ws_bytes=1 << 30, **kw) == _lib.FA_ERR_INVALID_ARGUMENT
    assert text in _lib.last_error()


def test_the_ragged_forwards_own_argument_errors():
    assert _launch(_prob(b=7, g=2), 2, 64, 32) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "multiple of kv_group" in _lib.last_error()
    assert _launch(_prob(b=4), 0, 64, 32) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "kv_group" in _lib.last_error()
    assert _launch(_prob(policy=_lib.CAUSAL), 4, 64, 32) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "FA_FULL" in _lib.last_error()


def test_short_workspace():
    p = _prob(cap=2048, b=24)
    need = _bytes(p, 4, 64)
    assert _launch(p, 4, 64, 32, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "fa_forward_paged_workspace_bytes" in _lib.last_error()
    assert _launch(p, 4, 64, 32, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL


def test_an_empty_batch_is_ok_with_null_pointers():
    p0 = _prob(b=0)
    assert _bytes(p0, 4, 64) == 0
    assert _launch(p0, 4, 64, 32, table=None, pools=(None, None), k_lens=None) == _lib.FA_OK
