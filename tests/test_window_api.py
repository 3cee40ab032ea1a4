"""CPU tests of the sliding-window decode interface: the exports, the host-side statuses of the four
fa_forward_*_window* entry points with pointers that are never dereferenced, the window_size keyword's own errors
(raised before any device call), and that window_size=None still reaches the un-windowed entry points."""

import contextlib
import ctypes

import pytest
import torch

from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

HK = 2
NAMES = ("fa_forward_ragged_window", "fa_forward_paged_window", "fa_forward_ragged_window_fp8",
         "fa_forward_paged_window_fp8", "fa_forward_ragged_window_plan", "fa_forward_paged_window_plan",
         "fa_forward_ragged_window_workspace_bytes", "fa_forward_paged_window_workspace_bytes")


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "sliding-window" in _lib.lib().fa_build_info().decode()
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "fa_api.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header
    assert "They must be finite" in header


def test_the_docstrings_state_the_rule_the_guarantee_and_the_contract():
    for doc in (fa.ragged_1d.__doc__, fa.paged_1d.__doc__):
        assert "max(0, pos - W + 1) <= j <= pos" in doc and "never read" in doc and "must be finite" in doc
    assert "merge_partials([O1, O2], [l1, l2], [m1, m2])" in fa.paged_1d.__doc__
    assert "never loaded" in fa.paged_1d.__doc__


# ------------------------------------------------------------------ the ABI's host-side statuses
PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _prob(nq=4, cap=2048, d=64, g=4, b=None, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, 2 * g if b is None else b, (nq,), (cap,), d, d)


def _launch_ragged(p, g, window, fp8=False, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_ragged_window_workspace_bytes(p, g, window)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_ragged_window_fp8(None, p, g, None, PTR, PTR, None, None, k_lens, kv_per_len, window, None,
                                              None, None, ws, ws_bytes)
    return L.fa_forward_ragged_window(None, p, g, None, PTR, PTR, k_lens, kv_per_len, window, None, None, None, ws,
                                      ws_bytes)


def _launch_paged(p, g, window, page=64, max_pages=32, fp8=False, num_pages=8, kv_per_len=1, ws=PTR, ws_bytes=None,
                  k_lens=PTR, table=PTR, pools=(PTR, PTR)):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_paged_window_workspace_bytes(p, g, page, window)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_paged_window_fp8(None, p, g, None, pools[0], pools[1], None, None, table, max_pages, page,
                                             num_pages, k_lens, kv_per_len, window, None, None, None, ws, ws_bytes)
    return L.fa_forward_paged_window(None, p, g, None, pools[0], pools[1], table, max_pages, page, num_pages, k_lens,
                                     kv_per_len, window, None, None, None, ws, ws_bytes)


FORMS = [(_launch_ragged, False), (_launch_ragged, True), (_launch_paged, False), (_launch_paged, True)]
FORM_IDS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("window", [0, -1, -2 ** 31])
def test_a_window_below_one_is_an_argument_error_with_text(launch, fp8, window):
    assert launch(_prob(), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "window" in _lib.last_error() and ">= 1" in _lib.last_error()
    assert launch(_prob(b=0), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("window", [1, 600, 2047, 2048, 10 ** 6], ids=lambda w: f"w{w}")
def test_the_twins_statuses(launch, fp8, window):
    p = _prob()
    L = _lib.lib()
    need = int(L.fa_forward_ragged_window_workspace_bytes(p, 4, window))
    assert need > 0 and need == int(L.fa_forward_paged_window_workspace_bytes(p, 4, 64, window))
    if window >= 2048:
        assert need == int(L.fa_forward_ragged_workspace_bytes(p, 4))
    # a short or null workspace
    assert launch(p, 4, window, fp8=fp8, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "workspace_bytes" in _lib.last_error()
    assert launch(p, 4, window, fp8=fp8, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    # outside the envelope
    assert launch(_prob(d=136), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    assert launch(_prob(dtype=_lib.F32), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    # an empty batch needs no pointer
    kw = dict(k_lens=None) if launch is _launch_ragged else dict(k_lens=None, table=None, pools=(None, None))
    assert launch(_prob(b=0), 4, window, fp8=fp8, **kw) == _lib.FA_OK
    # the twins' argument errors
    for st in (launch(_prob(policy=_lib.CAUSAL), 4, window, fp8=fp8, ws_bytes=1 << 30),
               launch(p, 3, window, fp8=fp8, ws_bytes=1 << 30), launch(p, 4, window, fp8=fp8, kv_per_len=0),
               launch(p, 4, window, fp8=fp8, kv_per_len=3), launch(p, 4, window, fp8=fp8, k_lens=None)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_the_paged_forms_own_errors(fp8):
    p = _prob()
    assert _launch_paged(p, 4, 600, page=32, max_pages=64, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    assert "page % 64" in _lib.last_error()
    for st in (_launch_paged(p, 4, 600, page=0, fp8=fp8, ws_bytes=1 << 30), _launch_paged(p, 4, 600, max_pages=31, fp8=fp8),
               _launch_paged(p, 4, 600, max_pages=0, fp8=fp8), _launch_paged(p, 4, 600, num_pages=0, fp8=fp8),
               _launch_paged(p, 4, 600, table=None, fp8=fp8), _launch_paged(p, 4, 600, pools=(None, PTR), fp8=fp8)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()


# ------------------------------------------------------------------ the keyword
def _ragged(batch=(3,), hq=8, c=64, cv=64, nq=4, cap=256, kv=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros(batch + (HK, c, cap), dtype=kv),
            torch.zeros(batch + (HK, cv, cap), dtype=kv), torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hq=8, c=64, cv=64, nq=4, page=64, max_pages=4, num_pages=7, kv=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros((num_pages, HK, c, page), dtype=kv),
            torch.zeros((num_pages, HK, cv, page), dtype=kv), torch.zeros(batch + (max_pages,), dtype=torch.int32),
            torch.ones(batch, dtype=torch.int32)]


CALLS = [(fa.ragged_1d, _ragged), (fa.paged_1d, _paged)]
IDS = ["ragged", "paged"]


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_the_keywords_errors(call, args):
    for w in (0, -3):
        with pytest.raises(fa.InvalidArgumentError, match="window_size must be >= 1"):
            call(*args(), tail_causal=True, window_size=w)
    with pytest.raises(fa.InvalidArgumentError, match="requires tail_causal=True"):
        call(*args(), window_size=16)
    with pytest.raises(fa.InvalidArgumentError, match="requires tail_causal=True"):
        call(*args(), tail_causal=False, window_size=10 ** 6)
    for w in (2.0, "8", True):
        with pytest.raises(TypeError, match="window_size must be an int"):
            call(*args(), tail_causal=True, window_size=w)
    # a well-formed windowed call passes every check but the device check; one query takes either tail_causal
    for kw in (dict(tail_causal=True, window_size=16), dict(tail_causal=True, window_size=10 ** 12)):
        with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
            call(*args(), **kw)
    for tail in (False, True):
        with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
            call(*args(nq=1), tail_causal=tail, window_size=16, returning_l_m=True)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(kv=torch.float8_e4m3fn), tail_causal=True, window_size=16, k_scale=torch.ones(HK))
    with pytest.raises(NotImplementedError, match="fused envelope"):
        call(*args(c=136), tail_causal=True, window_size=16)


class _Recorder:
    """Stands in for the library object: every plan is one chunk, every workspace 0 bytes, every forward FA_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            if name.endswith("_plan"):
                a[-1][0] = 1
            return 0
        return f


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_without_a_window_the_call_reaches_the_old_entry_points(monkeypatch, call, args, fp8):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(fa, "_check_device_tensors", lambda *t: None)
    monkeypatch.setattr(fa, "_stream_handle", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    form = "ragged" if call is fa.ragged_1d else "paged"
    a = args(kv=torch.float8_e4m3fn if fp8 else torch.float16)
    tail = "_fp8" if fp8 else ""
    call(*a)
    call(*a, tail_causal=True, window_size=None)
    old = [f"fa_forward_{form}_plan", f"fa_forward_{form}_workspace_bytes", f"fa_forward_{form}{tail}"]
    assert rec.calls == old + old
    rec.calls.clear()
    call(*a, tail_causal=True, window_size=16)
    assert rec.calls == [f"fa_forward_{form}_window_plan", f"fa_forward_{form}_window_workspace_bytes",
                         f"fa_forward_{form}_window{tail}"]
