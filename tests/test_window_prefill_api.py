"""CPU tests of the sliding-window prefill interface: the exports, the host-side statuses of the four
fa_forward_*_window_prefill* entry points with pointers that are never dereferenced, the wrappers' own errors (raised
before any device call), which entry points a call reaches, and that the un-windowed prefill wrappers still take no
window."""

import contextlib
import ctypes

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

HK = 2
NAMES = ("fa_forward_ragged_window_prefill", "fa_forward_paged_window_prefill", "fa_forward_ragged_window_prefill_fp8",
         "fa_forward_paged_window_prefill_fp8", "fa_forward_ragged_window_prefill_plan",
         "fa_forward_paged_window_prefill_plan", "fa_forward_ragged_window_prefill_workspace_bytes",
         "fa_forward_paged_window_prefill_workspace_bytes")


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "sliding-window prefill" in _lib.lib().fa_build_info().decode()
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "fa_api.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header
    for name in ("ragged_window_prefill_1d", "paged_window_prefill_1d"):
        assert name in fa.__all__ and name in pkg.__all__ and getattr(pkg, name) is getattr(fa, name)
    assert "window_prefill" in _lib.DECODE_FORMS
    assert _lib.decode_entry_points("paged", "window_prefill", True) == (
        "fa_forward_paged_window_prefill_plan", "fa_forward_paged_window_prefill_workspace_bytes",
        "fa_forward_paged_window_prefill_fp8")
    for cache in _lib.DECODE_CACHES:  # the `_window` entry points' argument lists
        for fp8 in (False, True):
            for a, b in zip(_lib.decode_entry_points(cache, "window", fp8), _lib.decode_entry_points(cache, "window_prefill", fp8)):
                assert getattr(_lib.lib(), a).argtypes == getattr(_lib.lib(), b).argtypes


def test_the_docstrings_state_the_contract_and_the_parents_point_here():
    for doc in (fa.ragged_window_prefill_1d.__doc__, fa.paged_window_prefill_1d.__doc__):
        assert "read on the device" in doc and "captured graph" in doc
        assert "right-align" in doc and "must be finite" in doc and "never read" in doc
        assert "max(0, k_lens[s] - Nq - W + 1)" in doc and "merge_partials" in doc
    assert "max(0, pos - W + 1) <= j <= pos" in fa.ragged_window_prefill_1d.__doc__
    assert "never\n    loaded" in fa.paged_window_prefill_1d.__doc__
    for twin, new in ((fa.ragged_prefill_1d, "ragged_window_prefill_1d"), (fa.paged_prefill_1d, "paged_window_prefill_1d")):
        assert "There is no" in twin.__doc__ and "``window_size``" in twin.__doc__ and new in twin.__doc__


# ------------------------------------------------------------------ the ABI's host-side statuses
PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _prob(nq=200, cap=2048, d=64, g=4, b=None, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, 2 * g if b is None else b, (nq,), (cap,), d, d)


def _launch_ragged(p, g, window, fp8=False, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_ragged_window_prefill_workspace_bytes(p, g, window)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_ragged_window_prefill_fp8(None, p, g, None, PTR, PTR, None, None, k_lens, kv_per_len, window,
                                                      None, None, None, ws, ws_bytes)
    return L.fa_forward_ragged_window_prefill(None, p, g, None, PTR, PTR, k_lens, kv_per_len, window, None, None, None, ws,
                                              ws_bytes)


def _launch_paged(p, g, window, page=64, max_pages=32, fp8=False, num_pages=8, kv_per_len=1, ws=PTR, ws_bytes=None,
                  k_lens=PTR, table=PTR, pools=(PTR, PTR)):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_paged_window_prefill_workspace_bytes(p, g, page, window)) if ws_bytes is None else ws_bytes
    if fp8:
        return L.fa_forward_paged_window_prefill_fp8(None, p, g, None, pools[0], pools[1], None, None, table, max_pages,
                                                     page, num_pages, k_lens, kv_per_len, window, None, None, None, ws,
                                                     ws_bytes)
    return L.fa_forward_paged_window_prefill(None, p, g, None, pools[0], pools[1], table, max_pages, page, num_pages,
                                             k_lens, kv_per_len, window, None, None, None, ws, ws_bytes)


FORMS = [(_launch_ragged, False), (_launch_ragged, True), (_launch_paged, False), (_launch_paged, True)]
FORM_IDS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("window", [0, -1, -2 ** 31])
def test_a_window_below_one_is_an_argument_error_with_text(launch, fp8, window):
    assert launch(_prob(), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "window" in _lib.last_error() and ">= 1" in _lib.last_error()
    assert launch(_prob(b=0), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_INVALID_ARGUMENT
    L = _lib.lib()
    out = (ctypes.c_int32 * 8)()
    assert L.fa_forward_ragged_window_prefill_plan(_prob(), 4, window, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert L.fa_forward_paged_window_prefill_plan(_prob(), 4, 64, window, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert L.fa_forward_ragged_window_prefill_workspace_bytes(_prob(), 4, window) == 0


@pytest.mark.parametrize("launch,fp8", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("nq", [4, 200], ids=["one-block", "blocks"])
@pytest.mark.parametrize("window", [1, 600, 2047, 2048, 10 ** 6], ids=lambda w: f"w{w}")
def test_the_statuses(launch, fp8, window, nq):
    """The undelegated call (nq = 200 under a window below the capacity) and both delegations refuse alike."""
    p = _prob(nq=nq)
    L = _lib.lib()
    need = int(L.fa_forward_ragged_window_prefill_workspace_bytes(p, 4, window))
    assert need > 0 and need == int(L.fa_forward_paged_window_prefill_workspace_bytes(p, 4, 64, window))
    if window >= 2048:
        assert need == int(L.fa_forward_ragged_prefill_workspace_bytes(p, 4))
    elif nq == 4:
        assert need == int(L.fa_forward_ragged_window_workspace_bytes(p, 4, window))
    # a short or null workspace
    assert launch(p, 4, window, fp8=fp8, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "workspace_bytes" in _lib.last_error()
    assert launch(p, 4, window, fp8=fp8, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    # outside the envelope
    assert launch(_prob(nq=nq, d=136), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    assert "envelope" in _lib.last_error()
    assert launch(_prob(nq=nq, dtype=_lib.F32), 4, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    assert launch(_prob(nq=nq, g=129), 129, window, fp8=fp8, ws_bytes=1 << 30) == _lib.FA_ERR_UNSUPPORTED
    # an empty batch needs no pointer
    kw = dict(k_lens=None) if launch is _launch_ragged else dict(k_lens=None, table=None, pools=(None, None))
    assert launch(_prob(nq=nq, b=0), 4, window, fp8=fp8, **kw) == _lib.FA_OK
    # the twins' argument errors
    for st in (launch(_prob(nq=nq, policy=_lib.CAUSAL), 4, window, fp8=fp8, ws_bytes=1 << 30),
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


# ------------------------------------------------------------------ the wrappers
def _ragged(batch=(3,), hq=8, c=64, cv=64, nq=200, cap=256, kv=torch.float16, hk=HK, dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros(batch + (hk, c, cap), dtype=kv),
            torch.zeros(batch + (hk, cv, cap), dtype=kv), torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hq=8, c=64, cv=64, nq=200, page=64, max_pages=4, num_pages=7, kv=torch.float16, hk=HK,
           dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros((num_pages, hk, c, page), dtype=kv),
            torch.zeros((num_pages, hk, cv, page), dtype=kv), torch.zeros(batch + (max_pages,), dtype=torch.int32),
            torch.ones(batch, dtype=torch.int32)]


CALLS = [(fa.ragged_window_prefill_1d, _ragged), (fa.paged_window_prefill_1d, _paged)]
IDS = ["ragged", "paged"]


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_the_windows_errors(call, args):
    with pytest.raises(TypeError, match="window_size"):
        call(*args())  # required
    for w in (0, -3):
        with pytest.raises(fa.InvalidArgumentError, match="window_size must be >= 1"):
            call(*args(), w)
    for w in (2.0, "8", True, None):
        with pytest.raises(TypeError, match="window_size must be an int"):
            call(*args(), window_size=w)
    with pytest.raises(TypeError, match="tail_causal"):
        call(*args(), 16, tail_causal=True)  # the tail rule is implied, not a keyword
    # a well-formed call passes every check but the device check, whatever the window and the number of queries
    for kw in (dict(), dict(nq=1), dict(nq=4), dict(nq=2048), dict(hq=256, nq=2), dict(batch=()), dict(c=40, cv=72, nq=37)):
        for w in (1, 16, 10 ** 12):
            with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
                call(*args(**kw), w, returning_l_m=True)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(kv=torch.float8_e4m3fn), window_size=16, k_scale=torch.ones(HK))


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_the_twins_errors(call, args):
    with pytest.raises(fa.InvalidArgumentError, match="a float16 cache takes no scale"):
        call(*args(), 16, k_scale=torch.ones(HK))
    a = args()
    a[-1] = a[-1].to(torch.int64)
    with pytest.raises(TypeError, match="k_lens must be an int32 tensor"):
        call(*a, 16)
    a = args()
    a[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match=call.__name__ + " is inference only"):
        call(*a, 16)
    for kw in (dict(hq=258, nq=2), dict(c=129), dict(cv=136), dict(nq=0)):
        with pytest.raises(NotImplementedError, match="fused envelope .*1 <= g <= 128"):
            call(*args(**kw), 16)
    if call is fa.paged_window_prefill_1d:
        with pytest.raises(NotImplementedError, match="page size .* must be a multiple of 64 keys, got page = 32"):
            call(*args(page=32), 16)


def test_the_parents_keep_their_signatures_and_envelopes():
    for call, args in ((fa.ragged_prefill_1d, _ragged), (fa.paged_prefill_1d, _paged)):
        with pytest.raises(TypeError, match="window_size"):
            call(*args(), tail_causal=True, window_size=16)
    with pytest.raises(NotImplementedError, match=r"g \* next_pow2\(Nq\) <= 128"):
        fa.ragged_1d(*_ragged(), tail_causal=True, window_size=16)
    with pytest.raises(NotImplementedError, match=r"g \* next_pow2\(Nq\) <= 128"):
        fa.paged_1d(*_paged(), tail_causal=True, window_size=16)


class _Recorder:
    """Stands in for the library object: every plan is one chunk, every workspace 0 bytes, every forward FA_OK."""

    def __init__(self):
        self.calls, self.nargs, self.args = [], [], []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            self.nargs.append(len(a))
            self.args.append(a)
            if name.endswith("_plan"):
                a[-1][0] = 1
            return 0
        return f


@pytest.mark.parametrize("cache", ["ragged", "paged"])
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("window,sent", [(16, 16), (2 ** 40, 2 ** 31 - 1)])
def test_every_route_reaches_its_three_entry_points(monkeypatch, cache, fp8, window, sent):
    """{ragged, paged} x {f16, fp8}: the plan, the workspace size and the forward of the form, in that order, each with
    as many arguments as the loaded library declares, and the window (clamped to 2^31 - 1) where the ABI takes it."""
    real = _lib.lib()
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(fa, "_check_device_tensors", lambda *t: None)
    monkeypatch.setattr(fa, "_stream_handle", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    call = getattr(fa, cache + "_window_prefill_1d")
    args = (_ragged if cache == "ragged" else _paged)(kv=torch.float8_e4m3fn if fp8 else torch.float16)
    out = call(*args, window, returning_l_m=True)
    stem = f"fa_forward_{cache}_window_prefill"
    assert rec.calls == [stem + "_plan", stem + "_workspace_bytes", stem + ("_fp8" if fp8 else "")]
    assert tuple(rec.calls) == fa.decode_entry_points(cache, "window_prefill", fp8)
    assert rec.nargs == [len(getattr(real, name).argtypes) for name in rec.calls]
    assert rec.args[0][-2] == sent and rec.args[1][-1] == sent and rec.args[2][-6] == sent
    assert out[0].shape == (3, 8, 64, 200) and out[1].shape == out[2].shape == (3, 8, 200)
