"""CPU tests of the query-blocked wrappers flash_attention.ragged_prefill_1d / paged_prefill_1d:
the exports, the twins' argument checks with the twins' messages (raised before any device call, so CPU tensors reach
all of them), the wider envelope, and which entry points a call reaches."""

import contextlib

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

HK = 2
NAMES = ("fa_forward_ragged_prefill", "fa_forward_paged_prefill", "fa_forward_ragged_prefill_fp8",
         "fa_forward_paged_prefill_fp8", "fa_forward_ragged_prefill_plan", "fa_forward_paged_prefill_plan",
         "fa_forward_ragged_prefill_workspace_bytes", "fa_forward_paged_prefill_workspace_bytes")


def _ragged(batch=(3,), hq=8, c=64, cv=64, nq=200, cap=256, kv=torch.float16, hk=HK, dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros(batch + (hk, c, cap), dtype=kv),
            torch.zeros(batch + (hk, cv, cap), dtype=kv), torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hq=8, c=64, cv=64, nq=200, page=64, max_pages=4, num_pages=7, kv=torch.float16, hk=HK,
           dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros((num_pages, hk, c, page), dtype=kv),
            torch.zeros((num_pages, hk, cv, page), dtype=kv), torch.zeros(batch + (max_pages,), dtype=torch.int32),
            torch.ones(batch, dtype=torch.int32)]


CALLS = [(fa.ragged_prefill_1d, _ragged), (fa.paged_prefill_1d, _paged)]
IDS = ["ragged", "paged"]


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "query-blocked prefill" in _lib.lib().fa_build_info().decode()
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "fa_api.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header
    for name in ("ragged_prefill_1d", "paged_prefill_1d"):
        assert name in fa.__all__ and name in pkg.__all__ and getattr(pkg, name) is getattr(fa, name)


def test_the_docstrings_say_how_a_mixed_batch_is_laid_out_and_the_twins_point_here():
    for doc in (fa.ragged_prefill_1d.__doc__, fa.paged_prefill_1d.__doc__):
        assert "right-aligns each sequence's real queries in the Nq slots" in doc
        assert "padding queries in front compute earlier\n    positions' rows, or empty rows" in doc
        assert "There is no" in doc and "``window_size``" in doc
    assert "ragged_prefill_1d" in fa.ragged_1d.__doc__ and "paged_prefill_1d" in fa.paged_1d.__doc__


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_there_is_no_window(call, args):
    with pytest.raises(TypeError, match="window_size"):
        call(*args(), tail_causal=True, window_size=16)


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_dtypes_and_scales(call, args):
    with pytest.raises(TypeError, match="unsupported dtype"):
        call(*args(dtype=torch.bfloat16, kv=torch.bfloat16))
    for dt in (torch.float32, torch.float64):
        with pytest.raises(TypeError, match="does not accept"):
            call(*args(dtype=dt, kv=dt))
    a = args()
    a[1] = a[1].float()
    with pytest.raises(TypeError, match="share one dtype"):
        call(*a)
    a = args(kv=torch.float8_e4m3fn)
    a[2] = a[2].to(torch.float16)
    with pytest.raises(TypeError, match="must both be an FP8 cache"):
        call(*a)
    with pytest.raises(fa.InvalidArgumentError, match="a float16 cache takes no scale"):
        call(*args(), k_scale=torch.ones(HK))
    f8 = args(kv=torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="v_scale must be a float32 tensor"):
        call(*f8, v_scale=torch.ones(HK, dtype=torch.float64))
    with pytest.raises(fa.InvalidArgumentError, match=r"shape of k_scale should be \(Hk,\)"):
        call(*f8, k_scale=torch.ones(HK + 1))
    with pytest.raises(fa.InvalidArgumentError, match="k_scale must be on the device of Q"):
        call(*f8, k_scale=torch.ones(HK, device="meta"))
    with pytest.raises(fa.InvalidArgumentError, match="v_scale must be contiguous"):
        call(*f8, v_scale=torch.ones(2 * HK)[::2])


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_lengths_and_table(call, args):
    for bad in (torch.int64, torch.float32):
        a = args()
        a[-1] = a[-1].to(bad)
        with pytest.raises(TypeError, match="k_lens must be an int32 tensor"):
            call(*a)
    a = args()
    a[-1] = [1, 1, 1]
    with pytest.raises(TypeError, match="k_lens must be an int32 tensor"):
        call(*a)
    a = args()
    a[-1] = torch.ones((3, 2), dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="shape of k_lens"):
        call(*a)
    a = args()
    a[-1] = a[-1].to("meta")
    with pytest.raises(fa.InvalidArgumentError, match="on the device of Q"):
        call(*a)
    if call is fa.paged_prefill_1d:
        a = args()
        a[3] = a[3].to(torch.int64)
        with pytest.raises(TypeError, match="block_table must be an int32 tensor"):
            call(*a)
        a = args()
        a[3] = torch.zeros((2, 4), dtype=torch.int32)
        with pytest.raises(fa.InvalidArgumentError, match="shape of block_table"):
            call(*a)
        with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, Hk, channels, page\]"):
            call(a[0], a[1][0], a[2], torch.zeros((3, 4), dtype=torch.int32), a[4])
        with pytest.raises(NotImplementedError, match="page size .* must be a multiple of 64 keys, got page = 32"):
            call(*args(page=32))


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_shapes(call, args):
    with pytest.raises(fa.InvalidArgumentError, match="multiple of"):
        call(*args(hq=7))
    a = args()
    with pytest.raises(fa.InvalidArgumentError, match="[Cc]hannel"):
        call(a[0][:, :, :32], *a[1:])


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_inference_only(call, args, which):
    a = args()
    a[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match=call.__name__ + " is inference only"):
        call(*a)


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("kw", [dict(), dict(nq=4), dict(nq=2048), dict(hq=256, nq=2), dict(hq=2, nq=129), dict(batch=(2, 3)),
                                dict(batch=()), dict(c=40, cv=72, nq=37), dict(kv=torch.float8_e4m3fn)], ids=str)
def test_inside_the_envelope_the_device_check_comes_last(call, args, kw):
    """Well-formed CPU inputs for any number of queries (the twins' shapes among them): the one remaining error is
    that there is no CPU kernel."""
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(**kw))
    a = args(**kw)
    a[0].requires_grad_(True)
    with torch.no_grad(), pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*a, tail_causal=True, returning_l_m=True)


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("kw", [dict(hq=258, nq=2), dict(c=129), dict(cv=136), dict(nq=0)], ids=str)
def test_outside_the_envelope_is_not_implemented(call, args, kw):
    """g = 129 among them: more heads per K/V head than one workgroup's rows."""
    with pytest.raises(NotImplementedError, match="fused envelope .*1 <= g <= 128"):
        call(*args(**kw))


def test_the_twins_keep_their_envelope():
    with pytest.raises(NotImplementedError, match=r"g \* next_pow2\(Nq\) <= 128"):
        fa.ragged_1d(*_ragged())
    with pytest.raises(NotImplementedError, match=r"g \* next_pow2\(Nq\) <= 128"):
        fa.paged_1d(*_paged())


class _Recorder:
    """Stands in for the library object: every plan is one chunk, every workspace 0 bytes, every forward FA_OK."""

    def __init__(self):
        self.calls, self.nargs = [], []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            self.nargs.append(len(a))
            if name.endswith("_plan"):
                a[-1][0] = 1
            return 0
        return f


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_the_call_reaches_the_prefill_entry_points(monkeypatch, call, args, fp8):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(fa, "_check_device_tensors", lambda *t: None)
    monkeypatch.setattr(fa, "_stream_handle", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    form = "ragged" if call is fa.ragged_prefill_1d else "paged"
    out = call(*args(kv=torch.float8_e4m3fn if fp8 else torch.float16), tail_causal=True, returning_l_m=True)
    assert rec.calls == [f"fa_forward_{form}_prefill_plan", f"fa_forward_{form}_prefill_workspace_bytes",
                         f"fa_forward_{form}_prefill" + ("_fp8" if fp8 else "")]
    assert out[0].shape == (3, 8, 64, 200) and out[1].shape == out[2].shape == (3, 8, 200)


ROUTES = {"plain": dict(), "window": dict(window_size=16), "prefill": dict()}


@pytest.mark.parametrize("cache", ["ragged", "paged"])
@pytest.mark.parametrize("form", list(ROUTES))
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_every_cache_and_form_reaches_its_three_entry_points(monkeypatch, cache, form, fp8):
    """All twelve routes {ragged, paged} x {plain, window, prefill} x {f16, fp8}: the plan, the workspace size and the
    forward of that cache and form, in that order, each with as many arguments as the loaded library declares."""
    real = _lib.lib()
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(fa, "_check_device_tensors", lambda *t: None)
    monkeypatch.setattr(fa, "_stream_handle", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    call = getattr(fa, cache + ("_prefill_1d" if form == "prefill" else "_1d"))
    nq = 200 if form == "prefill" else 4
    args = (_ragged if cache == "ragged" else _paged)(nq=nq, kv=torch.float8_e4m3fn if fp8 else torch.float16)
    out = call(*args, tail_causal=True, returning_l_m=True, **ROUTES[form])
    stem = f"fa_forward_{cache}" + ("" if form == "plain" else f"_{form}")
    assert rec.calls == [stem + "_plan", stem + "_workspace_bytes", stem + ("_fp8" if fp8 else "")]
    assert tuple(rec.calls) == fa.decode_entry_points(cache, form, fp8)
    assert rec.nargs == [len(getattr(real, name).argtypes) for name in rec.calls]
    assert out[0].shape == (3, 8, 64, nq) and out[1].shape == out[2].shape == (3, 8, nq)
