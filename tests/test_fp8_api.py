"""CPU tests of the FP8 K/V cache's interface: the argument checks that ragged_1d and paged_1d
gained with k_scale / v_scale and an FP8 cache, every one raised before any device call; the host-side statuses of
fa_forward_ragged_fp8 / fa_forward_paged_fp8, with pointers that are never dereferenced; and quantize_kv_fp8, which
is plain torch and runs on the CPU."""

import ctypes

import numpy as np
import pytest
import torch

import tf_flash_attention_amd as pkg
from tests import fp8_ref
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

F8 = torch.float8_e4m3fn
HK = 2


def _ragged(batch=(3,), hq=8, c=64, cv=64, nq=4, cap=256, kv=F8):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros(batch + (HK, c, cap), dtype=kv),
            torch.zeros(batch + (HK, cv, cap), dtype=kv), torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hq=8, c=64, cv=64, nq=4, page=64, max_pages=2, num_pages=7, kv=F8):
    return [torch.zeros(batch + (hq, c, nq), dtype=torch.float16), torch.zeros((num_pages, HK, c, page), dtype=kv),
            torch.zeros((num_pages, HK, cv, page), dtype=kv), torch.zeros(batch + (max_pages,), dtype=torch.int32),
            torch.ones(batch, dtype=torch.int32)]


CALLS = [(fa.ragged_1d, _ragged), (fa.paged_1d, _paged)]
IDS = ["ragged", "paged"]


def _scale(n=HK):
    return torch.ones(n, dtype=torch.float32)


def test_exported():
    assert "quantize_kv_fp8" in fa.__all__
    assert "quantize_kv_fp8" in pkg.__all__ and pkg.quantize_kv_fp8 is fa.quantize_kv_fp8
    for name in ("fa_forward_ragged_fp8", "fa_forward_paged_fp8"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "fp8" in _lib.lib().fa_build_info().decode()


def test_the_docstring_gives_the_fp8_append_recipe():
    doc = fa.paged_1d.__doc__
    assert "quantize_kv_fp8(new, head_axis=0, scale=k_scale)" in doc
    assert "K_pool[block_table[s, pos // page], :, :, pos % page] = new8" in doc


# ------------------------------------------------------------------ the wrappers' checks
@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("kv", [F8, torch.uint8], ids=["float8_e4m3fn", "uint8"])
@pytest.mark.parametrize("scales", [False, True], ids=["none", "scales"])
def test_an_fp8_cache_passes_every_check_but_the_device_check(call, args, kv, scales):
    kw = dict(k_scale=_scale(), v_scale=_scale()) if scales else {}
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(kv=kv), **kw)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*args(kv=kv, batch=()), tail_causal=True, returning_l_m=True, **kw)


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_k_and_v_must_both_be_fp8(call, args):
    a = args()
    a[2] = a[2].to(torch.float16)
    with pytest.raises(TypeError, match="must both be an FP8 cache"):
        call(*a)
    a = args()
    a[1] = a[1].to(torch.float16)
    with pytest.raises(TypeError, match="share one dtype"):
        call(*a)
    a = args(kv=F8)
    a[2] = a[2].view(torch.uint8)  # the same bytes under either dtype: fine
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*a)


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("name", ["k_scale", "v_scale"])
def test_a_float16_cache_takes_no_scale(call, args, name):
    with pytest.raises(fa.InvalidArgumentError, match=name + " was given, but .* are not an FP8 cache"):
        call(*args(kv=torch.float16), **{name: _scale()})


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("name", ["k_scale", "v_scale"])
@pytest.mark.parametrize("bad", [torch.float16, torch.float64, torch.int32])
def test_scales_must_be_float32_tensors(call, args, name, bad):
    with pytest.raises(TypeError, match=name + " must be a float32 tensor"):
        call(*args(), **{name: _scale().to(bad)})
    with pytest.raises(TypeError, match=name + " must be a float32 tensor"):
        call(*args(), **{name: [1.0, 1.0]})
    with pytest.raises(TypeError, match=name + " must be a float32 tensor"):
        call(*args(), **{name: 1.0})


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("name", ["k_scale", "v_scale"])
@pytest.mark.parametrize("shape", [(), (1,), (3,), (HK, 1), (1, HK), (8,)])
def test_scale_shape_is_the_kv_heads(call, args, name, shape):
    with pytest.raises(fa.InvalidArgumentError, match=r"shape of " + name + r" should be \(Hk,\) = \[2\]"):
        call(*args(), **{name: torch.ones(shape, dtype=torch.float32)})


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
@pytest.mark.parametrize("name", ["k_scale", "v_scale"])
def test_scale_device_and_contiguity(call, args, name):
    with pytest.raises(fa.InvalidArgumentError, match=name + " must be on the device of Q"):
        call(*args(), **{name: _scale().to("meta")})
    with pytest.raises(fa.InvalidArgumentError, match=name + " must be contiguous"):
        call(*args(), **{name: torch.ones(2 * HK, dtype=torch.float32)[::2]})


@pytest.mark.parametrize("call,args", CALLS, ids=IDS)
def test_the_other_checks_are_unchanged_with_an_fp8_cache(call, args):
    a = args()
    a[-1] = a[-1].to(torch.int64)
    with pytest.raises(TypeError, match="k_lens must be an int32 tensor"):
        call(*a, k_scale=_scale())
    a = args()
    a[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        call(*a)
    with pytest.raises(NotImplementedError, match="fused envelope"):
        call(*args(c=136))
    with pytest.raises(NotImplementedError, match="multiple of 64 keys"):
        fa.paged_1d(*_paged(page=32))


# ------------------------------------------------------------------ the ABI's host-side statuses
PTR = ctypes.c_void_p(256)  # a non-null pointer that no case here may touch


def _prob(nq=4, cap=2048, d=64, g=4, b=None, policy=_lib.FULL, dtype=_lib.F16):
    return _lib.make_problem(dtype, policy, 1, _lib.NONE_FRONT, 2 * g if b is None else b, (nq,), (cap,), d, d)


def _launch_ragged(p, g, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR, scales=(None, None)):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_ragged_workspace_bytes(p, g)) if ws_bytes is None else ws_bytes
    return L.fa_forward_ragged_fp8(None, p, g, None, PTR, PTR, scales[0], scales[1], k_lens, kv_per_len, 0, None, None,
                                   None, ws, ws_bytes)


def _launch_paged(p, g, page, max_pages, num_pages=8, kv_per_len=1, ws=PTR, ws_bytes=None, k_lens=PTR, table=PTR,
                  pools=(PTR, PTR), scales=(None, None)):
    L = _lib.lib()
    ws_bytes = int(L.fa_forward_paged_workspace_bytes(p, g, page)) if ws_bytes is None else ws_bytes
    return L.fa_forward_paged_fp8(None, p, g, None, pools[0], pools[1], scales[0], scales[1], table, max_pages, page,
                                  num_pages, k_lens, kv_per_len, 0, None, None, None, ws, ws_bytes)


def test_the_workspace_is_the_fp16_twins_and_a_short_one_is_rejected():
    p = _prob()
    need = int(_lib.lib().fa_forward_ragged_workspace_bytes(p, 4))
    assert need > 0 and need == int(_lib.lib().fa_forward_paged_workspace_bytes(p, 4, 64))
    assert _launch_ragged(p, 4, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "fa_forward_ragged_workspace_bytes" in _lib.last_error()
    assert _launch_ragged(p, 4, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert _launch_paged(p, 4, 64, 32, ws_bytes=need - 1) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
    assert "fa_forward_paged_workspace_bytes" in _lib.last_error()
    assert _launch_paged(p, 4, 64, 32, ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL


def test_outside_the_envelope_is_unsupported():
    assert _launch_ragged(_prob(d=136), 4) == _lib.FA_ERR_UNSUPPORTED
    assert _launch_ragged(_prob(dtype=_lib.F32), 4) == _lib.FA_ERR_UNSUPPORTED
    assert _launch_paged(_prob(), 4, 32, 64) == _lib.FA_ERR_UNSUPPORTED and "page % 64" in _lib.last_error()
    assert _launch_paged(_prob(d=136), 4, 64, 32) == _lib.FA_ERR_UNSUPPORTED


def test_an_empty_batch_is_ok_and_needs_no_pointer():
    p = _prob(b=0)
    assert _launch_ragged(p, 4, k_lens=None) == _lib.FA_OK
    assert _launch_paged(p, 4, 64, 32, k_lens=None, table=None, pools=(None, None)) == _lib.FA_OK


def test_argument_errors_are_the_fp16_twins():
    p = _prob()
    for st in (_launch_ragged(_prob(policy=_lib.CAUSAL), 4), _launch_ragged(p, 3), _launch_ragged(p, 4, kv_per_len=0),
               _launch_ragged(p, 4, kv_per_len=3), _launch_ragged(p, 4, k_lens=None),
               _launch_paged(p, 4, 0, 32), _launch_paged(p, 4, 64, 31), _launch_paged(p, 4, 64, 0),
               _launch_paged(p, 4, 64, 32, num_pages=0), _launch_paged(p, 4, 64, 32, table=None),
               _launch_paged(p, 4, 64, 32, pools=(None, PTR)), _launch_paged(p, 4, 64, 32, k_lens=None)):
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and _lib.last_error()


# ------------------------------------------------------------------ quantize_kv_fp8
def test_quantize_computes_a_per_head_amax_scale_and_round_trips():
    rng = np.random.default_rng(3)
    x = rng.uniform(-2, 2, (3, HK, 5, 70)).astype(np.float32)
    x[:, 1] *= 100.0
    x8, scale = fa.quantize_kv_fp8(torch.from_numpy(x), head_axis=1)
    assert x8.dtype == F8 and x8.shape == x.shape and scale.dtype == torch.float32 and scale.shape == (HK,)
    amax = np.abs(x).max(axis=(0, 2, 3))
    assert np.allclose(scale.numpy(), amax / 448.0, rtol=1e-6)
    b8 = x8.view(torch.uint8).numpy()
    assert not np.isin(b8 & 0x7F, [0x7F]).any()
    # torch's division and cast against the numpy reference on the same quotient
    q = x / scale.numpy().reshape(1, HK, 1, 1)
    assert (b8 == fp8_ref.encode(q.astype(np.float32))).all()
    back = fp8_ref.dequantize(b8, scale.numpy(), 1)
    assert (np.abs(back - x) <= np.maximum(np.abs(x) * 2.0 ** -4, amax.reshape(1, HK, 1, 1) / 448 * 2.0 ** -10) * 1.001).all()
    # a negative head axis, and a head of zeros
    z8, zs = fa.quantize_kv_fp8(torch.zeros(HK, 4, 8), head_axis=-3)
    assert zs.tolist() == [1.0, 1.0] and (z8.view(torch.uint8) == 0).all()


def test_quantize_with_a_given_scale_clamps_instead_of_making_nan():
    x = torch.tensor([[500.0, -1e6, 1.0, 464.0], [3.0, -3.0, 0.0, 1e-3]]).reshape(HK, 1, 4)
    scale = torch.tensor([1.0, 0.5])
    x8, s = fa.quantize_kv_fp8(x, head_axis=0, scale=scale)
    assert s is scale
    got = x8.view(torch.uint8).numpy()
    assert (got == fp8_ref.quantize(np.clip(x.numpy(), -448 * scale.numpy().reshape(HK, 1, 1), 448 * scale.numpy().reshape(HK, 1, 1)),
                                    scale.numpy(), 0)).all()
    assert got[0, 0].tolist()[:2] == [0x7E, 0xFE]
    with pytest.raises(TypeError, match="scale must be a float32 tensor"):
        fa.quantize_kv_fp8(x, 0, scale=scale.double())
    with pytest.raises(fa.InvalidArgumentError, match=r"shape of scale should be \(Hk,\)"):
        fa.quantize_kv_fp8(x, 0, scale=torch.ones(3))
