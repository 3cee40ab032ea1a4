"""CPU tests of the fused K/V append's argument checks: flash_attention.ragged_append_1d and
paged_append_1d raise every error before any device call, so CPU tensors reach all of them and the device check is the
last; fa_append_* check every argument on the host before any device call, so ctypes reaches every
FA_ERR_INVALID_ARGUMENT and the envelope without a GPU."""

import ctypes

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

NAMES = ("fa_append_ragged", "fa_append_paged", "fa_append_ragged_fp8", "fa_append_paged_fp8")
FP8 = getattr(torch, "float8_e4m3fn", torch.uint8)


def _ragged(batch=(3,), hk=2, c=64, cv=64, n_new=4, cap=100, dtype=torch.float16):
    """[K, V, K_new, V_new, k_lens]"""
    return [torch.zeros(batch + (hk, c, cap), dtype=dtype), torch.zeros(batch + (hk, cv, cap), dtype=dtype),
            torch.zeros(batch + (hk, c, n_new), dtype=torch.float16), torch.zeros(batch + (hk, cv, n_new), dtype=torch.float16),
            torch.ones(batch, dtype=torch.int32)]


def _paged(batch=(3,), hk=2, c=64, cv=64, n_new=4, page=64, max_pages=2, num_pages=7, dtype=torch.float16):
    """[K_pool, V_pool, K_new, V_new, block_table, k_lens]"""
    return [torch.zeros((num_pages, hk, c, page), dtype=dtype), torch.zeros((num_pages, hk, cv, page), dtype=dtype),
            torch.zeros(batch + (hk, c, n_new), dtype=torch.float16), torch.zeros(batch + (hk, cv, n_new), dtype=torch.float16),
            torch.zeros(batch + (max_pages,), dtype=torch.int32), torch.ones(batch, dtype=torch.int32)]


CALLS = [(fa.ragged_append_1d, _ragged), (fa.paged_append_1d, _paged)]
IDS = ["ragged", "paged"]


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "fused K/V append" in _lib.lib().fa_build_info().decode()
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "fa_api.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header
    for name in ("ragged_append_1d", "paged_append_1d"):
        assert name in fa.__all__ and name in pkg.__all__ and getattr(pkg, name) is getattr(fa, name)
    assert [_lib.append_entry_point(c, f) for c in ("ragged", "paged") for f in (False, True)] == [
        "fa_append_ragged", "fa_append_ragged_fp8", "fa_append_paged", "fa_append_paged_fp8"]


def test_the_docstrings_point_to_the_appends_and_keep_the_recipes():
    doc = fa.paged_1d.__doc__
    assert "paged_append_1d" in doc and "paged_append_1d" in fa.paged_prefill_1d.__doc__
    assert "ragged_append_1d" in fa.quantize_kv_fp8.__doc__ and "paged_append_1d" in fa.quantize_kv_fp8.__doc__
    assert "K_pool[block_table[s, pos // page], :, :, pos % page] = new\n" in doc
    assert "K_pool[block_table[s, pos // page], :, :, pos % page] = new8" in doc
    assert "quantize_kv_fp8(new, head_axis=0, scale=k_scale)" in doc
    assert "never loaded" in doc and "merge_partials([O1, O2], [l1, l2], [m1, m2])" in doc
    for f in (fa.ragged_append_1d, fa.paged_append_1d):
        assert "Returns None" in f.__doc__
    out = fa.paged_append_1d.__doc__
    assert "allocates no" in out and "computes no scales" in out and "copy-on-write" in out


def test_cache_shapes():
    a = _ragged()
    with pytest.raises(fa.InvalidArgumentError, match=r"batch \+ \(Hk, channels, cap\)"):
        fa.ragged_append_1d(a[0][0, 0], *a[1:])
    with pytest.raises(fa.InvalidArgumentError, match=r"batch \+ \(Hk, channels, cap\)"):
        fa.ragged_append_1d(a[0], a[1][None], *a[2:])
    for bad in (a[1][:2], a[1][:, :1], a[1][..., :50]):
        with pytest.raises(fa.InvalidArgumentError, match="agree in the batch shape, Hk and cap"):
            fa.ragged_append_1d(a[0], bad, *a[2:])
    a = _paged()
    with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, Hk, channels, page\]"):
        fa.paged_append_1d(a[0][0], *a[1:])
    with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, Hk, channels, page\]"):
        fa.paged_append_1d(a[0], a[1][None], *a[2:])
    for bad in (a[1][:5], a[1][:, :1], a[1][..., :32]):
        with pytest.raises(fa.InvalidArgumentError, match="agree in num_pages, Hk and page"):
            fa.paged_append_1d(a[0], bad, *a[2:])
    with pytest.raises(fa.InvalidArgumentError, match="should hold a page"):
        fa.paged_append_1d(*_paged(num_pages=0))


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
def test_new_tokens_are_float16_tensors_of_the_caches_shape(call, make):
    for which, name in ((2, "K_new"), (3, "V_new")):
        for bad in (torch.float32, torch.bfloat16, FP8):
            a = make()
            a[which] = a[which].to(bad)
            with pytest.raises(TypeError, match=name + " must be a float16 tensor"):
                call(*a)
        a = make()
        a[which] = a[which].tolist()
        with pytest.raises(TypeError, match=name + " must be a float16 tensor"):
            call(*a)
    a = make()
    for which, bad in ((2, a[2][:2]), (2, a[2][:, :1]), (2, a[2][:, :, :32]), (2, a[2][..., :3]), (3, a[3][..., :3]),
                       (3, a[3][:, :, :32]), (2, a[2][0, 0]), (3, a[3][None])):
        b = list(a)
        b[which] = bad
        with pytest.raises(fa.InvalidArgumentError, match=r"K_new and V_new should be batch \+ \(Hk, C, Nnew\)"):
            call(*b)


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
def test_cache_dtypes_and_scales(call, make):
    what = "K and V" if make is _ragged else "K_pool and V_pool"
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(TypeError, match="K_new and V_new, " + what + " must share one dtype"):
            call(*make(dtype=dt))
    a = make()
    a[0] = a[0].to(FP8)
    with pytest.raises(TypeError, match="must both be an FP8 cache"):
        call(*a)
    one = torch.ones(2, dtype=torch.float32)
    with pytest.raises(fa.InvalidArgumentError, match="k_scale was given, but " + what + " are not an FP8 cache"):
        call(*make(), k_scale=one)
    with pytest.raises(fa.InvalidArgumentError, match="v_scale was given"):
        call(*make(), v_scale=one)
    for dt in (FP8, torch.uint8):
        with pytest.raises(TypeError, match="k_scale must be a float32 tensor"):
            call(*make(dtype=dt), k_scale=one.double())
        with pytest.raises(TypeError, match="v_scale must be a float32 tensor"):
            call(*make(dtype=dt), v_scale=[1.0, 1.0])
        with pytest.raises(fa.InvalidArgumentError, match=r"shape of k_scale should be \(Hk,\)"):
            call(*make(dtype=dt), k_scale=torch.ones(3))
        with pytest.raises(fa.InvalidArgumentError, match="v_scale must be on the device of K_new and V_new"):
            call(*make(dtype=dt), v_scale=one.to("meta"))
        with pytest.raises(fa.InvalidArgumentError, match="k_scale must be contiguous"):
            call(*make(dtype=dt), k_scale=torch.ones(4)[::2])


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
@pytest.mark.parametrize("bad", [torch.int64, torch.int16, torch.float32])
def test_int32_tensors(call, make, bad):
    names = ["k_lens"] if make is _ragged else ["block_table", "k_lens"]
    for i, name in enumerate(names):
        a = make()
        a[4 + i] = a[4 + i].to(bad)
        with pytest.raises(TypeError, match=name + " must be an int32 tensor"):
            call(*a)
        a[4 + i] = a[4 + i].tolist()
        with pytest.raises(TypeError, match=name + " must be an int32 tensor"):
            call(*a)
    a = make()
    with pytest.raises(TypeError, match="new_lens must be an int32 tensor"):
        call(*a, new_lens=a[-1].to(bad))
    with pytest.raises(TypeError, match="new_lens must be an int32 tensor"):
        call(*a, new_lens=[1, 1, 1])


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
@pytest.mark.parametrize("batch,shape", [((3,), (3, 2)), ((3,), (2,)), ((3,), ()), ((2, 3), (6,)), ((), (1,))])
def test_lengths_have_the_batch_shape(call, make, batch, shape):
    a = make(batch=batch)
    good = a[-1]
    a[-1] = torch.ones(shape, dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="shape of k_lens"):
        call(*a)
    a[-1] = good
    with pytest.raises(fa.InvalidArgumentError, match="shape of new_lens"):
        call(*a, new_lens=torch.ones(shape, dtype=torch.int32))


@pytest.mark.parametrize("batch,shape", [((3,), (3,)), ((3,), (2, 2)), ((3,), (3, 2, 2)), ((2, 3), (6, 2)), ((), (1, 2)),
                                         ((3,), (3, 0))])
def test_block_table_shape_is_the_batch_shape_plus_max_pages(batch, shape):
    a = _paged(batch=batch)
    a[4] = torch.zeros(shape, dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="shape of block_table"):
        fa.paged_append_1d(*a)


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
def test_devices(call, make):
    what = "K and V" if make is _ragged else "K_pool and V_pool"
    for which in range(1, len(make())):
        a = make()
        a[which] = a[which].to("meta")
        with pytest.raises(fa.InvalidArgumentError, match="must be on the device of " + what):
            call(*a)
    a = make()
    with pytest.raises(fa.InvalidArgumentError, match="new_lens, K_new and V_new must be on the device of " + what):
        call(*a, new_lens=a[-1].to("meta"))


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_inference_only(call, make, which):
    a = make()
    a[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        call(*a)


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
@pytest.mark.parametrize("which", [0, 1])
def test_a_cache_that_is_not_contiguous_is_refused(call, make, which):
    """A .contiguous() copy would silently take the write."""
    a = make(c=32, cv=32)
    wide = make(c=64, cv=64)[which]
    a[which] = wide[..., ::2, :]
    assert not a[which].is_contiguous() and a[which].shape == make(c=32, cv=32)[which].shape
    with pytest.raises(fa.InvalidArgumentError, match="must be contiguous: the append writes in place"):
        call(*a)
    # K_new and V_new may be anything: they are only read
    a = make()
    a[2] = make(n_new=8)[2][..., ::2]
    assert not a[2].is_contiguous()
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*a)


@pytest.mark.parametrize("page", [32, 16, 96, 1])
def test_a_small_page_is_not_implemented_and_the_text_names_the_condition(page):
    with pytest.raises(NotImplementedError, match="paged_append_1d: the page size .* must be a multiple of 64 keys, "
                                                  "got page = " + str(page)):
        fa.paged_append_1d(*_paged(page=page))


@pytest.mark.parametrize("call,make", CALLS, ids=IDS)
@pytest.mark.parametrize("batch", [(3,), (2, 3), ()])
@pytest.mark.parametrize("dtype", [torch.float16, FP8], ids=["f16", "fp8"])
def test_the_device_check_comes_last(call, make, batch, dtype):
    """Well-formed CPU inputs, also under no_grad with an input that requires grad, with new_lens and scales: the one
    remaining error is that there is no CPU kernel."""
    kw = dict(page=192) if make is _paged else dict(c=1, cv=160)
    a = make(batch=batch, dtype=dtype, **kw)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*a)
    a[2].requires_grad_(True)
    sc = dict(k_scale=torch.ones(2), v_scale=torch.ones(2)) if dtype is not torch.float16 else {}
    with torch.no_grad(), pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        call(*a, new_lens=torch.ones(batch, dtype=torch.int32), **sc)


# ---- the C entry points through ctypes: every check is made on the host before any device call, and the pointers
# are never dereferenced there, so made-up non-null values stand for device buffers
PTR = 0x1000


def _c_args(cache, fp8, sequences=3, kv_heads=2, d=64, v_d=64, n_new=4, max_pages=2, page=64, num_pages=7, nk=None,
            K_new=PTR, V_new=PTR, K=PTR, V=PTR, table=PTR, k_lens=PTR, new_lens=None):
    nk = max_pages * page if nk is None else nk
    return ([None, sequences, kv_heads, d, v_d, n_new, nk, K_new, V_new, K, V] + ([None, None] if fp8 else [])
            + ([table, max_pages, page, num_pages] if cache == "paged" else []) + [k_lens, new_lens])


ENTRIES = [(c, f) for c in ("ragged", "paged") for f in (False, True)]
ENTRY_IDS = ["ragged", "ragged_fp8", "paged", "paged_fp8"]


def _call(cache, fp8, **kw):
    L = _lib.lib()
    st = getattr(L, _lib.append_entry_point(cache, fp8))(*_c_args(cache, fp8, **kw))
    return st, L.fa_last_error().decode()


@pytest.mark.parametrize("cache,fp8", ENTRIES, ids=ENTRY_IDS)
def test_c_sizes(cache, fp8):
    for kw in (dict(sequences=-1), dict(n_new=-1)):
        st, msg = _call(cache, fp8, **kw)
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and "must not be negative" in msg and cache + " append" in msg
    for kw in (dict(kv_heads=0), dict(d=0), dict(v_d=0), dict(nk=0, max_pages=1, page=64), dict(d=-3), dict(kv_heads=-1)):
        st, msg = _call(cache, fp8, **kw)
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and "must be >= 1" in msg, (kw, msg)


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_c_paged_arguments_and_envelope(fp8):
    for kw, text in ((dict(page=0, nk=128), "page must be >= 1"), (dict(page=-64, nk=128), "page must be >= 1"),
                     (dict(max_pages=0, nk=128), "max_pages must be >= 1"),
                     (dict(max_pages=2, page=64, nk=192), "max_pages * page = 128 is not the capacity nk = 192"),
                     (dict(num_pages=0), "num_pages must be >= 1")):
        st, msg = _call("paged", fp8, **kw)
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and text in msg, (kw, msg)
    for page in (32, 96, 1, 65):
        st, msg = _call("paged", fp8, page=page)
        assert st == _lib.FA_ERR_UNSUPPORTED and "page % 64 == 0" in msg and "got page = " + str(page) in msg
    # the envelope is checked before the empty call returns, the argument errors before the envelope
    assert _call("paged", fp8, page=32, sequences=0)[0] == _lib.FA_ERR_UNSUPPORTED
    assert _call("paged", fp8, page=32, num_pages=0)[0] == _lib.FA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("cache,fp8", ENTRIES, ids=ENTRY_IDS)
def test_c_null_pointers_where_there_is_work(cache, fp8):
    nulls = [("K_new", "null K_new or V_new"), ("V_new", "null K_new or V_new"),
             ("K", "null K_pool or V_pool" if cache == "paged" else "null K or V"),
             ("V", "null K_pool or V_pool" if cache == "paged" else "null K or V"), ("k_lens", "null k_lens")]
    if cache == "paged":
        nulls.append(("table", "null block_table"))
    for name, text in nulls:
        st, msg = _call(cache, fp8, **{name: None})
        assert st == _lib.FA_ERR_INVALID_ARGUMENT and text in msg, (name, msg)
    # without work nothing is launched and nothing is read: every pointer may be null
    allnull = dict(K_new=None, V_new=None, K=None, V=None, table=None, k_lens=None)
    assert _call(cache, fp8, sequences=0, **allnull)[0] == _lib.FA_OK
    assert _call(cache, fp8, n_new=0, **allnull)[0] == _lib.FA_OK


@pytest.mark.parametrize("cache,fp8", ENTRIES, ids=ENTRY_IDS)
def test_c_a_grid_that_does_not_fit_is_unsupported(cache, fp8):
    """sequences * kv_heads * ceil((d + v_d) * ((n_new + 14) / 8) / 256) blocks must fit 2^31 - 1: checked on the host."""
    for kw in (dict(sequences=2 ** 31), dict(sequences=2 ** 62, kv_heads=4), dict(sequences=2 ** 30, kv_heads=2),
               dict(sequences=2 ** 20, kv_heads=8, d=128, v_d=128, n_new=2048, max_pages=32),
               dict(sequences=1, kv_heads=1, d=2 ** 30, v_d=2 ** 30, n_new=2 ** 30, max_pages=2 ** 24)):
        st, msg = _call(cache, fp8, **kw)
        assert st == _lib.FA_ERR_UNSUPPORTED and "do not fit one launch" in msg, (kw, st, msg)
    assert ctypes.sizeof(ctypes.c_int64) == 8
