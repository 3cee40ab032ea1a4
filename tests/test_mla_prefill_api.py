"""CPU tests of the query-blocked and tree-masked MLA forward's host side: the exported names, the
plan and workspace functions of fa_forward_mla_paged_prefill, and the refusals of the entry points and of
flash_attention.mla_paged_prefill_1d.  Every error is raised before any device call, so CPU tensors and null
pointers reach all of them; the last check of the wrapper is the device check itself."""

import ctypes

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

NAMES = ("fa_forward_mla_paged_prefill_plan", "fa_forward_mla_paged_prefill_workspace_bytes",
         "fa_forward_mla_paged_prefill", "fa_forward_mla_paged_prefill_fp8")
OK, INVALID, UNSUPPORTED, TOO_SMALL = (_lib.FA_OK, _lib.FA_ERR_INVALID_ARGUMENT, _lib.FA_ERR_UNSUPPORTED,
                                       _lib.FA_ERR_WORKSPACE_TOO_SMALL)


def _problem(hq=16, c=576, v=512, nq=40, cap=4096, seqs=3, dtype=_lib.F16):
    return _lib.make_problem(dtype, _lib.FULL, 1, _lib.NONE_FRONT, seqs * hq, (nq,), (cap,), c, v)


def _plan(prob, hq, page=64):
    out = (ctypes.c_int32 * 6)()
    return _lib.lib().fa_forward_mla_paged_prefill_plan(prob, hq, page, out), tuple(out)


def _forward(prob, hq, page=64, tail=1, mask=0, ws_bytes=None, ptr=0, fp8=False):
    """The entry point with every pointer ``ptr`` (null: no call here gets as far as a launch) and the mask ``mask``."""
    L = _lib.lib()
    need = int(L.fa_forward_mla_paged_prefill_workspace_bytes(prob, hq, page))
    head = (None, prob, hq, ptr, ptr, ptr, prob.k_seq[0] // page, page, 9, ptr, tail, 0.07)
    tail_ = (mask, ptr, ptr, ptr, 1 if ws_bytes is not None else ptr, need if ws_bytes is None else ws_bytes)
    return L.fa_forward_mla_paged_prefill_fp8(*head, ptr, *tail_) if fp8 else L.fa_forward_mla_paged_prefill(*head, *tail_)


def _args(batch=(3,), hq=16, c=576, nq=40, page=64, max_pages=2, num_pages=7, dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros(num_pages, c, page, dtype=dtype),
            torch.zeros(batch + (max_pages,), dtype=torch.int32), torch.ones(batch, dtype=torch.int32)]


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "mla_paged_prefill_1d" in fa.__all__ and "mla_paged_prefill_1d" in pkg.__all__
    assert pkg.mla_paged_prefill_1d is fa.mla_paged_prefill_1d


@pytest.mark.parametrize("hq,nq,cap,want", [(128, 5, 2624, (3, 1024, 1, 10, 5, 2)), (16, 33, 2624, (3, 1024, 4, 9, 9, 1)),
                                            (1, 70, 2624, (3, 1024, 64, 2, 2, 1)), (16, 128, 2624, (2, 1344, 4, 32, 32, 1)),
                                            (16, 2048, 16384, (1, 16384, 4, 512, 512, 1)), (3, 4, 4096, (8, 512, 16, 1, 1, 1))])
def test_the_plan_and_the_workspace_are_pure(hq, nq, cap, want):
    """{chunks, keys a chunk, P_b, row blocks, query blocks, head blocks}: P_b = max(1, 64 / next_pow2(Hq)), at most
    max(1, 64 / row blocks) chunks of at least 1024 keys (512 for one block); b changes neither, and the workspace is
    sequences * row blocks * chunks records of 64 * (v + 3) floats."""
    L = _lib.lib()
    for seqs in (1, 5):
        prob = _problem(hq=hq, nq=nq, cap=cap, seqs=seqs)
        assert _plan(prob, hq) == (OK, want)
        assert (L.fa_forward_mla_paged_prefill_workspace_bytes(prob, hq, 64)
                == -(-seqs * want[3] * want[0] * 64 * 515 * 4 // 256) * 256)


@pytest.mark.parametrize("kw,page", [(dict(c=600, v=512), 64), (dict(c=96, v=64), 64), (dict(c=320, v=384), 64),
                                     (dict(c=576, v=576), 64), (dict(c=576, v=96), 64), (dict(), 32),
                                     (dict(hq=129), 64), (dict(hq=128, nq=2 ** 15), 64), (dict(dtype=_lib.F32), 64)], ids=str)
def test_outside_the_envelope(kw, page):
    """C = 600, C = 96, v > C, v = 576, v = 96, page = 32, Hq = 129, Hq * Nq * v = 2^31, not fp16: 0 chunks, 0 bytes,
    FA_ERR_UNSUPPORTED before anything is read, from both entry points; NotImplementedError from the wrapper."""
    hq = kw.get("hq", 16)
    prob = _problem(cap=4096, **kw)
    st, plan = _plan(prob, hq, page)
    assert st == OK and plan[0] == 0
    assert _lib.lib().fa_forward_mla_paged_prefill_workspace_bytes(prob, hq, page) == 0
    for fp8 in (False, True):
        assert _forward(prob, hq, page, fp8=fp8) == UNSUPPORTED and "outside the envelope" in _lib.last_error()
    if "dtype" not in kw and kw.get("nq", 0) < 2 ** 15:  # (the wrapper's shapes are real tensors)
        shape = dict(hq=hq, c=kw.get("c", 576), page=page)
        with pytest.raises(NotImplementedError, match="page size|outside the envelope|v_channels <= C"):
            fa.mla_paged_prefill_1d(*_args(**shape), kw.get("v", 512))


def test_argument_errors_of_the_entry_points():
    prob, hq = _problem(), 16
    for fp8 in (False, True):
        assert _forward(prob, hq, tail=0, mask=64, fp8=fp8) == INVALID and "requires tail_causal" in _lib.last_error()
        assert _forward(_problem(nq=129), hq, mask=64, fp8=fp8) == INVALID and "at most 128 queries" in _lib.last_error()
        assert _forward(_problem(nq=129), hq, fp8=fp8) == TOO_SMALL  # (without a mask Nq is free)
        assert _forward(prob, 7, fp8=fp8) == INVALID and "multiple of heads" in _lib.last_error()
        assert _forward(prob, hq, page=192, fp8=fp8) == INVALID and "multiple of page" in _lib.last_error()
        assert _forward(prob, hq, ws_bytes=1000, fp8=fp8) == TOO_SMALL
        assert _forward(prob, hq, ws_bytes=2 ** 40, fp8=fp8) == INVALID and "null" in _lib.last_error()
        assert _forward(_problem(seqs=0), hq, ws_bytes=0, fp8=fp8) == OK  # b == 0: nothing launched
    # 2^22 sequences x 512 row blocks: the partial grid is 2^31 workgroups
    assert _forward(_problem(nq=2048, seqs=2 ** 22), hq, ws_bytes=2 ** 62) == INVALID and "launch grid" in _lib.last_error()


def test_argument_errors_of_the_wrapper():
    a = _args()
    mask = torch.zeros(3, 40, 2, dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="draft_mask requires tail_causal=True"):
        fa.mla_paged_prefill_1d(*a, 512, draft_mask=mask)
    with pytest.raises(TypeError, match="draft_mask must be an int32 tensor"):
        fa.mla_paged_prefill_1d(*a, 512, tail_causal=True, draft_mask=mask.long())
    with pytest.raises(fa.InvalidArgumentError, match="shape of draft_mask"):
        fa.mla_paged_prefill_1d(*a, 512, tail_causal=True, draft_mask=mask[:, :, :1])
    with pytest.raises(fa.InvalidArgumentError, match="draft_mask must be on the device of Q"):
        fa.mla_paged_prefill_1d(*a, 512, tail_causal=True, draft_mask=mask.to("meta"))
    with pytest.raises(NotImplementedError, match="at most 128 draft tokens"):
        fa.mla_paged_prefill_1d(*_args(nq=129), 512, tail_causal=True, draft_mask=torch.zeros(3, 129, 5, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="page size"):
        fa.mla_paged_prefill_1d(*_args(page=32), 512)
    with pytest.raises(NotImplementedError, match="outside the envelope"):
        fa.mla_paged_prefill_1d(*_args(hq=129), 512)
    with pytest.raises(fa.InvalidArgumentError, match="kv_scale was given"):
        fa.mla_paged_prefill_1d(*a, 512, kv_scale=torch.ones(1))
    a[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="mla_paged_prefill_1d is inference only"):
        fa.mla_paged_prefill_1d(*a, 512)


@pytest.mark.parametrize("nq", [2, 40])
def test_the_device_check_comes_last(nq):
    """Delegated to mla_paged_1d (Hq * next_pow2(Nq) <= 512, no mask) and not."""
    a = _args(nq=nq, page=192)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.mla_paged_prefill_1d(*a, 256, tail_causal=True, returning_l_m=True)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.mla_paged_prefill_1d(*a, 256, tail_causal=True, draft_mask=torch.zeros(3, nq, (nq + 31) // 32, dtype=torch.int32))
