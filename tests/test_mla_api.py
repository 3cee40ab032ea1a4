"""CPU tests of MLA decode's host side: the exported names, the plan and workspace functions of
fa_forward_mla_paged, and every refusal and argument error of the C entry points and of flash_attention.mla_paged_1d.
Every error is raised before any device call, so CPU tensors and null pointers reach all of them; the last check of
the wrapper is the device check itself."""

import ctypes

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

NAMES = ("fa_forward_mla_paged_plan", "fa_forward_mla_paged_workspace_bytes", "fa_forward_mla_paged")
OK, INVALID, UNSUPPORTED, TOO_SMALL = (_lib.FA_OK, _lib.FA_ERR_INVALID_ARGUMENT, _lib.FA_ERR_UNSUPPORTED,
                                       _lib.FA_ERR_WORKSPACE_TOO_SMALL)


def _problem(hq=16, c=576, v=512, nq=1, cap=4096, seqs=3, dtype=_lib.F16):
    return _lib.make_problem(dtype, _lib.FULL, 1, _lib.NONE_FRONT, seqs * hq, (nq,), (cap,), c, v)


def _plan(prob, hq, page=64):
    out = (ctypes.c_int32 * 5)()
    return _lib.lib().fa_forward_mla_paged_plan(prob, hq, page, out), tuple(out)


def _forward(prob, hq, page=64, max_pages=None, scale=0.07, ws_bytes=None, ptr=0):
    """fa_forward_mla_paged with every pointer ``ptr`` (null: no call here gets as far as a launch)."""
    L = _lib.lib()
    need = int(L.fa_forward_mla_paged_workspace_bytes(prob, hq, page))
    max_pages = prob.k_seq[0] // page if max_pages is None else max_pages
    return L.fa_forward_mla_paged(None, prob, hq, ptr, ptr, ptr, max_pages, page, 9, ptr, 0, scale, ptr, ptr, ptr,
                                  1 if ws_bytes is not None else ptr, need if ws_bytes is None else ws_bytes)


def _args(batch=(3,), hq=16, c=576, nq=1, page=64, max_pages=2, num_pages=7, dtype=torch.float16):
    return [torch.zeros(batch + (hq, c, nq), dtype=dtype), torch.zeros(num_pages, c, page, dtype=dtype),
            torch.zeros(batch + (max_pages,), dtype=torch.int32), torch.ones(batch, dtype=torch.int32)]


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "MLA paged latent decode" in _lib.lib().fa_build_info().decode()
    assert "mla_paged_1d" in fa.__all__ and "mla_paged_1d" in pkg.__all__ and pkg.mla_paged_1d is fa.mla_paged_1d
    doc = fa.mla_paged_1d.__doc__
    assert "KV_pool[block_table[s, pos // page], :, pos % page] = new" in doc and "FIXED in a captured graph" in doc


@pytest.mark.parametrize("hq,nq,cap,want", [(16, 1, 4096, (8, 512, 1, 16, 1)), (128, 1, 4096, (4, 1024, 1, 128, 2)),
                                            (65, 1, 2624, (3, 1024, 1, 65, 2)), (16, 3, 2624, (6, 512, 4, 64, 1)),
                                            (128, 4, 2 ** 20, (64, 16384, 4, 512, 8)), (1, 1, 64, (1, 512, 1, 1, 1))])
def test_the_plan_and_the_workspace_are_pure(hq, nq, cap, want):
    """The ragged plan's chunk formula over the capacity, the fold and the row blocks; b changes neither, and the
    workspace is the plan's records times the sequences."""
    L = _lib.lib()
    for seqs in (1, 5):
        prob = _problem(hq=hq, nq=nq, cap=cap, seqs=seqs)
        assert _plan(prob, hq) == (OK, want)
        assert L.fa_forward_mla_paged_workspace_bytes(prob, hq, 64) == -(-seqs * want[4] * want[0] * 64 * 515 * 4 // 256) * 256


@pytest.mark.parametrize("kw,page", [(dict(c=600, v=512), 64), (dict(c=96, v=64), 64), (dict(c=320, v=384), 64),
                                     (dict(c=576, v=576), 64), (dict(c=576, v=96), 64), (dict(), 32),
                                     (dict(hq=129), 64), (dict(hq=128, nq=5), 64), (dict(dtype=_lib.F32), 64)], ids=str)
def test_outside_the_envelope(kw, page):
    """C = 600, C = 96, v > C, v = 576, v = 96, page = 32, Hq = 129, R = 1024, not fp16: 0 chunks, 0 bytes,
    FA_ERR_UNSUPPORTED before anything is read."""
    hq = kw.get("hq", 16)
    prob = _problem(cap=4096, **kw)
    st, plan = _plan(prob, hq, page)
    assert st == OK and plan[0] == 0
    assert _lib.lib().fa_forward_mla_paged_workspace_bytes(prob, hq, page) == 0
    assert _forward(prob, hq, page) == UNSUPPORTED and "outside the envelope" in _lib.last_error()
    shape = dict(hq=hq, c=kw.get("c", 576), nq=kw.get("nq", 1), page=page)
    if "dtype" not in kw:
        with pytest.raises(NotImplementedError, match="page size|outside the envelope|v_channels <= C"):
            fa.mla_paged_1d(*_args(**shape), kw.get("v", 512))


def test_argument_errors_of_the_entry_points():
    prob, hq = _problem(), 16
    assert _forward(prob, hq, scale=0.0) == INVALID and "softmax_scale" in _lib.last_error()
    assert _forward(prob, hq, scale=-1.0) == INVALID
    assert _forward(prob, hq, scale=float("inf")) == INVALID
    assert _forward(prob, hq, scale=float("nan")) == INVALID
    assert _forward(prob, 0) == INVALID and _plan(prob, 0)[0] == INVALID
    assert _forward(prob, 7) == INVALID and "multiple of heads" in _lib.last_error()
    assert _forward(prob, hq, page=0, max_pages=1) == INVALID
    assert _forward(prob, hq, page=192) == INVALID and "multiple of page" in _lib.last_error()
    assert _forward(prob, hq, max_pages=63) == INVALID and "is not the capacity" in _lib.last_error()
    assert _forward(prob, hq, ws_bytes=1000) == TOO_SMALL
    assert _forward(prob, hq) == TOO_SMALL  # (a null workspace)
    assert _forward(prob, hq, ws_bytes=2 ** 40) == INVALID and "null" in _lib.last_error()  # b > 0: null pointers
    assert _forward(_problem(seqs=0), hq, ws_bytes=0) == OK  # b == 0: nothing launched


def test_argument_errors_of_the_wrapper():
    a = _args()
    with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, channels, page\]"):
        fa.mla_paged_1d(a[0], a[1][None], a[2], a[3], 512)
    with pytest.raises(fa.InvalidArgumentError, match=r"batch \+ \(Hq, C, Nq\)"):
        fa.mla_paged_1d(a[0][0, 0], a[1], a[2], a[3], 512)
    with pytest.raises(fa.InvalidArgumentError, match="channels of Q and KV_pool"):
        fa.mla_paged_1d(a[0][:, :, :64], a[1], a[2], a[3], 64)
    with pytest.raises(fa.InvalidArgumentError, match="v_channels must be a positive int"):
        fa.mla_paged_1d(*a, 0)
    with pytest.raises(TypeError, match="unsupported dtype"):
        fa.mla_paged_1d(*_args(dtype=torch.bfloat16), 512)
    with pytest.raises(TypeError, match="share one dtype"):
        fa.mla_paged_1d(a[0], a[1].float(), a[2], a[3], 512)
    with pytest.raises(TypeError, match="block_table must be an int32 tensor"):
        fa.mla_paged_1d(a[0], a[1], a[2].long(), a[3], 512)
    with pytest.raises(TypeError, match="k_lens must be an int32 tensor"):
        fa.mla_paged_1d(a[0], a[1], a[2], a[3].tolist(), 512)
    with pytest.raises(fa.InvalidArgumentError, match="shape of block_table"):
        fa.mla_paged_1d(a[0], a[1], a[2][:2], a[3], 512)
    with pytest.raises(fa.InvalidArgumentError, match="shape of k_lens"):
        fa.mla_paged_1d(a[0], a[1], a[2], a[3][:2], 512)
    with pytest.raises(fa.InvalidArgumentError, match="on the device of Q and KV_pool"):
        fa.mla_paged_1d(a[0], a[1], a[2].to("meta"), a[3], 512)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(fa.InvalidArgumentError, match="softmax_scale must be positive and finite"):
            fa.mla_paged_1d(*a, 512, softmax_scale=bad)
    a[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        fa.mla_paged_1d(*a, 512)


@pytest.mark.parametrize("batch", [(3,), (2, 3), ()])
def test_the_device_check_comes_last(batch):
    a = _args(batch=batch, page=192)
    a[0].requires_grad_(True)
    with torch.no_grad(), pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.mla_paged_1d(*a, 256, tail_causal=True, softmax_scale=192 ** -0.5, returning_l_m=True)
