"""CPU tests of the host side of the FP8 latent pool and of the latent pool's fused append: the new
names and refusals, each raised before any device call, and the FP8 forward under the fp16 plan and workspace."""

import pytest
import torch

import tf_flash_attention_amd as pkg
from tests import test_mla_api as api
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

FP8, BAD_ARG = torch.uint8, fa.InvalidArgumentError


def _new(n_new=2, batch=(3,), c=576):
    return torch.zeros(batch + (c, n_new), dtype=torch.float16)


@pytest.mark.parametrize("kv_scale,pool_dtype,error,match", [
    (torch.ones(1), torch.float16, BAD_ARG, "a float16 pool takes no scale"),
    (torch.ones(1, dtype=torch.float64), FP8, TypeError, "kv_scale must be a float32 tensor"),
    (0.5, FP8, TypeError, "kv_scale must be a float32 tensor"),
    (torch.ones(2), FP8, BAD_ARG, "kv_scale should hold one element"),
    (torch.ones(1, device="meta"), FP8, BAD_ARG, "kv_scale must be on the device"),
    (None, FP8, BAD_ARG, "no CPU kernel")])  # (a valid FP8 call gets as far as the device check)
def test_refusals_of_kv_scale(kv_scale, pool_dtype, error, match):
    q, pool, table, lens = api._args()
    with pytest.raises(error, match=match):
        fa.mla_paged_1d(q, pool.to(pool_dtype), table, lens, 512, kv_scale=kv_scale)
    with pytest.raises(error, match=match):
        fa.mla_paged_append_1d(pool.to(pool_dtype), _new(), table, lens, kv_scale=kv_scale)


@pytest.mark.parametrize("change,error,match", [
    (dict(KV_new=_new().float()), TypeError, "KV_new must be a float16 tensor"),
    (dict(KV_new=_new(c=512)), BAD_ARG, r"batch \+ \(C, Nnew\)"),
    (dict(KV_new=_new(batch=(2,))), BAD_ARG, "shape of block_table"),
    (dict(KV_new=_new(batch=(3, 1))), BAD_ARG, "shape of block_table"),
    (dict(KV_pool=torch.zeros(64, 576, dtype=torch.float16)), BAD_ARG, r"\[num_pages, channels, page\]"),
    (dict(new_lens=torch.ones(2, dtype=torch.int32)), BAD_ARG, "shape of new_lens"),
    (dict(KV_pool=torch.zeros(7, 576, 64)), TypeError, "float16 or an FP8 pool"),
    (dict(KV_pool=torch.zeros(7, 64, 576, dtype=torch.float16).transpose(1, 2)), BAD_ARG, "KV_pool must be contiguous"),
    (dict(KV_pool=torch.zeros(7, 576, 32, dtype=torch.float16)), NotImplementedError, "multiple of 64")], ids=str)
def test_refusals_of_the_append(change, error, match):
    _, pool, table, lens = api._args()
    with pytest.raises(error, match=match):
        fa.mla_paged_append_1d(**{**dict(KV_pool=pool, KV_new=_new(), block_table=table, k_lens=lens), **change})


def test_the_entry_points():
    L = _lib.lib()
    for name in ("fa_forward_mla_paged_fp8", "fa_append_mla_paged", "fa_append_mla_paged_fp8"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert pkg.mla_paged_append_1d is fa.mla_paged_append_1d and "mla_paged_append_1d" in pkg.__all__
    assert "mla_paged_append_1d" in fa.mla_paged_1d.__doc__
    assert L.fa_append_mla_paged(None, 3, 0, 2, 128, 0, 0, 0, 2, 64, 7, 0, 0) == api.INVALID
    assert "MLA paged append: kv_heads = 1, d = 0, v_d = 0" in _lib.last_error()
    assert L.fa_append_mla_paged_fp8(None, 3, 576, 2, 128, 0, 0, 0, 0, 2, 64, 7, 0, 0) == api.INVALID
    assert "null KV_new" in _lib.last_error()
    assert L.fa_append_paged(None, 3, 1, 576, 0, 2, 128, 0, 0, 0, 0, 0, 2, 64, 7, 0, 0) == api.INVALID  # (v_d = 0: theirs only)
    # the FP8 forward takes the fp16 forward's plan and workspace
    prob, hq = api._problem(), 16
    need = int(L.fa_forward_mla_paged_workspace_bytes(prob, hq, 64))
    call = lambda p, n: L.fa_forward_mla_paged_fp8(None, p, hq, 0, 0, 0, 64, 64, 9, 0, 0, 0.07, 0, 0, 0, 0, 1, n)  # noqa: E731
    assert call(prob, need - 1) == api.TOO_SMALL
    assert call(prob, need) == api.INVALID and "null Q" in _lib.last_error()  # (past the workspace check)
    assert call(api._problem(c=600), need) == api.UNSUPPORTED
