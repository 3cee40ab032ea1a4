"""CPU tests of flash_attention.paged_1d's argument checks: every error is raised before any
device call, so CPU tensors reach all of them.  The last check of the wrapper is the device check itself."""

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import flash_attention as fa


def _args(batch=(3,), hq=8, hk=2, c=64, cv=64, nq=4, page=64, max_pages=2, num_pages=7, dtype=torch.float16):
    mk = lambda *s: torch.zeros(s, dtype=dtype)  # noqa: E731
    return [mk(*batch, hq, c, nq), mk(num_pages, hk, c, page), mk(num_pages, hk, cv, page),
            torch.zeros(batch + (max_pages,), dtype=torch.int32), torch.ones(batch, dtype=torch.int32)]


def test_exported():
    assert "paged_1d" in fa.__all__ and "paged_1d" in pkg.__all__ and pkg.paged_1d is fa.paged_1d


def test_the_docstring_gives_the_append_recipe():
    assert "K_pool[block_table[s, pos // page], :, :, pos % page] = new" in fa.paged_1d.__doc__


def test_pools_are_four_dimensional_and_agree():
    a = _args()
    with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, Hk, channels, page\]"):
        fa.paged_1d(a[0], a[1][0], a[2], a[3], a[4])
    with pytest.raises(fa.InvalidArgumentError, match=r"\[num_pages, Hk, channels, page\]"):
        fa.paged_1d(a[0], a[1], a[2][None], a[3], a[4])
    for bad in (a[2][:5], a[2][:, :1], a[2][..., :32]):
        with pytest.raises(fa.InvalidArgumentError, match="agree in num_pages, Hk and page"):
            fa.paged_1d(a[0], a[1], bad, a[3], a[4])


def test_q_shape_channels_and_heads():
    a = _args()
    with pytest.raises(fa.InvalidArgumentError, match=r"batch \+ \(Hq, C, Nq\)"):
        fa.paged_1d(a[0][0, 0], *a[1:])
    with pytest.raises(fa.InvalidArgumentError, match="channels of Q and K_pool"):
        fa.paged_1d(a[0][:, :, :32], *a[1:])
    with pytest.raises(fa.InvalidArgumentError, match="multiple of the heads of a page"):
        fa.paged_1d(*_args(hq=7))
    with pytest.raises(fa.InvalidArgumentError, match="multiple of the heads of a page"):
        fa.paged_1d(*_args(hk=0))
    with pytest.raises(fa.InvalidArgumentError, match="should hold a page"):
        fa.paged_1d(*_args(num_pages=0))


def test_dtypes():
    with pytest.raises(TypeError, match="unsupported dtype"):
        fa.paged_1d(*_args(dtype=torch.bfloat16))
    for dt in (torch.float32, torch.float64):
        with pytest.raises(TypeError, match="does not accept"):
            fa.paged_1d(*_args(dtype=dt))
    a = _args()
    with pytest.raises(TypeError, match="share one dtype"):
        fa.paged_1d(a[0], a[1].float(), a[2], a[3], a[4])
    with pytest.raises(TypeError, match="share one dtype"):
        fa.paged_1d(a[0], a[1], a[2].double(), a[3], a[4])


@pytest.mark.parametrize("which,name", [(3, "block_table"), (4, "k_lens")])
@pytest.mark.parametrize("bad", [torch.int64, torch.int16, torch.float32])
def test_table_and_lengths_must_be_int32_tensors(which, name, bad):
    a = _args()
    a[which] = a[which].to(bad)
    with pytest.raises(TypeError, match=name + " must be an int32 tensor"):
        fa.paged_1d(*a)
    a[which] = a[which].tolist()
    with pytest.raises(TypeError, match=name + " must be an int32 tensor"):
        fa.paged_1d(*a)


@pytest.mark.parametrize("batch,shape", [((3,), (3,)), ((3,), (2, 2)), ((3,), (3, 2, 2)), ((2, 3), (6, 2)), ((), (1, 2)),
                                         ((3,), (3, 0))])
def test_block_table_shape_is_the_batch_shape_plus_max_pages(batch, shape):
    a = _args(batch=batch)
    a[3] = torch.zeros(shape, dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="shape of block_table"):
        fa.paged_1d(*a)


@pytest.mark.parametrize("batch,shape", [((3,), (3, 2)), ((3,), (2,)), ((3,), ()), ((2, 3), (6,)), ((), (1,))])
def test_k_lens_shape_is_the_batch_shape(batch, shape):
    a = _args(batch=batch)
    a[4] = torch.ones(shape, dtype=torch.int32)
    with pytest.raises(fa.InvalidArgumentError, match="shape of k_lens"):
        fa.paged_1d(*a)


@pytest.mark.parametrize("which", [3, 4])
def test_table_and_lengths_device(which):
    a = _args()
    a[which] = a[which].to("meta")
    with pytest.raises(fa.InvalidArgumentError, match="on the device of Q, K_pool and V_pool"):
        fa.paged_1d(*a)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_inference_only(which):
    a = _args()
    a[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        fa.paged_1d(*a)


@pytest.mark.parametrize("page", [32, 16, 96, 1])
def test_a_small_page_is_not_implemented_and_the_text_names_the_condition(page):
    with pytest.raises(NotImplementedError, match="page size .* must be a multiple of 64 keys, got page = " + str(page)):
        fa.paged_1d(*_args(page=page))


@pytest.mark.parametrize("kw", [dict(c=129), dict(cv=136), dict(hq=8, hk=2, nq=33), dict(hq=2, hk=2, nq=129),
                                dict(nq=0)], ids=str)
def test_outside_the_ragged_envelope_is_not_implemented(kw):
    with pytest.raises(NotImplementedError, match="fused envelope"):
        fa.paged_1d(*_args(**kw))


@pytest.mark.parametrize("batch", [(3,), (2, 3), ()])
@pytest.mark.parametrize("page", [64, 192])
def test_the_device_check_comes_last(batch, page):
    """Well-formed CPU inputs inside the envelope, also under no_grad with an input that requires grad: the
    one remaining error is that there is no CPU kernel."""
    a = _args(batch=batch, page=page)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.paged_1d(*a)
    a[0].requires_grad_(True)
    with torch.no_grad(), pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.paged_1d(*a, tail_causal=True, returning_l_m=True)
