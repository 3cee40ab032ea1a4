"""CPU tests of the grouped-query wrappers' argument checks (flash_attention.grouped_1d / grouped_2d /
attention_forward_grouped): every check here runs before any device work, so CPU tensors reach it."""

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import flash_attention as fa


def _t(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_public_names():
    for name in ("grouped_1d", "grouped_2d", "attention_forward_grouped"):
        assert getattr(pkg, name) is getattr(fa, name)
        assert name in pkg.__all__ and name in fa.__all__


# ------------------------------------------------------------------ shapes
def test_shapes_are_extracted():
    out = fa.verify_grouped_shapes(1, (3, 8, 64, 5), (3, 2, 64, 77), (3, 2, 48, 77))
    assert out == ((3, 8), (5,), 64, (3, 2), (77,), 48, 4)
    out = fa.verify_grouped_shapes(2, (8, 64, 2, 4), (8, 64, 40, 66), (8, 32, 40, 66))
    assert out == ((8,), (2, 4), 64, (8,), (40, 66), 32, 1)
    # MQA: every query head shares one K/V head
    assert fa.verify_grouped_shapes(1, (2, 16, 64, 1), (2, 1, 64, 9), (2, 1, 64, 9))[-1] == 16


@pytest.mark.parametrize("f", [fa.grouped_1d, lambda *a: fa.attention_forward_grouped("full", 1, *a, "none_front")])
def test_unequal_ranks(f):
    with pytest.raises(fa.InvalidArgumentError, match="The number of dimensions of Q, K, and V should be equal"):
        f(_t(2, 8, 64, 5), _t(8, 64, 7), _t(8, 64, 7))


def test_rank_too_small():
    with pytest.raises(fa.InvalidArgumentError, match="should be >= 4"):
        fa.grouped_2d(_t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 7))


def test_batch_shapes_differ_outside_the_last_axis():
    with pytest.raises(fa.InvalidArgumentError) as e:
        fa.grouped_1d(_t(3, 8, 64, 5), _t(2, 2, 64, 7), _t(2, 2, 64, 7))
    msg = str(e.value)
    assert "except in its last axis" in msg
    assert "Q_batch_shape = [3,8], K_batch_shape = [2,2], V_batch_shape = [2,2]" in msg


def test_k_and_v_batch_shapes_differ():
    with pytest.raises(fa.InvalidArgumentError, match="K_batch_shape = \\[3,2\\], V_batch_shape = \\[3,4\\]"):
        fa.grouped_1d(_t(3, 8, 64, 5), _t(3, 2, 64, 7), _t(3, 4, 64, 7))


@pytest.mark.parametrize("hq,hk", [(8, 3), (2, 4), (7, 2)])
def test_heads_are_not_a_multiple(hq, hk):
    with pytest.raises(fa.InvalidArgumentError) as e:
        fa.grouped_1d(_t(3, hq, 64, 5), _t(3, hk, 64, 7), _t(3, hk, 64, 7))
    msg = str(e.value)
    assert "should be a multiple" in msg
    assert f"Q_batch_shape = [3,{hq}], K_batch_shape = [3,{hk}]" in msg


def test_channel_and_sequence_mismatches_keep_the_existing_texts():
    with pytest.raises(fa.InvalidArgumentError, match="The channel dimension of Q and K should be equal"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 32, 7), _t(2, 64, 7))
    with pytest.raises(fa.InvalidArgumentError, match="The sequence shape of K and V are expected to be equal"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 9))


def test_unknown_policy_and_sync_mode():
    with pytest.raises(fa.InvalidArgumentError, match="Unsupported policy: banded"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 7), policy="banded")
    with pytest.raises(fa.InvalidArgumentError, match="Unsupported sync_mode: middle"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 7), sync_mode="middle")


# ------------------------------------------------------------------ dtypes (the existing checks), device
def test_dtype_checks():
    with pytest.raises(TypeError, match="unsupported dtype"):
        fa.grouped_1d(_t(8, 64, 5, dtype=torch.bfloat16), _t(2, 64, 7, dtype=torch.bfloat16),
                      _t(2, 64, 7, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="Q, K and V must share one dtype"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 64, 7, dtype=torch.float32), _t(2, 64, 7))
    with pytest.raises(TypeError, match="Q, K and V must share one dtype"):
        fa.attention_forward_grouped("causal", 1, _t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 7, dtype=torch.float64),
                                     "scale_end")


def test_cpu_tensors_are_rejected_after_the_shape_and_dtype_checks():
    with pytest.raises(fa.InvalidArgumentError, match="there is no CPU kernel"):
        fa.grouped_1d(_t(8, 64, 5), _t(2, 64, 7), _t(2, 64, 7))
    with pytest.raises(fa.InvalidArgumentError, match="there is no CPU kernel"):  # g = 1: the ungrouped wrapper
        fa.grouped_1d(_t(2, 64, 5), _t(2, 64, 7), _t(2, 64, 7))


# ------------------------------------------------------------------ the existing wrappers keep their check
EXISTING = [
    lambda q, k, v: fa.full_1d(q, k, v),
    lambda q, k, v: fa.causal_1d(q, k, v, "scale_end"),
    lambda q, k, v: fa.local_1d(q, k, v, 3, 0, False, "none_front"),
    lambda q, k, v: fa.full_2d(q[..., None], k[..., None], v[..., None]),
    lambda q, k, v: fa.causal_2d(q[..., None], k[..., None], v[..., None], "scale_end"),
    lambda q, k, v: fa.local_2d(q[..., None], k[..., None], v[..., None], 3, 0, False, "none_front"),
    lambda q, k, v: fa.combined_1d(q, [fa.Part("full", k, v)]),
    lambda q, k, v: fa.combined_2d(q[..., None], [fa.Part("full", k[..., None], v[..., None])]),
]


@pytest.mark.parametrize("i", range(len(EXISTING)))
def test_existing_wrappers_still_reject_unequal_batch_shapes(i):
    with pytest.raises(fa.InvalidArgumentError) as e:
        EXISTING[i](_t(3, 8, 64, 5), _t(3, 2, 64, 7), _t(3, 2, 64, 7))
    assert str(e.value) == ("The batch shape of all inputs should be equal, but Q_batch_shape = [3,8], "
                            "K_batch_shape = [3,2], V_batch_shape = [3,2] were received")
