"""CPU tests of flash_attention.ragged_1d's argument checks: every error is raised before any
device call, so CPU tensors reach all of them.  The last check of the wrapper is the device check itself."""

import pytest
import torch

import tf_flash_attention_amd as pkg
from tf_flash_attention_amd import flash_attention as fa


def _qkv(batch=(3,), hq=8, hk=2, c=64, cv=64, nq=4, cap=96, dtype=torch.float16):
    mk = lambda *s: torch.zeros(s, dtype=dtype)  # noqa: E731
    return mk(*batch, hq, c, nq), mk(*batch, hk, c, cap), mk(*batch, hk, cv, cap)


def _lens(batch=(3,), dtype=torch.int32):
    return torch.ones(batch, dtype=dtype)


def test_exported():
    assert "ragged_1d" in fa.__all__ and "ragged_1d" in pkg.__all__ and pkg.ragged_1d is fa.ragged_1d


@pytest.mark.parametrize("kw,text", [
    (dict(hq=7), "multiple of the one of K and V"),
    (dict(hk=0), "multiple of the one of K and V"),
])
def test_heads_must_divide(kw, text):
    Q, K, V = _qkv(**kw)
    with pytest.raises(fa.InvalidArgumentError, match=text):
        fa.ragged_1d(Q, K, V, _lens())


def test_shape_errors_of_the_grouped_wrapper():
    Q, K, V = _qkv()
    with pytest.raises(fa.InvalidArgumentError, match="number of dimensions of Q, K, and V should be equal"):
        fa.ragged_1d(Q, K[0], V, _lens())
    with pytest.raises(fa.InvalidArgumentError, match="channel dimension of Q and K"):
        fa.ragged_1d(Q, K[:, :, :32], V, _lens())
    with pytest.raises(fa.InvalidArgumentError, match="sequence shape of K and V"):
        fa.ragged_1d(Q, K, V[..., :80], _lens())
    with pytest.raises(fa.InvalidArgumentError, match="batch shapes of K and V"):
        fa.ragged_1d(Q, K, V[:2], _lens())
    with pytest.raises(fa.InvalidArgumentError, match=">= 3"):
        fa.ragged_1d(Q[0, 0, 0], K[0, 0, 0], V[0, 0, 0], _lens(()))


def test_dtypes():
    with pytest.raises(TypeError, match="unsupported dtype"):
        fa.ragged_1d(*_qkv(dtype=torch.bfloat16), _lens())
    for dt in (torch.float32, torch.float64):
        with pytest.raises(TypeError, match="does not accept"):
            fa.ragged_1d(*_qkv(dtype=dt), _lens())
    Q, K, V = _qkv()
    with pytest.raises(TypeError, match="share one dtype"):
        fa.ragged_1d(Q, K.float(), V, _lens())
    with pytest.raises(TypeError, match="share one dtype"):
        fa.ragged_1d(Q, K, V.double(), _lens())


@pytest.mark.parametrize("bad", [torch.int64, torch.int16, torch.float32])
def test_k_lens_must_be_int32(bad):
    with pytest.raises(TypeError, match="int32"):
        fa.ragged_1d(*_qkv(), _lens(dtype=bad))


def test_k_lens_must_be_a_tensor():
    with pytest.raises(TypeError, match="int32"):
        fa.ragged_1d(*_qkv(), [1, 1, 1])


@pytest.mark.parametrize("batch,shape", [((3,), (3, 2)), ((3,), (2,)), ((3,), ()), ((2, 3), (6,)), ((), (1,))])
def test_k_lens_shape_is_the_batch_shape_without_the_heads(batch, shape):
    with pytest.raises(fa.InvalidArgumentError, match="shape of k_lens"):
        fa.ragged_1d(*_qkv(batch=batch), _lens(shape))


def test_k_lens_device():
    with pytest.raises(fa.InvalidArgumentError, match="device of Q, K and V"):
        fa.ragged_1d(*_qkv(), _lens().to("meta"))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_inference_only(which):
    ts = list(_qkv())
    ts[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        fa.ragged_1d(*ts, _lens())


@pytest.mark.parametrize("kw", [dict(c=129), dict(cv=136), dict(hq=8, hk=2, nq=33), dict(hq=2, hk=2, nq=129),
                                dict(nq=0), dict(cap=0)], ids=str)
def test_outside_the_envelope_is_not_implemented(kw):
    Q, K, V = _qkv(**kw)
    with pytest.raises(NotImplementedError, match="fused envelope"):
        fa.ragged_1d(Q, K, V, _lens())


@pytest.mark.parametrize("batch", [(3,), (2, 3), ()])
def test_the_device_check_comes_last(batch):
    """Well-formed CPU inputs inside the envelope, also under no_grad with an input that requires grad: the
    one remaining error is that there is no CPU kernel."""
    Q, K, V = _qkv(batch=batch)
    with pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.ragged_1d(Q, K, V, _lens(batch))
    Q.requires_grad_(True)
    with torch.no_grad(), pytest.raises(fa.InvalidArgumentError, match="no CPU kernel"):
        fa.ragged_1d(Q, K, V, _lens(batch), tail_causal=True, returning_l_m=True)
