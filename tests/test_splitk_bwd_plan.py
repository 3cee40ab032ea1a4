"""CPU tests of the split-key backward's routing rule (include/fa_api.h: fa_backward_split_plan,
fa_backward_split_workspace_bytes).  Host-only: no device work.

The backward plan is the forward's (same chunks, same key range) wherever a slice's K / V channel rows
stay inside the dQ kernel's 32-bit buffer offsets, and 0 chunks elsewhere."""

import ctypes

import pytest

from tests.test_splitk_plan import NOT_SPLITTING, SPLITTING, _nelems, _prob
from tf_flash_attention_amd import _lib


def _plan(p, which="backward"):
    out = (ctypes.c_int32 * 4)()
    fn = _lib.lib().fa_backward_split_plan if which == "backward" else _lib.lib().fa_forward_split_plan
    assert fn(p, out) == _lib.FA_OK
    return tuple(out)


def _split_bytes(p):
    return int(_lib.lib().fa_backward_split_workspace_bytes(p))


def _plain_bytes(p):
    return int(_lib.lib().fa_backward_workspace_bytes(p))


@pytest.mark.parametrize("kw", SPLITTING, ids=lambda k: f"{k['policy']}-{len(k['qs'])}d")
def test_backward_plan_is_the_forward_plan(kw):
    p = _prob(**kw)
    assert _plan(p, "forward")[0] >= 2
    assert _plan(p) == _plan(p, "forward")


@pytest.mark.parametrize("name", sorted(NOT_SPLITTING))
def test_envelope_edges_do_not_split(name):
    p = _prob(**NOT_SPLITTING[name])
    assert _plan(p)[0] == 0
    assert _split_bytes(p) == _plain_bytes(p)


def test_key_rows_past_the_32_bit_offsets_do_not_split():
    """fp16, d = v_d = 128, nq = 32, nk = 2^24: the K row set of one slice is 2^32 bytes.  The forward
    still splits (it addresses K and V with 64-bit pointers); the dQ kernel cannot take the shape."""
    kw = dict(policy="full", qs=(32,), ks=(1 << 24,), d=128)
    p = _prob(**kw)
    assert _plan(p, "forward")[0] >= 2
    assert _plan(p)[0] == 0
    assert _split_bytes(p) == _plain_bytes(p)
    # the condition is max(d, v_d) * (nk + 8) * 2 < 2^31: one channel set below it splits again
    edge = (1 << 31) // (2 * 128) - 8
    assert _plan(_prob(**dict(kw, ks=(edge - 1,))))[0] >= 2
    assert _plan(_prob(**dict(kw, ks=(edge,))))[0] == 0
    assert _plan(_prob(**dict(kw, ks=(edge - 1,), d=64, vd=128)))[0] >= 2
    assert _plan(_prob(**dict(kw, ks=(edge,), d=64, vd=128)))[0] == 0


@pytest.mark.parametrize("kw", SPLITTING + [NOT_SPLITTING["local256"], NOT_SPLITTING["nk2047"]],
                         ids=lambda k: "-".join(map(str, k.values())))
def test_plan_and_per_slice_workspace_do_not_depend_on_batch(kw):
    plans = {_plan(_prob(**dict(kw, b=b))) for b in (1, 5, 4096)}
    assert len(plans) == 1
    chunks = plans.pop()[0]
    p1 = _prob(**dict(kw, b=1))
    per_slice = chunks * p1.d * _nelems(kw["qs"]) * 4
    for b in (1, 5, 4096):
        p = _prob(**dict(kw, b=b))
        extra = _split_bytes(p) - _plain_bytes(p)
        assert b * per_slice <= extra < b * per_slice + 256


@pytest.mark.parametrize("kw", SPLITTING + list(NOT_SPLITTING.values()), ids=lambda k: "-".join(map(str, k.values())))
def test_workspace_formula(kw):
    """Outside the envelope fa_backward's workspace; inside it that plus b * chunks * d * nq floats rounded
    up to the 256-byte granularity of the other regions."""
    for b in (1, 5, 4096):
        p = _prob(**dict(kw, b=b))
        chunks = _plan(p)[0]
        if chunks == 0:
            assert _split_bytes(p) == _plain_bytes(p)
        else:
            part = b * chunks * p.d * _nelems(kw["qs"]) * 4
            assert _split_bytes(p) == _plain_bytes(p) + (part + 255) // 256 * 256


def test_unequal_channels_size_the_partials_by_d():
    p = _prob(policy="full", qs=(33,), ks=(2600,), d=96, vd=40, b=3)
    chunks = _plan(p)[0]
    assert chunks == 6
    part = 3 * chunks * 96 * 33 * 4
    assert _split_bytes(p) == _plain_bytes(p) + (part + 255) // 256 * 256


def test_invalid_problem_is_rejected():
    p = _prob()
    p.seq_dims = 3
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_backward_split_plan(p, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert _split_bytes(p) == 0
