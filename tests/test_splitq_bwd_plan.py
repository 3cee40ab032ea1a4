"""CPU tests of the split-query backward's routing rule (include/fa_api.h: fa_backward_split_q_plan,
fa_backward_split_workspace_bytes).  Host-only: no device work.

The plan cuts the dK/dV pass of an fp16 backward with one key block (nk <= 128), max(d, v_d) <= 128 and a
query range of at least 2048 queries into chunks of max(min_chunk, ceil(ceil(span / 64) / 128) * 128)
queries (min_chunk 512 for nk <= 64, 1024 above), independent of b; it is never active together with the
key-chunk plan of the dQ pass (fa_backward_split_plan)."""

import ctypes
import itertools

import pytest

from tests.test_splitk_plan import SPLITTING as FEW_QUERY_SHAPES
from tests.test_splitk_plan import _nelems, _prob
from tf_flash_attention_amd import _lib


def _qplan(p):
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_backward_split_q_plan(p, out) == _lib.FA_OK
    return tuple(out)


def _kplan(p, which="backward"):
    out = (ctypes.c_int32 * 4)()
    fn = _lib.lib().fa_backward_split_plan if which == "backward" else _lib.lib().fa_forward_split_plan
    assert fn(p, out) == _lib.FA_OK
    return tuple(out)


def _split_bytes(p):
    return int(_lib.lib().fa_backward_split_workspace_bytes(p))


def _plain_bytes(p):
    return int(_lib.lib().fa_backward_workspace_bytes(p))


def _part_bytes(b, chunks, d, vd, nk):
    return (b * chunks * (d + vd) * nk * 4 + 255) // 256 * 256


SPLITTING = [
    dict(policy="full", qs=(2048,), ks=(1,)),
    dict(policy="full", qs=(16384,), ks=(77,)),
    dict(policy="full", qs=(16384,), ks=(128,), d=128),
    dict(policy="full", qs=(2600,), ks=(33,), d=96, vd=40),
    dict(policy="causal", qs=(4101,), ks=(33,), mode="scale_front"),
    dict(policy="causal", qs=(4200,), ks=(128,), mode="scale_end", d=128),
    dict(policy="causal", qs=(2603,), ks=(33,), mode="scale_end"),
    dict(policy="local", qs=(4101,), ks=(128,), ws=3000),
    dict(policy="local", qs=(4101,), ks=(128,), ws=40, mode="scale_end", causal=True),
    dict(policy="local", qs=(40, 66), ks=(4, 8), ws=20, ls=1, mode="scale_end"),
    dict(policy="full", qs=(64, 64), ks=(8, 8)),
    dict(policy="full", qs=(1 << 20,), ks=(128,), d=128),
]
NOT_SPLITTING = {
    "fp32": dict(dtype=_lib.F32, qs=(16384,), ks=(32,)),
    "fp64": dict(dtype=_lib.F64, qs=(16384,), ks=(32,)),
    "d129": dict(qs=(16384,), ks=(32,), d=129, vd=64),
    "vd129": dict(qs=(16384,), ks=(32,), d=64, vd=129),
    "nk129": dict(qs=(16384,), ks=(129,)),
    "nq2047": dict(qs=(2047,), ks=(1,)),
    # none_front, window 256: the 128 keys are seen by the first 128 + 256 queries or so, not by 16384
    "local256": dict(policy="local", qs=(16384,), ks=(128,), ws=256),
}


def _ids(k):
    return "-".join(map(str, k.values()))


@pytest.mark.parametrize("kw", SPLITTING, ids=_ids)
def test_qualifying_shapes_split(kw):
    p = _prob(**kw)
    nq, nk = _nelems(kw["qs"]), _nelems(kw["ks"])
    chunks, chunk, qb, qe = _qplan(p)
    assert chunks >= 2
    assert chunks <= 64
    assert chunk % 128 == 0 and chunk >= 512
    assert chunk >= (512 if nk <= 64 else 1024)
    assert qe - qb >= 2048
    # the chunks tile the range from the 32-query tile that holds its first query
    first = qb // 32 * 32
    assert (chunks - 1) * chunk < qe - first <= chunks * chunk
    # the chunk length is the stated function of the span
    span = qe - first
    want = max(512 if nk <= 64 else 1024, -(-(-(-span // 64)) // 128) * 128)
    assert chunk == want
    # the range is the rule's query range of the whole key block
    probe = (ctypes.c_int32 * 5)()
    assert _lib.lib().fa_rule_probe(p, 0, nq - 1, 0, nk - 1, probe) == _lib.FA_OK
    assert (qb, qe) == (probe[2], probe[3])


def test_known_plans():
    """The shapes of tests/test_gpu_splitq_bwd.py and of tools/splitq_bwd_time.py."""
    assert _qplan(_prob(qs=(2600,), ks=(33,)))[:2] == (6, 512)
    assert _qplan(_prob(qs=(2600,), ks=(64,)))[:2] == (6, 512)
    assert _qplan(_prob(qs=(2600,), ks=(65,)))[:2] == (3, 1024)
    assert _qplan(_prob(qs=(2600,), ks=(128,)))[:2] == (3, 1024)
    assert _qplan(_prob(policy="causal", qs=(4101,), ks=(33,), mode="scale_front"))[:2] == (9, 512)
    assert _qplan(_prob(qs=(16384,), ks=(77,))) == (16, 1024, 0, 16384)
    assert _qplan(_prob(qs=(16384,), ks=(32,))) == (32, 512, 0, 16384)
    assert _qplan(_prob(qs=(1 << 20,), ks=(32,))) == (64, 16384, 0, 1 << 20)


@pytest.mark.parametrize("name", sorted(NOT_SPLITTING))
def test_envelope_edges_do_not_split(name):
    p = _prob(**NOT_SPLITTING[name])
    assert _qplan(p)[0] == 0
    assert _split_bytes(p) == _plain_bytes(p)


def test_short_local_window_has_a_short_query_range():
    p = _prob(**NOT_SPLITTING["local256"])
    chunks, _, qb, qe = _qplan(p)
    probe = (ctypes.c_int32 * 5)()
    assert _lib.lib().fa_rule_probe(p, 0, 16383, 0, 127, probe) == _lib.FA_OK
    assert (qb, qe) == (probe[2], probe[3])
    assert 0 < qe - qb < 2048 and chunks == 0


def test_query_rows_past_the_32_bit_offsets_do_not_split():
    """max(d, v_d) * (nq + 8) * 2 < 2^31: the dK/dV kernels address a slice's Q / dO channel rows with 32-bit
    buffer offsets.  One query below the edge splits, the edge does not, with either channel count at 128."""
    edge = (1 << 31) // (2 * 128) - 8
    kw = dict(policy="full", ks=(32,), d=128)
    assert _qplan(_prob(**dict(kw, qs=(edge - 1,))))[0] >= 2
    for q in (edge, edge + 1):
        p = _prob(**dict(kw, qs=(q,)))
        assert _qplan(p)[0] == 0
        assert _split_bytes(p) == _plain_bytes(p)
    assert _qplan(_prob(**dict(kw, qs=(edge - 1,), d=64, vd=128)))[0] >= 2
    assert _qplan(_prob(**dict(kw, qs=(edge,), d=64, vd=128)))[0] == 0
    # at 64 channels the edge is twice as far
    assert _qplan(_prob(**dict(kw, qs=(edge,), d=64, vd=64)))[0] >= 2


@pytest.mark.parametrize("kw", SPLITTING + [NOT_SPLITTING["local256"], NOT_SPLITTING["nq2047"]], ids=_ids)
def test_plan_and_per_slice_workspace_do_not_depend_on_batch(kw):
    plans = {_qplan(_prob(**dict(kw, b=b))) for b in (1, 5, 4096)}
    assert len(plans) == 1
    chunks = plans.pop()[0]
    p1 = _prob(**dict(kw, b=1))
    per_slice = chunks * (p1.d + p1.v_d) * _nelems(kw["ks"]) * 4
    for b in (1, 5, 4096):
        p = _prob(**dict(kw, b=b))
        extra = _split_bytes(p) - _plain_bytes(p)
        assert b * per_slice <= extra < b * per_slice + 256


@pytest.mark.parametrize("kw", SPLITTING + list(NOT_SPLITTING.values()), ids=_ids)
def test_workspace_formula(kw):
    """Outside the envelope fa_backward's workspace; inside it that plus b * chunks * (d + v_d) * nk floats
    rounded up to the 256-byte granularity of the other regions."""
    for b in (1, 5, 4096):
        p = _prob(**dict(kw, b=b))
        chunks = _qplan(p)[0]
        if chunks == 0:
            assert _split_bytes(p) == _plain_bytes(p)
        else:
            assert _split_bytes(p) == _plain_bytes(p) + _part_bytes(b, chunks, p.d, p.v_d, _nelems(kw["ks"]))


def test_unequal_channels_size_the_partials_by_d_plus_vd():
    p = _prob(policy="full", qs=(2600,), ks=(33,), d=96, vd=40, b=3)
    assert _qplan(p)[0] == 6
    assert _split_bytes(p) == _plain_bytes(p) + _part_bytes(3, 6, 96, 40, 33)
    assert _part_bytes(3, 6, 96, 40, 33) != _part_bytes(3, 6, 96, 96, 33)


def test_the_two_plans_are_never_both_active():
    seen_q = seen_k = 0
    for nq, nk, pol, d in itertools.product((1, 33, 128, 129, 2047, 2048, 4101), (1, 33, 128, 129, 2047, 2048, 4101),
                                            ("full", "causal", "local"), (64, 128)):
        for mode in ("none_front", "scale_end"):
            p = _prob(policy=pol, qs=(nq,), ks=(nk,), d=d, mode=mode, ws=3000)
            q, k = _qplan(p)[0], _kplan(p)[0]
            assert q == 0 or k == 0, (nq, nk, pol, mode, d)
            seen_q += q > 0
            seen_k += k > 0
            part = _part_bytes(p.b, q, p.d, p.v_d, nk) if q else (p.b * k * p.d * nq * 4 + 255) // 256 * 256 if k else 0
            assert _split_bytes(p) == _plain_bytes(p) + part
    assert seen_q > 0 and seen_k > 0


@pytest.mark.parametrize("kw", FEW_QUERY_SHAPES, ids=lambda k: f"{k['policy']}-{len(k['qs'])}d")
def test_key_chunk_plan_is_unchanged_on_few_query_shapes(kw):
    p = _prob(**kw)
    assert _kplan(p)[0] >= 2
    assert _kplan(p) == _kplan(p, "forward")
    assert _qplan(p)[0] == 0
    nq = _nelems(kw["qs"])
    assert _split_bytes(p) == _plain_bytes(p) + (p.b * _kplan(p)[0] * p.d * nq * 4 + 255) // 256 * 256


@pytest.mark.parametrize("kw", SPLITTING, ids=_ids)
def test_key_chunk_plan_is_empty_on_few_key_shapes(kw):
    assert _kplan(_prob(**kw))[0] == 0


def test_invalid_problem_is_rejected():
    p = _prob(qs=(16384,), ks=(32,))
    assert _qplan(p)[0] >= 2
    p.seq_dims = 3
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_backward_split_q_plan(p, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert _lib.lib().fa_backward_split_plan(p, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert _split_bytes(p) == 0
    assert _lib.lib().fa_backward_split_q_plan(_prob(qs=(16384,), ks=(32,)), None) == _lib.FA_ERR_INVALID_ARGUMENT
