"""CPU tests of the split-key forward's routing rule (include/fa_api.h: fa_forward_split_plan,
fa_forward_workspace_bytes).  Host-only: no device work."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}


def _prob(policy="full", qs=(1,), ks=(2048,), d=64, vd=None, mode="none_front", dtype=_lib.F16, b=2, ws=1, ls=0,
          causal=False):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], b, qs, ks, d, d if vd is None else vd, ws, ls,
                             causal)


def _plan(p):
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(p, out) == _lib.FA_OK
    return tuple(out)


def _bytes(p):
    return int(_lib.lib().fa_forward_workspace_bytes(p))


def _nelems(seq):
    n = 1
    for s in seq:
        n *= s
    return n


SPLITTING = [
    dict(policy="full", qs=(1,), ks=(2048,)),
    dict(policy="causal", qs=(64,), ks=(8192,), mode="scale_end"),
    dict(policy="full", qs=(8, 8), ks=(64, 64)),
]
NOT_SPLITTING = {
    "fp32": dict(dtype=_lib.F32, qs=(32,), ks=(16384,)),
    "fp64": dict(dtype=_lib.F64, qs=(32,), ks=(16384,)),
    "d129": dict(qs=(32,), ks=(16384,), d=129, vd=64),
    "vd129": dict(qs=(32,), ks=(16384,), d=64, vd=129),
    "nq129": dict(qs=(129,), ks=(16384,)),
    "local256": dict(policy="local", qs=(128,), ks=(16384,), ws=256),
    "nk2047": dict(qs=(1,), ks=(2047,)),
}


@pytest.mark.parametrize("kw", SPLITTING, ids=lambda k: f"{k['policy']}-{len(k['qs'])}d")
def test_qualifying_shapes_split(kw):
    p = _prob(**kw)
    chunks, chunk, kb, ke = _plan(p)
    assert chunks >= 2
    assert chunk % 64 == 0 and chunk >= 512
    assert ke - kb >= 2048
    # the chunks tile the range from the 64-key tile that holds its first key
    first = kb // 64 * 64
    assert (chunks - 1) * chunk < ke - first <= chunks * chunk


@pytest.mark.parametrize("name", sorted(NOT_SPLITTING))
def test_envelope_edges_do_not_split(name):
    p = _prob(**NOT_SPLITTING[name])
    assert _plan(p)[0] == 0
    assert _bytes(p) == 0


@pytest.mark.parametrize("kw", SPLITTING + list(NOT_SPLITTING.values()), ids=lambda k: "-".join(map(str, k.values())))
def test_plan_and_workspace_agree(kw):
    for b in (1, 5, 4096):
        p = _prob(**dict(kw, b=b))
        chunks = _plan(p)[0]
        nbytes = _bytes(p)
        assert (chunks == 0) == (nbytes == 0)
        if chunks:
            exact = b * chunks * _nelems(kw["qs"]) * (p.v_d + 3) * 4
            assert exact <= nbytes < exact + 256


@pytest.mark.parametrize("kw", SPLITTING + [NOT_SPLITTING["local256"], NOT_SPLITTING["nk2047"]],
                         ids=lambda k: "-".join(map(str, k.values())))
def test_plan_does_not_depend_on_batch(kw):
    plans = {_plan(_prob(**dict(kw, b=b))) for b in (1, 5, 4096)}
    assert len(plans) == 1


CASES_RANGE = SPLITTING + [
    dict(policy="causal", qs=(33,), ks=(4101,), mode="scale_front"),
    dict(policy="local", qs=(128,), ks=(4101,), ws=3000),
    dict(policy="local", qs=(128,), ks=(4101,), ws=3000, causal=True, mode="scale_front"),
    dict(policy="causal", qs=(4, 8), ks=(40, 66), mode="scale_end"),
    NOT_SPLITTING["local256"],
]


@pytest.mark.parametrize("kw", CASES_RANGE, ids=lambda k: "-".join(map(str, k.values())))
def test_range_matches_rule_probe(kw):
    p = _prob(**kw)
    nq, nk = _nelems(kw["qs"]), _nelems(kw["ks"])
    probe = (ctypes.c_int32 * 5)()
    assert _lib.lib().fa_rule_probe(p, 0, nq - 1, 0, nk - 1, probe) == _lib.FA_OK
    chunks, chunk, kb, ke = _plan(p)
    assert (kb, ke) == (probe[0], probe[1])
    assert (chunks >= 2) == (ke - kb >= 2048)
    if chunks:
        assert chunk % 64 == 0 and chunk >= 512


def test_invalid_problem_is_rejected():
    p = _prob()
    p.seq_dims = 3
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(p, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert _bytes(p) == 0
