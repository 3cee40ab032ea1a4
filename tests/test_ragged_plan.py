"""CPU tests of the ragged forward's routing rule (include/fa_api.h: fa_forward_ragged_plan,
fa_forward_ragged_workspace_bytes, the host checks of fa_forward_ragged).  Host-only: no device
work."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}


def _prob(policy="full", qs=(1,), ks=(2601,), d=64, vd=None, dtype=_lib.F16, b=None, g=4):
    return _lib.make_problem(dtype, POL[policy], len(qs), _lib.NONE_FRONT, 2 * g if b is None else b, qs, ks, d,
                             d if vd is None else vd)


def _plan(p, g, fn="fa_forward_ragged_plan"):
    out = (ctypes.c_int32 * 6)()
    assert getattr(_lib.lib(), fn)(p, g, out) == _lib.FA_OK
    return tuple(out)


def _bytes(p, g):
    return int(_lib.lib().fa_forward_ragged_workspace_bytes(p, g))


def _launch(p, g, kv_per_len=1, ws_bytes=0, k_lens=None, ws=None):
    """fa_forward_ragged with null tensors: every case here must return before a pointer is touched."""
    return _lib.lib().fa_forward_ragged(None, p, g, None, None, None, k_lens, kv_per_len, 0, None, None, None, ws,
                                        ws_bytes)


GROUPED = [dict(g=2, qs=(1,)), dict(g=8, qs=(1,)), dict(g=128, qs=(1,)), dict(g=3, qs=(3,)), dict(g=2, qs=(33,)),
           dict(g=2, qs=(64,)), dict(g=4, qs=(8,), d=128), dict(g=4, qs=(8,), d=96, vd=40),
           dict(g=8, qs=(4,), ks=(1,)), dict(g=4, qs=(8,), ks=(16384,)), dict(g=4, qs=(32,), ks=(100000,))]


@pytest.mark.parametrize("kw", GROUPED, ids=lambda k: "-".join(map(str, k.values())))
def test_plan_is_the_grouped_plan_under_the_full_rule(kw):
    p = _prob(**kw)
    plan = _plan(p, kw["g"])
    assert plan == _plan(p, kw["g"], "fa_forward_grouped_plan")
    assert plan[0] >= 1 and plan[2:4] == (0, p.k_seq[0])
    assert _bytes(p, kw["g"]) == int(_lib.lib().fa_forward_grouped_workspace_bytes(p, kw["g"]))


@pytest.mark.parametrize("nq,nk,chunks,chunk,pitch", [(1, 1, 1, 512, 1), (1, 2601, 6, 512, 1), (33, 2601, 6, 512, 64),
                                                      (128, 2601, 3, 1024, 128), (4, 16384, 32, 512, 4),
                                                      (4, 32769, 57, 576, 4)])
def test_one_group_is_planned(nq, nk, chunks, chunk, pitch):
    """Ungrouped decode: grouped_plan's formula with kv_group = 1 (fa_forward_grouped_plan reports 0 chunks)."""
    p = _prob(g=1, qs=(nq,), ks=(nk,))
    assert _plan(p, 1) == (chunks, chunk, 0, nk, pitch, pitch)
    assert _plan(p, 1, "fa_forward_grouped_plan")[0] == 0


OUT = {
    "d129": dict(g=4, qs=(8,), d=129, vd=64),
    "vd129": dict(g=4, qs=(8,), d=64, vd=129),
    "g2-P128": dict(g=2, qs=(128,)),           # g * P = 256
    "g1-nq129": dict(g=1, qs=(129,)),          # P = 256
    "g129": dict(g=129, qs=(1,)),
    "fp32": dict(g=4, qs=(8,), dtype=_lib.F32),
    "fp64": dict(g=1, qs=(1,), dtype=_lib.F64),
    "2d": dict(g=2, qs=(2, 4), ks=(40, 66)),
    "nk0": dict(g=4, qs=(8,), ks=(0,)),
    "nq0": dict(g=4, qs=(0,)),
}


@pytest.mark.parametrize("name", sorted(OUT))
def test_outside_the_envelope(name):
    kw = OUT[name]
    p = _prob(**kw)
    assert _plan(p, kw["g"])[0] == 0
    assert _bytes(p, kw["g"]) == 0
    assert _launch(p, kw["g"]) == _lib.FA_ERR_UNSUPPORTED
    assert "envelope" in _lib.last_error()


@pytest.mark.parametrize("policy", ["causal", "local"])
def test_policy_must_be_full(policy):
    p = _prob(policy=policy, g=4, qs=(8,))
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    assert _lib.lib().fa_forward_ragged_plan(p, 4, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "FA_FULL" in _lib.last_error()
    assert tuple(out) == (-7,) * 6
    assert _bytes(p, 4) == 0
    assert _launch(p, 4) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "FA_FULL" in _lib.last_error()


@pytest.mark.parametrize("b,g,kv_per_len,text", [(24, 4, 0, "kv_per_len must be >= 1"), (24, 4, -2, "kv_per_len must be >= 1"),
                                                 (24, 4, 4, "multiple of kv_per_len"), (8, 8, 2, "multiple of kv_per_len"),
                                                 (7, 2, 1, "multiple of kv_group"), (4, 0, 1, "kv_group")])
def test_lengths_and_groups_must_divide(b, g, kv_per_len, text):
    p = _prob(b=b, g=max(g, 1), qs=(1,))
    assert _launch(p, g, kv_per_len) == _lib.FA_ERR_INVALID_ARGUMENT
    assert text in _lib.last_error()


def test_workspace_formula_and_short_workspace():
    for g, nq, vd, bkv in ((1, 1, 64, 16), (1, 33, 40, 3), (4, 4, 128, 5), (8, 1, 8, 1024)):
        p = _prob(g=g, qs=(nq,), d=vd, b=bkv * g)
        chunks, _, _, _, pitch, rows = _plan(p, g)
        assert rows == g * pitch
        exact = bkv * chunks * rows * (vd + 3) * 4
        assert _bytes(p, g) == (exact + 255) // 256 * 256
        assert _launch(p, g, 1, _bytes(p, g) - 1, ws=ctypes.c_void_p(256)) == _lib.FA_ERR_WORKSPACE_TOO_SMALL
        assert _launch(p, g, 1, _bytes(p, g), ws=None) == _lib.FA_ERR_WORKSPACE_TOO_SMALL


@pytest.mark.parametrize("kw", GROUPED + [dict(g=1, qs=(1,)), dict(g=1, qs=(33,))] + [OUT[k] for k in sorted(OUT)],
                         ids=lambda k: "-".join(map(str, k.values())))
def test_plan_does_not_depend_on_batch(kw):
    g = kw["g"]
    assert len({_plan(_prob(**dict(kw, b=bkv * g)), g) for bkv in (0, 1, 5, 4096)}) == 1


def test_an_empty_batch_is_ok_and_a_null_k_lens_is_not():
    p0 = _prob(b=0, g=4, qs=(8,))
    assert _bytes(p0, 4) == 0
    assert _launch(p0, 4, 1, 0, ws=ctypes.c_void_p(256)) == _lib.FA_OK
    p = _prob(b=8, g=4, qs=(8,))
    assert _launch(p, 4, 1, _bytes(p, 4), ws=ctypes.c_void_p(256)) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "k_lens" in _lib.last_error()
