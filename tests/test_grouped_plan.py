"""CPU tests of the grouped-query forward's routing rule (include/fa_api.h: fa_forward_grouped_plan,
fa_forward_grouped_workspace_bytes).  Host-only: no device work."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}


def _prob(policy="full", qs=(1,), ks=(2601,), d=64, vd=None, mode="none_front", dtype=_lib.F16, b=None, g=4, ws=1, ls=0,
          causal=False):
    return _lib.make_problem(dtype, POL[policy], len(qs), SYNC[mode], 2 * g if b is None else b, qs, ks, d,
                             d if vd is None else vd, ws, ls, causal)


def _plan(p, g):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_grouped_plan(p, g, out) == _lib.FA_OK
    return tuple(out)


def _bytes(p, g):
    return int(_lib.lib().fa_forward_grouped_workspace_bytes(p, g))


def _chunks(kb, ke, rows):
    """The chunk formula of fa_api.h: split_plan's, with min_chunk by the folded rows and no minimum range."""
    first = kb // 64 * 64
    span = ke - first
    capped = -(-(-(-span // 64)) // 64) * 64
    chunk = max(capped, 512 if rows <= 64 else 1024)
    return max(-(-span // chunk), 1), chunk


# ------------------------------------------------------------------ the envelope
IN = {
    "g128-nq1": dict(g=128, qs=(1,)),          # g * P = 128
    "g2-nq64": dict(g=2, qs=(64,)),            # g * P = 128 at the largest pitch
    "g4-nq32": dict(g=4, qs=(32,)),
    "g2-nq1": dict(g=2, qs=(1,)),
    "d128": dict(g=4, qs=(8,), d=128),
    "d96-vd40": dict(g=4, qs=(8,), d=96, vd=40),
    "nk1": dict(g=8, qs=(4,), ks=(1,)),
    "2d": dict(g=2, qs=(2, 4), ks=(40, 66)),
}
OUT = {
    "g129-nq1": dict(g=129, qs=(1,)),          # g * P = 129
    "g3-nq33": dict(g=3, qs=(33,)),            # 3 * 64 = 192
    "g2-nq65": dict(g=2, qs=(65,)),            # pitch 128
    "g5-nq32": dict(g=5, qs=(32,)),            # 160
    "d129": dict(g=4, qs=(8,), d=129, vd=64),
    "vd129": dict(g=4, qs=(8,), d=64, vd=129),
    "fp32": dict(g=4, qs=(8,), dtype=_lib.F32),
    "fp64": dict(g=4, qs=(8,), dtype=_lib.F64),
    "g1": dict(g=1, qs=(8,)),
    "nk0": dict(g=4, qs=(8,), ks=(0,)),
    "nq0": dict(g=4, qs=(0,)),
}


@pytest.mark.parametrize("name", sorted(IN))
def test_inside_the_envelope(name):
    kw = dict(IN[name])
    g = kw["g"]
    p = _prob(**kw)
    chunks, chunk, kb, ke, pitch, rows = _plan(p, g)
    assert chunks >= 1
    assert rows == g * pitch <= 128
    assert chunk % 64 == 0
    assert (chunks, chunk) == _chunks(kb, ke, rows)


@pytest.mark.parametrize("name", sorted(OUT))
def test_outside_the_envelope(name):
    kw = dict(OUT[name])
    g = kw["g"]
    p = _prob(**kw)
    assert _plan(p, g)[0] == 0
    if g > 1:
        assert _bytes(p, g) == 0


def test_group_of_one_is_the_ungrouped_entry_point():
    """kv_group = 1 reports no chunks; its workspace is fa_forward_ws's (the split-key plan may still fire)."""
    L = _lib.lib()
    for ks in ((2601,), (100,)):
        p = _prob(g=1, qs=(8,), ks=ks)
        assert _plan(p, 1)[0] == 0
        assert _bytes(p, 1) == int(L.fa_forward_workspace_bytes(p))
    assert int(L.fa_forward_workspace_bytes(_prob(g=1, qs=(8,), ks=(2601,)))) > 0


@pytest.mark.parametrize("nq,pitch", [(1, 1), (2, 2), (3, 4), (5, 8), (8, 8), (9, 16), (33, 64), (64, 64)])
def test_pitch(nq, pitch):
    g = 2
    out = _plan(_prob(g=g, qs=(nq,)), g)
    assert out[4] == pitch and out[5] == g * pitch
    assert out[0] >= 1


# ------------------------------------------------------------------ the chunk formula
@pytest.mark.parametrize("g,nq,nk,chunks,chunk", [
    (4, 8, 1, 1, 512),          # a short range is one chunk: no 2048-key minimum
    (4, 8, 512, 1, 512),
    (4, 8, 513, 2, 512),
    (4, 8, 2601, 6, 512),       # 32 rows: min_chunk 512
    (8, 8, 2601, 6, 512),       # 64 rows: still 512
    (8, 16, 2601, 3, 1024),     # 128 rows: min_chunk 1024
    (2, 64, 2601, 3, 1024),
    (4, 8, 16384, 32, 512),
    (4, 8, 32768, 64, 512),
    (4, 8, 32769, 57, 576),     # the cap: at most 64 chunks, tile-aligned
    (4, 32, 100000, 63, 1600),
])
def test_chunks_of_the_full_rule(g, nq, nk, chunks, chunk):
    out = _plan(_prob(g=g, qs=(nq,), ks=(nk,)), g)
    assert out[:4] == (chunks, chunk, 0, nk)
    assert out[0] <= 64 and (out[0] - 1) * out[1] < nk <= out[0] * out[1]


CASES_RANGE = [
    dict(policy="causal", qs=(1,), ks=(4200,), mode="scale_end"),
    dict(policy="causal", qs=(4,), ks=(4096,), mode="scale_end"),
    dict(policy="causal", qs=(16,), ks=(2600,), mode="none_front"),
    dict(policy="local", qs=(8,), ks=(8192,), ws=3000, mode="scale_front"),
    dict(policy="local", qs=(8,), ks=(8192,), ws=3000, mode="scale_front", causal=True),
    dict(policy="local", qs=(2, 4), ks=(40, 66), ws=20, ls=1, mode="scale_end", g=2),
    dict(policy="local", qs=(8,), ks=(8192,), ws=300, mode="scale_end"),   # a range that starts past key 0
]


@pytest.mark.parametrize("kw", CASES_RANGE, ids=lambda k: "-".join(map(str, k.values())))
def test_range_matches_rule_probe_and_formula(kw):
    g = kw.get("g", 4)
    p = _prob(**dict(kw, g=g))
    nq, nk = p.q_seq[0] * p.q_seq[1], p.k_seq[0] * p.k_seq[1]
    probe = (ctypes.c_int32 * 5)()
    assert _lib.lib().fa_rule_probe(p, 0, nq - 1, 0, nk - 1, probe) == _lib.FA_OK
    chunks, chunk, kb, ke, pitch, rows = _plan(p, g)
    assert (kb, ke) == (probe[0], probe[1])
    assert (chunks, chunk) == _chunks(kb, ke, rows)
    assert kb // 64 * 64 + chunks * chunk >= ke


def test_causal_none_front_sees_only_the_first_keys():
    out = _plan(_prob(policy="causal", qs=(16,), ks=(2600,), g=4), 4)
    assert out[:4] == (1, 512, 0, 16)


# ------------------------------------------------------------------ workspace, batch, errors
@pytest.mark.parametrize("name", sorted(IN))
def test_workspace_bytes_are_exact(name):
    kw = dict(IN[name])
    g = kw["g"]
    for bkv in (1, 5, 1024):
        p = _prob(**dict(kw, b=bkv * g))
        chunks, _, _, _, _, rows = _plan(p, g)
        exact = bkv * chunks * rows * (p.v_d + 3) * 4
        assert _bytes(p, g) == (exact + 255) // 256 * 256


@pytest.mark.parametrize("name", sorted(IN) + sorted(OUT))
def test_plan_does_not_depend_on_batch(name):
    kw = dict(IN.get(name) or OUT[name])
    g = kw["g"]
    plans = {_plan(_prob(**dict(kw, b=bkv * g)), g) for bkv in (0, 1, 5, 4096)}
    assert len(plans) == 1


@pytest.mark.parametrize("b,g", [(7, 2), (1, 4), (130, 128)])
def test_batch_must_be_a_multiple_of_the_group(b, g):
    L = _lib.lib()
    p = _prob(b=b, g=g, qs=(1,))
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    assert L.fa_forward_grouped_plan(p, g, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "multiple of kv_group" in _lib.last_error()
    assert tuple(out) == (-7,) * 6
    assert _bytes(p, g) == 0
    # the launch entry point checks on the host before it touches a pointer
    assert L.fa_forward_grouped(None, p, g, None, None, None, None, None, None, None, 0) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "multiple of kv_group" in _lib.last_error()


@pytest.mark.parametrize("g", [0, -3])
def test_group_must_be_positive(g):
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_grouped_plan(_prob(b=4, qs=(1,)), g, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert "kv_group" in _lib.last_error()


def test_invalid_problem_is_rejected():
    p = _prob()
    p.seq_dims = 3
    out = (ctypes.c_int32 * 6)()
    assert _lib.lib().fa_forward_grouped_plan(p, 4, out) == _lib.FA_ERR_INVALID_ARGUMENT
    assert _bytes(p, 4) == 0


def test_outside_the_envelope_the_launch_is_unsupported():
    """Host-only: the envelope is checked before any device call, so null pointers are never read."""
    p = _prob(g=4, qs=(8,), dtype=_lib.F32)
    st = _lib.lib().fa_forward_grouped(None, p, 4, None, None, None, None, None, None, None, 0)
    assert st == _lib.FA_ERR_UNSUPPORTED
    assert "envelope" in _lib.last_error()


def test_short_workspace_is_rejected_on_the_host():
    p = _prob(g=4, qs=(8,))
    need = _bytes(p, 4)
    assert need > 0
    st = _lib.lib().fa_forward_grouped(None, p, 4, None, None, None, None, None, None, None, need - 1)
    assert st == _lib.FA_ERR_WORKSPACE_TOO_SMALL
