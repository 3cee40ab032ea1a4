"""CPU tests of the decode staircase cases (tests/score_ramp.DECODE_CASES): the conditions that keep
tests/test_gpu_decode_score_range.py honest, computed from the inputs alone.

  * the special values survive fp16 exactly, the values past each length are the ones that would betray a read
    (scores above every climb and fall row's top, V = 65504), and the row kinds cycle over the folded row index;
  * the rebase model, run PER CHUNK (each chunk seeds afresh from its first tile), shows among the climb rows a
    rebase on two consecutive tiles, a rebase on a slice's ragged last tile and a quiet stretch; no flat, fall,
    padding or unseeded row moves by its own scores; every wave that fires also holds a row that must not move;
    under the tail rule a row without a key in a tile sits beside a wave-mate that rebases on it;
  * in the merge at least one live chunk's weight 2^(m_chunk - max) is exactly 0 in fp32 and one lies strictly
    between 0 and 1;
  * the emulated documented fp16 deviation passes test_gpu_ragged._check_ref (m with score_ramp.m_rounding_bound,
    as the GPU test passes it) using at most half of each allowance.

`python -m tests.test_decode_score_ramp_inputs` rewrites the decode section of profiles/score_ramp_gate.txt."""

import functools
import os

import numpy as np
import pytest
import torch

from oracle import fa_oracle as O
from tests import gate
from tests import ragged_ref
from tests import score_ramp as R
from tests import test_gpu_ragged as rg

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_ramp_gate.txt")
MARK = "Decode staircase cases"
HALF = 0.5
_id = lambda c: c.id  # noqa: E731


@functools.lru_cache(maxsize=None)
def _made(case_id):
    case = R.DECODE_CASE_BY_ID[case_id]
    made = R.decode_inputs(case)
    for n in ("Q", "K", "V"):
        made[n].setflags(write=False)
    return case, made


@functools.lru_cache(maxsize=None)
def _ratios(case_id):
    case, made = _made(case_id)
    if case.entry == "grouped":
        return _grouped_ratios(case, made)
    got = R.emulate_ragged_f16(made["Q"], made["K"], made["V"], made["lens"], case.g, case.tail)
    return rg._check_ref(tuple(torch.from_numpy(x) for x in got), made["Q"], made["K"], made["V"], made["lens"], case.g,
                         case.tail, m_bound=made["bound"])


def _grouped_ratios(case, made):
    """score_ramp.gate_ratios' forward part for a grouped case: emulate_f16 on expanded K / V under the case's
    rule, against the oracle, under run_case's checks with the per-head bounds."""
    prob = O.Problem("causal", 1, "scale_end") if case.tail else O.Problem("full", 1, "none_front")
    Q, K, V = made["Q"], np.repeat(made["K"], case.g, axis=0), np.repeat(made["V"], case.g, axis=0)
    got, has = R.emulate_f16(Q, K, V, None, prob, (case.nq,), (case.cap,), bwd=False)
    O64, L64, M64, _ = O.forward_f64(Q, K, V, prob)
    rtol, atol = gate.TOL[np.float16]["fwd"]
    res = {"O": float((np.abs(got["O"].astype(np.float64) - O64) / gate.plain_bound(O64, rtol, atol)).max())}
    m_f, M = got["m"].astype(np.float64)[:, has], M64.reshape(M64.shape[0], -1)[:, has]
    res["m"] = float((np.abs(m_f - M) / gate.m_tol_bounded(M, np.float16, made["bound"][:, has])).max())
    l_ref = L64.reshape(M64.shape[0], -1)[:, has] * np.exp(M - m_f)
    res["l"] = float((np.abs(got["l"].astype(np.float64)[:, has] - l_ref) / gate.plain_bound(l_ref, rtol, atol)).max())
    return res


@pytest.mark.parametrize("case", R.DECODE_CASES, ids=_id)
def test_shapes_and_lengths(case):
    chunks, chunk, pitch = case.plan
    assert case.g * pitch <= 128 and max(case.d, case.vd) <= 128
    lens = list(case.lens)
    if case.entry == "grouped":
        assert chunks >= 3 and set(lens) == {case.cap} and len(lens) >= 2
        return
    if "merge" in case.waive:
        return
    assert chunks >= 3 and max(lens) <= case.cap
    last = [L for L in lens if L > (chunks - 1) * chunk]
    assert any(L % 64 for L in last), "a length that ends mid-tile in the last chunk"
    assert any(L and L % chunk == 0 for L in lens), "a length on a chunk edge"
    assert any(L % chunk == 1 and L > chunk for L in lens), "a length one key past a chunk edge"
    assert any(0 < L < 64 for L in lens) and 0 in lens
    assert not case.tail or case.nq - 1 in lens
    for page in case.pages:
        assert case.cap % page == 0
    fast = case.d == case.vd and case.d in (32, 64, 128) and case.cap % 8 == 0
    assert fast != ("elem" in case.id or "big" in case.id)


@pytest.mark.parametrize("case", R.DECODE_CASES, ids=_id)
def test_special_values_and_the_values_past_the_lengths(case):
    _, made = _made(case.id)
    Q, K, V = made["Q"], made["K"], made["V"]
    assert max(np.abs(Q.astype(np.float64)).max(), np.abs(K.astype(np.float64)).max()) <= 16384
    assert all(np.isfinite(x.astype(np.float64)).all() for x in (Q, K, V))
    c2 = np.float32(np.float32(1.0 / np.sqrt(case.d)) * np.float32(R.LOG2E))
    assert np.isfinite((Q.astype(np.float32) * c2).astype(np.float16)).all()
    ramp = case.ramp
    for s, L in enumerate(made["lens"]):
        assert (K[s, [0, 3], L:] == 0).all() and (K[s, [1, 4], L:] == 1).all() and (V[s, :, L:] == 65504).all()
        assert (K[s, 2] == K[s, 2, 0]).all()                                     # the lift channel continues
        if L:
            e = R.plateau_exponents(L, ramp)
            assert (K[s, 0, :L].astype(np.float64) == -ramp.u * 2.0 ** e).all()
        if L == 0 or L == case.cap:
            continue
        for h in range(case.g):                                                 # scores past L lie above the tops
            bi = s * case.g + h
            sc = R.kernel_scores(Q[bi][None], K[s][None], case.d, True)
            mask = made["infos"][bi]["mask"]
            top = np.where(mask, sc[:, :L], -np.inf).max(axis=1)
            moving = (made["kinds"][bi] != R.FLAT) & made["infos"][bi]["has"]
            assert (sc[moving][:, L:].min(axis=1) > top[moving] + 0.5).all()
    # the kinds cycle over the folded row index head * nq + query
    for bi, (kind, info) in enumerate(zip(made["kinds"], made["infos"])):
        if info is not None:
            want = np.array(R.KIND_CYCLE)[((bi % case.g) * case.nq + np.arange(case.nq)) % 4]
            assert (kind[info["has"]] == want[info["has"]]).all()
    live = [k[i["has"]] for k, i in zip(made["kinds"], made["infos"]) if i is not None]
    assert {R.CLIMB, R.FLAT, R.FALL} <= set(np.concatenate(live).tolist())
    if case.lift < 0:
        assert (Q[:, 2] < 0).all()
        M = ragged_ref.forward_f64(Q, K, V, made["lens"], case.g, case.tail)[2]
        assert M.min() < -8 and M.max() <= 0


@pytest.mark.parametrize("case", R.DECODE_CASES, ids=_id)
def test_rebases_really_happen_in_every_chunk_model(case):
    _, made = _made(case.id)
    cond = R.decode_conditions(case, made)
    assert cond["n"] > 0 and cond["others_still"] and cond["fired_waves"] > 0, cond
    assert cond["waves_hold_a_still_row"], cond
    for name in ("consecutive", "last", "quiet"):
        if name in case.waive:
            assert not cond[name], f"{name} is waived for {case.id} but holds: drop the waiver"
        else:
            assert cond[name], (name, cond)
    if "merge" in case.waive:
        assert not cond["merge_zero"] and not cond["merge_between"]
    else:
        assert cond["merge_zero"] and cond["merge_between"], cond
    if case.tail and case.entry != "grouped":
        assert cond["idle"] != ("idle" in case.waive), cond


@pytest.mark.parametrize("case", R.DECODE_CASES, ids=_id)
def test_gate_admits_the_documented_deviation(case):
    r = _ratios(case.id)
    for name in ("O", "l", "m"):
        assert r[name] <= HALF, (name, r)


def test_emulation_is_the_base_one_on_full_lengths():
    """emulate_ragged_f16 with every length at the capacity is emulate_f16 under the full rule, bit for bit."""
    case, made = _made("grouped-d128-g4q7-full")
    Q, K, V = made["Q"], np.repeat(made["K"], case.g, axis=0), np.repeat(made["V"], case.g, axis=0)
    o, l, m = R.emulate_ragged_f16(made["Q"], made["K"], made["V"], made["lens"], case.g, False)
    ref, has = R.emulate_f16(Q, K, V, None, O.Problem("full", 1, "none_front"), (case.nq,), (case.cap,), bwd=False)
    assert has.all()
    assert np.array_equal(o, ref["O"]) and np.array_equal(l, ref["l"]) and np.array_equal(m, ref["m"])


@pytest.mark.parametrize("page", [0, 64], ids=["ragged", "paged64"])
@pytest.mark.parametrize("case", R.windowed_tail_cases(), ids=_id)
def test_a_window_of_capacity_minus_one_is_the_tail_plan_and_the_tail_mask(case, page):
    """What carries the proofs above over to the windowed run of tests/test_gpu_decode_score_range.py: at
    W = capacity - 1 the call is not delegated, its plan (the library's, host-only) is the tail plan chunk for chunk,
    lo = 0 for every length, and every query's interval is the tail rule's.  The paged run's capacity is rounded up to
    the page of 64 keys, which adds no chunk."""
    from tests import test_gpu_cache_fuzz as F
    from tests import test_gpu_window as gw
    from tests import window_ref
    cap = R.window_capacity(case, page)
    window = cap - 1
    chunks, chunk, pitch = case.plan
    assert len(R.windowed_tail_cases()) >= 3 and cap - case.cap < 64 and max(case.lens) < case.cap
    want = (chunks, chunk, cap, chunks, pitch, case.g * pitch, 0, 0)
    assert gw._plan(case.nq, cap, case.d, case.vd, case.g, window, page or None) == want
    assert F.window_plan(case.nq, cap, case.g, window) == want and R.decode_plan(case.nq, cap, case.g) == case.plan
    for L in case.lens:
        assert window_ref.window_lo(L, case.nq, window, cap) == 0
        mask = window_ref.window_mask(case.nq, cap, L, window)
        assert np.array_equal(mask, ragged_ref.ragged_mask(case.nq, cap, L, True))
        assert np.array_equal(mask[:, :L], case.mask(L)) and not mask[:, L:].any()


def _profile_lines():
    yield f"{MARK} (score_ramp.DECODE_CASES; written by `python -m tests.test_decode_score_ramp_inputs`): the"
    yield "emulated deviation under test_gpu_ragged._check_ref, m with the tight bound; every ratio must be <= 0.5."
    yield ""
    yield f"{'case':34s} {'O':>5s} {'l':>5s} {'m':>5s}"
    for c in R.DECODE_CASES:
        r = _ratios(c.id)
        yield f"{c.id:34s} {r['O']:5.2f} {r['l']:5.2f} {r['m']:5.2f}"


def test_profile_lists_every_case():
    with open(PROFILE) as f:
        text = f.read()
    for c in R.DECODE_CASES:
        assert f"\n{c.id} " in text, c.id


if __name__ == "__main__":
    with open(PROFILE) as f:
        head = f.read().split(MARK)[0].rstrip("\n")
    with open(PROFILE, "w") as f:
        f.write(head + "\n\n" + "\n".join(_profile_lines()) + "\n")
