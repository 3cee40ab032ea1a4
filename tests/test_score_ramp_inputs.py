"""CPU tests of the staircase-score inputs (tests/score_ramp.py): the conditions that keep
tests/test_gpu_score_range.py honest, computed from the inputs alone for every case of its table.

  * every special value survives the case's dtype exactly, and the fp16 kernels' pre-scaled Q stays finite;
  * a numpy model of the lazy rebase (the kernel's tile width and threshold) shows, among the climb rows
    of every case, a rebase on two consecutive tiles, a rebase on a row's last (ragged or rule-mixed)
    tile and a stretch of two tiles without one, and none on any flat or fall row;
  * the emulated documented fp16 deviation (pre-scaled fp16 Q, P, dS and the outputs rounded to fp16)
    passes run_case's checks of O, l and m (m with the tight bound the GPU test passes) using at most half
    of each allowance, and an fp16 case carries bwd=True exactly when the emulated gradients pass
    gate.grad_bound and the slope check at half the allowance too.

`python -m tests.test_score_ramp_inputs` rewrites profiles/score_ramp_gate.txt (the per-case worst
ratios); the test checks that the committed file lists every case."""

import ctypes
import functools
import os

import numpy as np
import pytest

from tests import score_ramp as R

ALL = R.CASES + [R.NO_REBASE_CASE]
F16_CASES = [c for c in ALL if c.dtype == np.float16]
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_ramp_gate.txt")
HALF = 0.5
_id = lambda c: c.id  # noqa: E731


@functools.lru_cache(maxsize=None)
def _made(case_id):
    case = R.CASE_BY_ID.get(case_id, R.NO_REBASE_CASE)
    inputs, info = case.inputs()
    for x in inputs:
        x.setflags(write=False)
    return case, inputs, info


@functools.lru_cache(maxsize=None)
def _ratios(case_id):
    case, inputs, info = _made(case_id)
    flat = [R._flat3(x, case.seq_dims) for x in inputs]
    got, has = R.emulate_f16(*flat, case.problem(), case.qs, case.ks, bwd=True)
    return R.gate_ratios(case, inputs, info, got, has)


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_special_values_round_trip(case):
    _, inputs, info = _made(case.id)
    exact, _ = R.ramp_inputs(case.problem(), np.float64, case.batch, case.d, case.vd, case.qs, case.ks, case.ramp,
                             case.seed)
    Q, K = (R._flat3(x, case.seq_dims) for x in inputs[:2])
    Q64, K64 = (R._flat3(x, case.seq_dims) for x in exact[:2])
    assert Q.dtype == case.dtype
    assert (Q[:, :R.N_SPECIAL].astype(np.float64) == Q64[:, :R.N_SPECIAL]).all()
    assert (K[:, :R.N_SPECIAL].astype(np.float64) == K64[:, :R.N_SPECIAL]).all()
    assert max(np.abs(Q64).max(), np.abs(K64).max()) <= 16384
    for x in inputs:
        assert np.isfinite(x.astype(np.float64)).all()
    if case.dtype == np.float16:
        c2 = np.float32(np.float32(1.0 / np.sqrt(case.d)) * np.float32(R.LOG2E))
        assert np.isfinite((Q.astype(np.float32) * c2).astype(np.float16)).all()
    # the three row kinds are interleaved in every group of four rows that attends anything
    kind = info["kind"]
    assert {R.CLIMB, R.FLAT, R.FALL} <= set(kind[info["has"]].tolist())


def test_lift_is_exact_after_pre_scaling():
    """Both factors of the lift channel keep their value under the fp16 kernels' pre-scaling to 2e-5
    (relative), so the shift it adds to every score moves P, and so l and dV, by less than 4e-4 of their
    1e-3 allowance at 24 log2 units, whichever operand a pass pre-scales."""
    for d in (32, 64, 128, 256, 300):
        L, kappa = R.lift_pair(d, 24.0)
        c = R.LOG2E / np.sqrt(d)
        assert abs(L * kappa * c - 24.0) <= 3.0
        c2 = np.float32(np.float32(1.0 / np.sqrt(d)) * np.float32(R.LOG2E))
        for x in (L, kappa):
            assert np.float64(np.float16(x)) == x
            assert abs(float(np.float16(np.float32(x) * c2)) / (x * c) - 1.0) < 2e-5


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_rebases_really_happen(case):
    _, inputs, info = _made(case.id)
    Q, K = (R._flat3(x, case.seq_dims) for x in inputs[:2])
    scores = R.kernel_scores(Q, K, case.d, case.log2_units)
    rebased, active = R.rebase_tiles(scores, info["mask"], case.tile, case.thr)
    cond = R.rebase_conditions(rebased, active, info["kind"])
    assert cond["n"] > 0 and cond["others_still"], cond
    for name in ("consecutive", "last", "quiet"):
        if name in case.waive:
            assert not cond[name], f"{name} is waived for {case.id} but holds: drop the waiver"
        else:
            assert cond[name], (name, cond)
    # the far steps overflow the fp32 exp2 of a speculative exponential (> 128 log2 units in one step)
    climb = info["kind"] == R.CLIMB
    span = scores[climb].max() - np.where(info["mask"], scores, np.inf)[climb].min()
    assert (span > 128 * (1 if case.log2_units else np.log(2))) != ("overflow" in case.waive), span


def test_rebase_model_on_a_hand_made_row():
    """Tile width 2, threshold 8: seed, a step under the threshold, accumulated steps over it, a masked
    tile, a fall."""
    s = np.array([[0.0, 1.0, 5.0, 6.0, 9.5, 9.0, 50.0, 50.0, 30.0, 10.0, 17.6, 3.0]])
    mask = np.ones_like(s, dtype=bool)
    mask[0, 6:8] = False
    rebased, active = R.rebase_tiles(s, mask, 2, 8.0)
    assert active.tolist() == [[True, True, True, False, True, True]]
    assert rebased.tolist() == [[False, False, True, False, True, False]]


@pytest.mark.parametrize("case", [c for c in ALL if c.split], ids=_id)
def test_split_cases_split(case):
    from tf_flash_attention_amd import _lib
    pol = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}[case.policy]
    sync = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}[case.mode]
    prob = _lib.make_problem(_lib.F16, pol, 1, sync, 1, case.qs, case.ks, case.d, case.vd, case.ws, case.ls, case.causal)
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(prob, out) == 0
    assert out[0] >= 2, tuple(out)


@pytest.mark.parametrize("case", F16_CASES, ids=_id)
def test_gate_admits_the_documented_deviation(case):
    r = _ratios(case.id)
    for name in ("O", "l", "m"):
        assert r[name] <= HALF, (name, r)


@pytest.mark.parametrize("case", [c for c in F16_CASES if not c.variant], ids=_id)
def test_backward_flag_follows_the_emulation(case):
    r = _ratios(case.id)
    worst = max(v for k, v in r.items() if k[0] == "d")
    assert case.bwd == (worst <= HALF), r


def _profile_lines():
    yield "Emulated documented fp16 deviation on the staircase-score inputs (tests/score_ramp.py): worst"
    yield "|error| / allowance under run_case's checks (m with the tight bound) and the backward gate."
    yield "Written by `python -m tests.test_score_ramp_inputs`; every forward ratio must be <= 0.5, and a"
    yield "case runs its backward on the GPU (bwd) only if every backward ratio is <= 0.5 too."
    yield ""
    yield f"{'case':34s} {'O':>5s} {'l':>5s} {'m':>5s} {'dQ':>5s} {'dK':>5s} {'dV':>5s} {'slope':>5s}  bwd"
    for c in F16_CASES:
        r = _ratios(c.id)
        slope = max([v for k, v in r.items() if k.endswith("_slope")] or [0.0])
        yield (f"{c.id:34s} {r['O']:5.2f} {r['l']:5.2f} {r['m']:5.2f} {r['dQ']:5.2f} {r['dK']:5.2f} {r['dV']:5.2f} "
               f"{slope:5.2f}  {'yes' if c.bwd else 'no'}")


def test_profile_lists_every_case():
    with open(PROFILE) as f:
        text = f.read()
    for c in F16_CASES:
        assert f"\n{c.id} " in text, c.id


if __name__ == "__main__":
    with open(PROFILE, "w") as f:
        f.write("\n".join(_profile_lines()) + "\n")
