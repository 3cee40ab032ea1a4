"""GPU tests of the forwards' lazy softmax rebase on staircase-score inputs (tests/score_ramp.py).

Every other input of the suite is U(-2, 2): after the seed tile no row's max passes m_run by the
rebase threshold, so the branch that rescales O and l, re-bases the scores of the tile in flight and
recomputes P after the speculative exponentials never runs with anything but zeros to rescale.  Here
each case's rows climb (or fall) in steps chosen against its kernel's tile width and threshold;
tests/test_score_ramp_inputs.py proves on the CPU that the rebases happen where intended and that the
documented fp16 deviation stays within half of run_case's unchanged tolerances on these inputs.

Each case goes through run_case with its existing tolerances; only m's dot-product term, which the
staircase's large cancelling products would make vacuous, is replaced by the bound the generator
justifies (score_ramp.m_rounding_bound).  The route of each case is named beside it in score_ramp.CASES."""

import ctypes

import numpy as np
import pytest

from tests import score_ramp as R
from tests.test_gpu_parity import diag_lib, run_case  # noqa: F401  (diag_lib is a fixture)

pytestmark = pytest.mark.gpu

_id = lambda c: c.id  # noqa: E731


def _assert_splits(case):
    from tf_flash_attention_amd import _lib
    pol = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}[case.policy]
    sync = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}[case.mode]
    prob = _lib.make_problem(_lib.F16, pol, 1, sync, 1, case.qs, case.ks, case.d, case.vd, case.ws, case.ls, case.causal)
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(prob, out) == 0
    assert out[0] >= 2, tuple(out)


def _run(case):
    inputs, info = case.inputs()
    Q, K = (R._flat3(x, case.seq_dims) for x in inputs[:2])
    return run_case(case.dtype, case.policy, case.seq_dims, case.mode, case.batch, case.d, case.vd, case.qs, case.ks,
                    ws=case.ws, ls=case.ls, causal=case.causal, bwd=case.bwd, inputs=inputs,
                    m_bound=R.m_rounding_bound(Q, K, info, case.dtype, case.d))


@pytest.mark.parametrize("case", [c for c in R.CASES if not c.variant], ids=_id)
def test_staircase_scores(case):
    if case.split:
        _assert_splits(case)
    _run(case)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.variant], ids=_id)
def test_staircase_scores_forced_structures(monkeypatch, diag_lib, case):  # noqa: F811
    monkeypatch.setenv("FA_FWD_VARIANT", case.variant)
    _run(case)


def test_a_missing_rebase_is_seen(monkeypatch, diag_lib):  # noqa: F811
    """FA_FWD_VARIANT=2116 runs the ping-pong study kernel without its seed and rebase (kANoRebase in
    csrc/diag/fa_fwd_f16_pp.hip, a numerics-only ablation: the same loads and stores, wrong values).  The
    full-policy case that every forced structure above passes must fail the gate there; the same kernel
    with the branch (2000) passes it."""
    case = R.NO_REBASE_CASE
    monkeypatch.setenv("FA_FWD_VARIANT", "2000")
    _run(case)
    monkeypatch.setenv("FA_FWD_VARIANT", case.variant)
    with pytest.raises(AssertionError):
        _run(case)
