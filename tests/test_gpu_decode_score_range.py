"""GPU tests of the lazy softmax rebase in the few-query decode forwards on staircase-score inputs
(tests/score_ramp.DECODE_CASES): the ragged partial kernel with per-slice lengths, its tail-causal form, its
D = 32 / 64 / 128 and element-wise instances, the pitch-64 and pitch-128 wave layouts, ragged_merge_kernel over three
chunks of which early ones underflow against the merged reference while dead ones are skipped, the same inputs
through a block table (fa_forward_paged), fa_forward_grouped at D = 128 and D = 32, and the tail cases through the sliding-window forwards at
W = capacity - 1 (the windowed partial kernels and window_merge_kernel under the tail plan and the tail mask).

Every other input of test_gpu_ragged.py and test_gpu_paged.py is U(-2, 2), which never moves a row's reference
after the seed tile.  tests/test_decode_score_ramp_inputs.py proves on the CPU, chunk by chunk, that these inputs
do, and that the documented fp16 deviation uses at most half of the unchanged allowances.  The ragged and paged
cases go through test_gpu_ragged._check_ref, the grouped ones through test_gpu_grouped._grouped_case; only m's
dot-product term, which the staircase's large cancelling products would make vacuous, is replaced by
score_ramp.m_rounding_bound.  The route of each case is named beside it in score_ramp.DECODE_CASES."""

import functools

import numpy as np
import pytest

from tests import score_ramp as R
from tests import test_gpu_ragged as rg
from tests.test_gpu_grouped import _grouped_case, _plan as _grouped_plan

pytestmark = pytest.mark.gpu

_id = lambda c: c.id  # noqa: E731
RAGGED = [c for c in R.DECODE_CASES if c.entry == "ragged"]
PAGED = [(c, page) for c in RAGGED for page in c.pages]
GROUPED = [c for c in R.DECODE_CASES if c.entry == "grouped"]
WINDOWED = R.windowed_tail_cases()
SPARE = 3


@functools.lru_cache(maxsize=None)
def _made(case_id):
    return R.decode_inputs(R.DECODE_CASE_BY_ID[case_id])  # shared by the ragged and paged tests; nothing writes to it


def _ragged(case, made):
    chunks, chunk, pitch = case.plan
    assert rg._plan(case.nq, case.cap, case.d, case.vd, case.g) == (chunks, chunk, 0, case.cap, pitch, case.g * pitch)
    st, *got = rg._abi(case.g, rg._dev(made["Q"]), rg._dev(made["K"]), rg._dev(made["V"]), made["lens"], tail=case.tail)
    assert st == 0
    return got


@pytest.mark.parametrize("case", RAGGED, ids=_id)
def test_staircase_scores_ragged(case):
    made = _made(case.id)
    got = _ragged(case, made)
    res = rg._check_ref(got, made["Q"], made["K"], made["V"], made["lens"], case.g, case.tail, m_bound=made["bound"])
    print(case.id, {k: round(v, 3) for k, v in res.items()})
    if case.lift < 0:
        m = got[2].cpu().numpy().astype(np.float64)
        live = np.repeat(np.asarray(made["lens"]) > 0, case.g)
        assert (m[live] < -8).all()


@pytest.mark.parametrize("case,page", PAGED, ids=lambda x: x.id if isinstance(x, R.DecodeCase) else f"page{x}")
def test_staircase_scores_paged(case, page):
    """The same padded cache scattered into a pool through a random table (pool pages that no sequence owns are
    NaN; one K/V head per sequence): bitwise the ragged result, and checked against the reference."""
    from tests import paged_ref
    from tests import test_gpu_paged as pg
    made = _made(case.id)
    bkv, max_pages = len(made["lens"]), case.cap // page
    num_pages = bkv * max_pages + SPARE
    table = np.random.default_rng(page).permutation(num_pages)[:bkv * max_pages].reshape(bkv, max_pages).astype(np.int32)

    def scatter(cache):
        pool = np.full((num_pages, 1, cache.shape[1], page), np.nan, np.float16)
        pool[table] = cache.reshape(bkv, 1, cache.shape[1], max_pages, page).transpose(0, 3, 1, 2, 4)
        return pool

    Kp, Vp = scatter(made["K"]), scatter(made["V"])
    st, *got = pg._abi(case.g, rg._dev(made["Q"]), rg._dev(Kp), rg._dev(Vp), table, made["lens"], tail=case.tail)
    assert st == 0
    assert rg._same(got, _ragged(case, made))
    rg._check_ref(got, made["Q"], paged_ref.gather(Kp, table, page), paged_ref.gather(Vp, table, page), made["lens"], case.g,
                  case.tail, m_bound=made["bound"])


@pytest.mark.parametrize("case", GROUPED, ids=_id)
def test_staircase_scores_grouped(monkeypatch, case):
    made = _made(case.id)
    policy, mode = ("causal", "scale_end") if case.tail else ("full", "none_front")
    assert _grouped_plan(policy, mode, (case.nq,), (case.cap,), case.d, case.vd, case.g)[:2] == case.plan[:2]
    dO = np.zeros((made["Q"].shape[0], case.vd, case.nq), np.float16)
    _grouped_case(monkeypatch, policy, mode, case.g, (case.nq,), (case.cap,), case.d, case.vd, bkv=len(made["lens"]),
                  inputs=(made["Q"], made["K"], made["V"], dO), m_bound=made["bound"])


@pytest.mark.parametrize("form", ["ragged", "paged"])
@pytest.mark.parametrize("case", WINDOWED, ids=_id)
def test_staircase_scores_windowed(case, form):
    """Every tail case whose lengths lie below its capacity through fa_forward_ragged_window / fa_forward_paged_window
    at W = capacity - 1: not delegated, so the windowed partial kernels and window_merge_kernel run; span_w is the
    capacity and every lo and klo is 0, so the plan is the tail plan and the mask the tail mask
    (tests/test_decode_score_ramp_inputs.py asserts both), and the CPU proofs of the tail cases carry over: rebases
    fire, chunks underflow in the merge, idle rows sit beside rebasing wave-mates.  The paged form runs on pages of
    64 keys at the capacity rounded up to the page (R.window_capacity; the keys added lie past every length)."""
    from tests import paged_ref
    from tests import test_gpu_cache_fuzz as F
    from tests import test_gpu_window as gw
    made = _made(case.id)
    page = 64 if form == "paged" else 0
    cap = R.window_capacity(case, page)
    window = cap - 1
    chunks, chunk, pitch = case.plan
    assert gw._plan(case.nq, cap, case.d, case.vd, case.g, window, page or None) == \
        (chunks, chunk, cap, chunks, pitch, case.g * pitch, 0, 0)
    K, V = (np.concatenate([x, np.repeat(x[:, :, -1:], cap - case.cap, axis=2)], axis=2) for x in (made["K"], made["V"]))
    bkv = len(made["lens"])
    c = dict(misalign=False, g=case.g, hk=1, lens=made["lens"], cap=cap, page=page, max_pages=cap // page if page else 0)
    tq = rg._dev(made["Q"])
    if form == "ragged":
        stores = (K, V, None)
    else:
        num_pages = bkv * c["max_pages"] + SPARE
        table = np.random.default_rng(7).permutation(num_pages)[:bkv * c["max_pages"]].reshape(bkv, -1).astype(np.int32)

        def scatter(cache):
            pool = np.full((num_pages, 1, cache.shape[1], page), np.nan, np.float16)
            pool[table] = cache.reshape(bkv, 1, cache.shape[1], c["max_pages"], page).transpose(0, 3, 1, 2, 4)
            return pool

        stores = (scatter(K), scatter(V), table)
        assert np.array_equal(paged_ref.gather(stores[0], table, page), K)
    got = F._forward(c, form, "fp16", window, True, tq, *stores, None, None)
    res = rg._check_ref(got, made["Q"], K, V, made["lens"], case.g, True, m_bound=made["bound"])
    tail = F._forward(c, form, "fp16", 0, True, tq, *stores, None, None)
    print(case.id, form, {k: round(v, 3) for k, v in res.items()}, "bitwise the tail call:", rg._same(got, tail))
