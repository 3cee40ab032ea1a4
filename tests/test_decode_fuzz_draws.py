"""CPU tests of the decode sweep (tests/test_gpu_decode_fuzz.py): its default range is not hollow, and the checker
it relies on rejects wrong models of the operation.

Coverage: over draw(0 .. 299) every (D instance) x (staging) x (ragged / paged) x (full / tail) cell, every pitch
class, plans of three or more chunks, an empty sequence beside a live one, lengths within one key of a chunk edge,
tail cases with some but not all rows empty and shared pages each occur at least a stated number of times (the
numbers lie under what the draw weights give; if a cell falls short, the weights change, not the number).

Mutations, in the style of tests/test_gate_mutations.py: four deliberately wrong numpy models of the operation
(float64, rounded to the output types as a kernel's results are) go through test_gpu_ragged._check_ref, the checker
of the GPU sweep, on default-range cases, and each must be rejected; the unmutated model and the float64 reference
with the documented fp16 roundings (score_ramp.emulate_ragged_f16) must pass.  Nothing here runs a kernel."""

import math
from collections import Counter

import numpy as np
import pytest
import torch

from tests import ragged_ref
from tests import score_ramp
from tests import test_gpu_decode_fuzz as F
from tests import test_gpu_ragged as rg

N = 300
DRAWS = [F.draw(i) for i in range(N)]
DECODE = [c for c in DRAWS if c["entry"] != "grouped"]


# ------------------------------------------------------------------ the draws
def test_every_case_is_inside_the_envelope():
    for c in DRAWS:
        assert c["g"] in F.GROUPS and 1 <= c["nq"] <= 128 and c["g"] * F.pitch_of(c["nq"]) <= 128
        assert 1 <= c["d"] <= 128 and 1 <= c["vd"] <= 128 and 1 <= c["cap"] <= F.MAX_CAP
        assert 1 <= c["seqs"] <= 3 and c["hk"] in (1, 2) and len(c["lens"]) == c["seqs"] and min(c["lens"]) >= 0
        if c["entry"] == "paged":
            assert c["page"] in F.PAGES and c["cap"] == c["page"] * c["max_pages"]
        if c["entry"] == "grouped":
            assert c["g"] >= 2
        assert F.draw(c["seed"]) == c


def test_plan_arithmetic_is_the_librarys():
    """plan() is tests/test_grouped_plan._chunks over [0, cap); spot-check it against the values that
    tests/test_ragged_plan.py pins for the library."""
    for nq, nk, chunks, chunk, pitch in [(1, 1, 1, 512, 1), (1, 2601, 6, 512, 1), (33, 2601, 6, 512, 64), (128, 2601, 3, 1024, 128)]:
        assert F.plan(nq, nk, 1) == (chunks, chunk, pitch)
    for c in DRAWS:
        assert F.plan(c["nq"], c["cap"], c["g"]) == score_ramp.decode_plan(c["nq"], c["cap"], c["g"])


def test_kernel_instances_and_stagings():
    cells = Counter((F.instance_of(c["d"], c["vd"]), F.fast_staging(c), c["entry"], c["tail"]) for c in DECODE)
    for D in F.INSTANCES:
        for fast in (True, False):
            for entry in ("ragged", "paged"):
                for tail in (False, True):
                    assert cells[(D, fast, entry, tail)] >= 3, ((D, fast, entry, tail), cells)


def test_pitch_classes_and_wave_layouts():
    pitches = Counter(F.pitch_of(c["nq"]) for c in DECODE)
    assert set(pitches) == {1, 2, 4, 8, 16, 32, 64, 128}
    assert sum(n for p, n in pitches.items() if p <= 32) >= 100 and pitches[64] >= 15 and pitches[128] >= 8
    assert len({c["g"] for c in DECODE}) == len(F.GROUPS)
    assert sum(c["g"] >= 3 and c["tail"] for c in DECODE) >= 30
    assert sum(c["hk"] == 2 and c["tail"] for c in DECODE) >= 30
    grouped = [c for c in DRAWS if c["entry"] == "grouped"]
    assert len(grouped) >= 15 and {c["tail"] for c in grouped} == {False, True}


def _near_chunk_edge(c):
    chunk = F.plan(c["nq"], c["cap"], c["g"])[1]
    return any(L >= chunk - 1 and min(L % chunk, chunk - L % chunk) <= 1 for L in F.clamped(c).tolist())


def test_edges():
    assert sum(F.plan(c["nq"], c["cap"], c["g"])[0] >= 3 for c in DECODE) >= 50
    assert sum(0 in F.clamped(c) and F.clamped(c).max() > 0 for c in DECODE) >= 20
    assert sum(_near_chunk_edge(c) for c in DECODE) >= 25
    assert sum(c["tail"] and any(0 < L < c["nq"] for L in c["lens"]) for c in DECODE) >= 8
    assert sum(c["shared"] for c in DECODE) >= 8
    assert sum(max(c["lens"]) > c["cap"] for c in DECODE) >= 15
    assert sum(c["misalign"] for c in DECODE) >= 20
    for junk in F.JUNK:
        assert sum(bool((F.build(c)["table_dev"] == junk).any()) for c in DECODE[:120] if c["entry"] == "paged") >= 5


def test_inputs_past_the_lengths_are_nan_and_the_pool_gathers_back():
    from tests import paged_ref
    for c in [c for c in DECODE if c["entry"] == "paged"][:12] + [c for c in DECODE if c["shared"]][:6]:
        p = F.build(c)
        K = paged_ref.gather(p["Kp"], p["table_ref"], c["page"])
        assert np.array_equal(K, p["K"], equal_nan=True)
        live = np.repeat(F.clamped(c), c["hk"])
        for s, L in enumerate(live):
            assert np.isfinite(p["K"][s, :, :L]).all() and np.isfinite(p["V"][s, :, :L]).all()
            if not c["shared"]:
                assert np.isnan(p["K"][s, :, L:]).all() and np.isnan(p["V"][s, :, L:]).all()
        named = set(p["table_ref"].ravel().tolist())
        spare = [i for i in range(p["Kp"].shape[0]) if i not in named]
        assert len(spare) >= F.SPARE and np.isnan(p["Kp"][spare]).all()
        dead = np.arange(c["max_pages"])[None, :] >= -(-F.clamped(c) // c["page"])[:, None]
        assert np.isin(p["table_dev"][dead], F.JUNK).all() and np.array_equal(p["table_dev"][~dead], p["table_ref"][~dead])


# ------------------------------------------------------------------ wrong models of the operation
MUTATIONS = ["tail_offset", "length", "head_map", "merge_rescale"]


def _model(c, p, mut=None):
    """(O fp16, l f32, m fp16) of a ragged / paged case: per Q slice the partial (m, l, O) of every planned chunk in
    float64, merged with weights exp(m_chunk - max), then rounded to the output types; rows without a key are
    O = 0, l = 0, m = bytes 0xFA.  mut: tail_offset (query i sees keys j <= L - nq + i + 1), length (L - 1 keys),
    head_map (Q head h reads K/V head h % Hk instead of h // g), merge_rescale (of several live chunks of a row
    the one with the lowest max enters the merge with weight 1)."""
    g, nq, hk, d, vd, cap = c["g"], c["nq"], c["hk"], c["d"], c["vd"], c["cap"]
    chunk = F.plan(nq, cap, g)[1]
    b = c["seqs"] * hk * g
    o = np.zeros((b, vd, nq), np.float16)
    l = np.zeros((b, nq), np.float32)
    m = np.full((b, nq), 0xFAFA, np.uint16).view(np.float16)
    for bi in range(b):
        s, h = divmod(bi, hk * g)
        kv = s * hk + (h % hk if mut == "head_map" else h // g)
        L = int(F.clamped(c)[s])
        L = max(L - 1, 0) if mut == "length" else L
        j = np.arange(L)[None, :]
        mask = np.ones((nq, L), bool)
        if c["tail"]:
            mask &= j <= (L - nq + np.arange(nq) + (1 if mut == "tail_offset" else 0))[:, None]
        has = mask.any(axis=1)
        if not has.any():
            continue
        sc = np.where(mask, (p["Q"][bi].astype(np.float64).T @ p["K"][kv, :, :L].astype(np.float64)) / math.sqrt(d), -np.inf)
        v = p["V"][kv, :, :L].astype(np.float64)
        parts = []
        for k0 in range(0, L, chunk):
            sl = slice(k0, min(k0 + chunk, L))
            mc = sc[:, sl].max(axis=1)
            with np.errstate(invalid="ignore"):
                pc = np.where(np.isfinite(mc)[:, None], np.exp(sc[:, sl] - np.where(np.isfinite(mc), mc, 0.0)[:, None]), 0.0)
            parts.append((mc, pc.sum(axis=1), v[:, sl] @ pc.T))
        M = np.max([x[0] for x in parts], axis=0)
        lsum, osum = np.zeros(nq), np.zeros((vd, nq))
        mcs = np.stack([x[0] for x in parts])                                  # [chunks, nq]
        lowest = np.where(np.isfinite(mcs), mcs, np.inf).argmin(axis=0)        # the live chunk furthest below the max
        several = np.isfinite(mcs).sum(axis=0) >= 2
        for ci, (mc, lc, oc) in enumerate(parts):
            live = np.isfinite(mc)
            w = np.where(live, np.exp(np.where(live, mc, 0.0) - np.where(has, M, 0.0)), 0.0)
            if mut == "merge_rescale":
                w = np.where(live & several & (lowest == ci), 1.0, w)
            lsum, osum = lsum + w * lc, osum + w * oc
        m16 = np.where(has, M, 0.0).astype(np.float16)
        l32 = (lsum * np.exp(np.where(has, M, 0.0) - m16.astype(np.float64))).astype(np.float32)
        o16 = (osum / np.where(has, lsum, 1.0)).astype(np.float16)
        o[bi][:, has], l[bi][has], m[bi][has] = o16[:, has], l32[has], m16[has]
    return o, l, m


def _rejected(c, p, got):
    """True / False: test_gpu_ragged._check_ref (and _check_empty on the rows the definition leaves empty), the
    checks of the GPU sweep, reject / accept the result."""
    got = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in got)
    try:
        rg._check_empty(got, F.empty_rows(c))
        rg._check_ref(got, p["Q"], p["K"], p["V"], p["kv_lens"], c["g"], c["tail"])
    except AssertionError:
        return True
    return False


def _applies(c, mut):
    live = F.clamped(c)
    if mut == "tail_offset":
        return c["tail"] and c["nq"] >= 2 and live.max() >= 2
    if mut == "length":                      # (one key of thousands is inside the tolerance: a short sequence)
        return bool(((live >= 1) & (live <= 64)).any())
    if mut == "head_map":
        return c["hk"] == 2 and c["g"] >= 2 and live.max() >= 1
    return live.max() > F.plan(c["nq"], c["cap"], c["g"])[1]


def _small(c):
    return c["seqs"] * c["hk"] * c["g"] * c["nq"] * c["cap"] <= 400_000


# of the first 8 default-range cases a mutation applies to, how many the checker must reject (a dropped key whose
# probability is below the tolerance is no defect an exact computation could see)
MUST_REJECT = {"tail_offset": 8, "length": 8, "head_map": 8, "merge_rescale": 8}


@pytest.mark.parametrize("mut", MUTATIONS)
def test_checker_rejects_a_wrong_model(mut):
    cases = [c for c in DECODE if _applies(c, mut) and _small(c)][:8]
    assert len(cases) == 8
    verdicts = {c["seed"]: _rejected(c, F.build(c), _model(c, F.build(c), mut)) for c in cases}
    print(mut, verdicts)
    assert sum(verdicts.values()) >= MUST_REJECT[mut], f"{mut}: accepted on cases {[s for s, r in verdicts.items() if not r]}"


def test_checker_accepts_the_correct_model_and_the_documented_rounding():
    cases = [c for c in DECODE if _small(c)][:12]
    assert {c["tail"] for c in cases} == {False, True} and {c["entry"] for c in cases} == {"ragged", "paged"}
    for c in cases:
        p = F.build(c)
        assert not _rejected(c, p, _model(c, p)), c["seed"]
        emulated = score_ramp.emulate_ragged_f16(p["Q"], p["K"], p["V"], p["kv_lens"], c["g"], c["tail"])
        assert not _rejected(c, p, emulated), c["seed"]
        ref = ragged_ref.forward_f64(p["Q"], p["K"], p["V"], p["kv_lens"], c["g"], c["tail"])
        assert np.array_equal(~ref[3], F.empty_rows(c))
