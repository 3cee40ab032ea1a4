"""CPU tests of the FP8-cache / sliding-window sweep (tests/test_gpu_cache_fuzz.py): its default range is not hollow,
its inputs are what its docstring says, and the checkers it relies on reject wrong models of the operation.

Coverage: over draw(0 .. 479) each of the 48 (D instance) x (staging) x (ragged / paged) x (fp16 / FP8) x (full / tail
/ window) cells, every pitch and group under a window, both regimes of the windowed plan, lengths past the capacity,
lo inside a tile and on chunk edges, ragged capacities that are no multiple of 8, both ends of the k_scale exponent
clamp ... each occur at least a stated number of times (the numbers lie under what the draw weights give; if a cell
falls short, the weights change, not the number).

Mutations, in the style of tests/test_decode_fuzz_draws.py: five deliberately wrong float64 chunked models of the
operation, rounded to the output types, go through the sweep's checkers (test_gpu_window._check_window,
test_gpu_ragged._check_ref, _check_empty) and each must be rejected; the unmutated model and the float64 reference
with the documented fp16 roundings (score_ramp.emulate_cache_f16: the window mask and the FP8 split
Q' = fp16(q c2 r), K' = k8 2^e) must pass, at both ends of the exponent clamp and at W = 1 and a large W.  That
acceptance is what makes the sweep's scale ranges legitimate.  Nothing here runs a kernel.

`python -m tests.test_cache_fuzz_draws STATS.jsonl [MORE.jsonl ...]` prints the per-cell table of
profiles/cache_fuzz_default.txt from the files FA_CACHE_FUZZ_STATS names."""

import json
import math
import sys
from collections import Counter

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import paged_ref
from tests import ragged_ref
from tests import score_ramp
from tests import test_gpu_cache_fuzz as F
from tests import test_gpu_decode_fuzz as D
from tests import test_gpu_ragged as rg
from tests import test_gpu_window as gw
from tests import window_ref

N = 480
DRAWS = [F.draw(i) for i in range(N)]
WINDOWED = [c for c in DRAWS if c["mode"] == "window"]
LIVE_W = [c for c in WINDOWED if not F.delegated(c)]          # the windowed kernels proper
FP8 = [c for c in DRAWS if c["cache"] == "fp8"]
REAL = [c for c in FP8 if c["scales"] == "real"]


def _plan(c):
    return F.window_plan(c["nq"], c["cap"], c["g"], c["W"])


def _lo(c):
    return [window_ref.window_lo(L, c["nq"], c["W"], c["cap"]) for L in c["lens"]]


def _live_chunks(c):
    """per sequence, the live launched chunks (L - 1) / chunk - lo / chunk + 1 (0 for an empty one)"""
    chunk = F.case_chunk(c)
    lo = _lo(c) if c["W"] else [0] * c["seqs"]
    return [(L - 1) // chunk - l // chunk + 1 if L > 0 else 0 for L, l in zip(F.clamped(c).tolist(), lo)]


# ------------------------------------------------------------------ the draws
def test_every_case_is_inside_the_envelope():
    for i, c in enumerate(DRAWS):
        assert c["seed"] == i and F.draw(c["seed"]) == c
        assert c["form"] in ("ragged", "paged") and (c["cache"], c["mode"]) in F.COMBOS
        assert c["g"] in F.GROUPS and 1 <= c["nq"] <= 128 and c["g"] * F.pitch_of(c["nq"]) <= 128
        assert 1 <= c["d"] <= 128 and 1 <= c["vd"] <= 128 and 1 <= c["cap"] <= F.MAX_CAP
        assert 1 <= c["seqs"] <= 3 and c["hk"] in (1, 2, 3) and len(c["lens"]) == c["seqs"]
        assert all(0 <= L < 2 ** 31 for L in c["lens"])
        assert c["seqs"] * c["hk"] * c["g"] * c["nq"] * c["cap"] <= max(F.MAX_WORK, c["g"] * c["nq"] * c["cap"])
        if c["form"] == "paged":
            assert c["page"] in F.PAGES and c["cap"] == c["page"] * c["max_pages"]
        assert (1 <= c["W"] <= F.INT32_MAX) == (c["mode"] == "window") and (c["W"] == 0) == (c["mode"] != "window")
        if c["scales"] == "real":
            assert len(c["k_scale"]) == len(c["v_scale"]) == c["hk"]
            assert all(2.0 ** F.K_LOG2[0] * 0.999 <= s <= 2.0 ** F.K_LOG2[1] * 1.001 for s in c["k_scale"])
            assert all(2.0 ** F.V_LOG2[0] * 0.999 <= s <= 2.0 ** F.V_LOG2[1] * 1.001 for s in c["v_scale"])
        assert (c["scales"] != "") == (c["cache"] == "fp8")


def test_the_weights_are_the_issues():
    n = Counter((c["cache"], c["mode"]) for c in DRAWS)
    assert n[("fp16", "window")] == n[("fp8", "window")] == N // 4 and len(WINDOWED) == N // 2
    kinds = Counter(c["scales"] for c in FP8)
    assert 0.25 <= kinds["null"] / len(FP8) <= 0.42 and 0.10 <= kinds["ones"] / len(FP8) <= 0.23 and 0.42 <= kinds["real"] / len(FP8) <= 0.58
    assert 0.10 <= sum(c["misalign"] for c in DRAWS) / N <= 0.20
    beacons = [c for c in DRAWS if c["beacons"]]
    assert len(beacons) >= 4 and all(c["cache"] == "fp16" and all(c["W"] + c["nq"] <= L < c["cap"] for L in c["lens"]) for c in beacons)


def test_the_existing_sweeps_draws_are_unchanged():
    """test_gpu_decode_fuzz.draw is reused here, never edited: a few recorded ids of its default range"""
    for i, want in [(0, "0-paged-g4q27-d128v128-s1x2-cap128-p128-L223"),
                    (7, "7-paged-tail-g2q16-d32v128-s1x1-cap1280-p128-L1"),
                    (123, "123-ragged-tail-g1q5-d128v128-s3x2-cap2632-L2653_2674_1"),
                    (299, "299-paged-tail-g32q1-d16v1-s3x2-cap1024-p256-L0_0_0-shared")]:
        assert D._id(i) == want


def test_window_plan_arithmetic_is_the_librarys():
    """F.window_plan restates what tests/test_window_plan.py brute-forces; here against the library's host-only plan"""
    for c in WINDOWED[:60]:
        assert gw._plan(c["nq"], c["cap"], c["d"], c["vd"], c["g"], c["W"], c["page"] or None) == _plan(c), c["seed"]
        assert _plan(c)[1] == (512 if c["g"] * F.pitch_of(c["nq"]) <= 64 else 1024)


def test_all_48_kernel_instance_cells():
    cells = Counter(F.cell(c) for c in DRAWS if not F.delegated(c))   # (a delegated call runs the twin's kernels)
    want = [(Dd, fast, form, cache, mode) for Dd in F.INSTANCES for fast in (True, False) for form in ("ragged", "paged")
            for cache, mode in F.COMBOS]
    assert len(want) == 48
    for key in want:
        assert cells[key] >= 3, (key, cells[key])


def test_pitches_groups_and_heads():
    pitches = Counter(F.pitch_of(c["nq"]) for c in LIVE_W)
    assert set(pitches) == {1, 2, 4, 8, 16, 32, 64, 128}
    p128 = [c for c in LIVE_W if F.pitch_of(c["nq"]) == 128]
    assert len(p128) >= 8

    def split(c):   # a length within W + 128 keys above a chunk edge: the four waves' windows lie in different chunks
        chunk = F.case_chunk(c)
        return any(L > chunk and 0 < L % chunk < c["W"] + 128 for L in F.clamped(c).tolist())
    assert sum(split(c) for c in p128) >= 3
    for sub in (FP8, LIVE_W):
        assert {c["g"] for c in sub} == set(F.GROUPS) and {c["hk"] for c in sub} == {1, 2, 3}


def test_windowed_plan_regimes():
    assert sum(_plan(c)[0] == _plan(c)[3] for c in LIVE_W) >= 20
    assert sum(_plan(c)[0] < _plan(c)[3] for c in LIVE_W) >= 20
    assert sum(any(0 < n < _plan(c)[0] for n in _live_chunks(c)) for c in LIVE_W) >= 20
    assert sum(max(_live_chunks(c)) >= 2 for c in LIVE_W) >= 40
    assert sum(F.delegated(c) for c in WINDOWED) >= 15
    assert {c["W"] - c["cap"] for c in WINDOWED if F.delegated(c)} >= {0, 17} and any(c["W"] == F.INT32_MAX for c in WINDOWED)
    for kind in set(F.W_KINDS) - {"cap", "cap+17", "max"}:
        assert any(c["w_kind"] == kind for c in LIVE_W), kind
    assert sum(c["W"] + c["nq"] - 1 == c["cap"] for c in LIVE_W) >= 8      # span_w meets the capacity
    assert sum(c["W"] == c["cap"] - 1 for c in LIVE_W) >= 8                 # the last non-delegated window


def test_window_edges():
    assert sum(max(c["lens"]) > c["cap"] for c in LIVE_W) >= 10
    assert sum(any(lo % 64 for lo in _lo(c)) for c in LIVE_W) >= 60
    assert sum(any(lo > 0 and (lo % F.case_chunk(c) == 0 or lo % F.case_chunk(c) == F.case_chunk(c) - 1) for lo in _lo(c))
               for c in LIVE_W) >= 15
    assert sum(any(lo > 0 and lo % 64 == 0 for lo in _lo(c)) for c in LIVE_W) >= 15
    assert sum(0 in F.clamped(c) and F.clamped(c).max() > 0 for c in LIVE_W) >= 15
    some = lambda c: 0 < F.empty_rows(c).sum() and (F.empty_rows(c).any(axis=1) & ~F.empty_rows(c).all(axis=1)).any()  # noqa: E731
    assert sum(some(c) for c in LIVE_W) >= 8
    for off in (-1, 0, 1):                   # lengths at W - 1, W, W + 1 and at W + nq - 1, W + nq
        assert any(c["W"] + off in c["lens"] for c in LIVE_W)
    assert any(c["W"] + c["nq"] - 1 in c["lens"] for c in LIVE_W) and any(c["W"] + c["nq"] in c["lens"] for c in LIVE_W)


def test_ragged_capacities_that_are_no_multiple_of_8():
    odd = [c for c in DRAWS if c["form"] == "ragged" and c["cap"] % 8]
    assert sum(c["cache"] == "fp8" for c in odd) >= 15 and sum(c["mode"] == "window" and not F.delegated(c) for c in odd) >= 15
    # ... of which element-wise staging forced by the row stride alone: d == v_d == D, aligned pointers
    forced = [c for c in odd if c["d"] == c["vd"] and c["d"] in F.INSTANCES and not c["misalign"]]
    assert sum(c["cache"] == "fp8" for c in forced) >= 3 and sum(c["mode"] == "window" for c in forced) >= 3


def test_scales_reach_both_ends_of_the_exponent_clamp():
    e_of = lambda c: [score_ramp.kv8_split(s)[0] for s in c["k_scale"]]  # noqa: E731
    assert sum(-8 in e_of(c) for c in REAL) >= 10 and sum(7 in e_of(c) for c in REAL) >= 10
    # and beyond them, where r leaves [2^-0.5, 2^0.5)
    assert sum(min(c["k_scale"]) < 2.0 ** -8.5 for c in REAL) >= 10 and sum(max(c["k_scale"]) >= 2.0 ** 7.5 for c in REAL) >= 3
    assert sum(len(set(c["k_scale"])) >= 2 and len(set(c["v_scale"])) >= 2 for c in REAL) >= 40
    assert {c["poison"] for c in FP8} == {0x7F, 0xFF}


# ------------------------------------------------------------------ the built inputs
def _finite(x):
    return np.isfinite(fp8_ref.decode(x)) if x.dtype == np.uint8 else np.isfinite(x.astype(np.float32))


def _sample():
    """a few cases of every (form, cache, mode), the beacon and the real-scale cases among them"""
    picked = {}
    for c in DRAWS:
        key = (c["form"], c["cache"], c["mode"], c["beacons"], c["scales"])
        if len(picked.setdefault(key, [])) < 2 and c["seqs"] * c["hk"] * c["cap"] * max(c["d"], c["vd"]) <= 600_000:
            picked[key].append(c)
    return [c for cs in picked.values() for c in cs]


def test_poison_masked_keys_pools_and_junk_entries_lie_where_the_docstring_says():
    sample = _sample()
    assert len(sample) >= 30 and any(c["beacons"] for c in sample)
    for c in sample:
        p = F.build(c)
        hk, cap, nq, W = c["hk"], c["cap"], c["nq"], c["W"]
        live = F.clamped(c)
        for s in range(c["seqs"] * hk):
            L = int(live[s // hk])
            lo = window_ref.window_lo(L, nq, W, cap) if W else 0
            first = lo // 64 * 64
            planted = {lo - 1, L} if c["beacons"] else set()       # (query 0's outer beacon and the last query's)
            for X in (p["K"], p["V"]):
                fin = _finite(X[s])
                assert fin[:, first:L].all(), (c["seed"], "the staged keys, masked ones included, are finite")
                dead = [j for j in list(range(first)) + list(range(L, cap)) if j not in planted]
                assert not fin[:, dead].any(), (c["seed"], "poison below the first staged tile and past the length")
                if c["cache"] == "fp8":
                    assert (X[s][:, dead] == c["poison"]).all()
            if c["beacons"]:
                assert _finite(p["K"][s])[:, lo - 1].all() and lo >= 1
            # what the reference reads is what the kernel reads
            if c["cache"] == "fp8":
                ks, vs = F.scale_arrays(c)
                k = 1.0 if ks is None else float(ks[s % hk])
                assert np.array_equal(p["Kd"][s], fp8_ref.decode(p["K"][s]) * k, equal_nan=True)
                if c["scales"] == "real":    # |true value| <= 2 up to e4m3fn's rounding: 2^-4 relative, or half a
                    v = float(vs[s % hk])    # subnormal step 2^-9 * scale where the scale is that large
                    assert np.nanmax(np.abs(p["Kd"][s]), initial=0.0) <= 2.0 * (1 + 2.0 ** -4) + k * 2.0 ** -10
                    assert np.nanmax(np.abs(p["Vd"][s]), initial=0.0) <= 2.0 * (1 + 2.0 ** -4) + v * 2.0 ** -10
        if c["form"] != "paged":
            continue
        page = c["page"]
        for name in ("K", "V"):
            assert np.array_equal(paged_ref.gather(p[name + "p"], p["table_ref"], page), p[name], equal_nan=c["cache"] == "fp16")
        named = set(p["table_ref"].ravel().tolist())
        spare = [i for i in range(p["Kp"].shape[0]) if i not in named]
        assert len(spare) >= F.SPARE and not _finite(p["Kp"][spare]).any() and not _finite(p["Vp"][spare]).any()
        for s in range(c["seqs"]):             # junk exactly on the pages without a staged key, by brute force
            L = int(live[s])
            first = (window_ref.window_lo(L, nq, W, cap) if W else 0) // 64 * 64
            for pi in range(c["max_pages"]):
                staged = any(first <= j < L for j in range(pi * page, (pi + 1) * page))
                assert (p["table_dev"][s, pi] == p["table_ref"][s, pi]) if staged else (int(p["table_dev"][s, pi]) in F.JUNK)


def test_wide_bytes_hold_every_exponent_code():
    c = next(c for c in FP8 if c["scales"] != "real" and min(F.clamped(c)) >= 1000 and c["d"] >= 32)
    p = F.build(c)
    codes = lambda x: set(((x >> 3) & 15).ravel().tolist())  # noqa: E731
    assert set(range(9)) <= codes(p["K"]) and len(codes(p["V"])) >= 15 and 0 in codes(p["V"])


# ------------------------------------------------------------------ wrong models of the operation
MUTATIONS = ["window_lo", "tile_unmasked", "merge_count", "k_pow2", "scale_head"]


def _model(c, p, mut=None):
    """(O fp16, l f32, m fp16) of a case: per Q slice the partial (m, l, O) of every live chunk of the case's plan
    (absolute multiples of the chunk) in float64 on the dequantized cache, merged with weights exp(m_chunk - max),
    then rounded to the output types; rows without a key are O = 0, l = 0, m = bytes 0xFA.  mut: window_lo (every
    query's lower edge one key lower), tile_unmasked (the lower edge rounded down to the 64-key tile), merge_count
    (the last live chunk left out of the merge), k_pow2 (k_scale replaced by its power-of-two part 2^e), scale_head
    (every head uses head 0's v_scale)."""
    g, nq, hk, d, vd, cap, W = (c[n] for n in ("g", "nq", "hk", "d", "vd", "cap", "W"))
    chunk = F.case_chunk(c)
    b = c["seqs"] * hk * g
    o = np.zeros((b, vd, nq), np.float16)
    l = np.zeros((b, nq), np.float32)
    m = np.full((b, nq), 0xFAFA, np.uint16).view(np.float16)
    fp8 = c["cache"] == "fp8"
    ks, vs = F.scale_arrays(c)
    ks = np.ones(hk) if ks is None else ks.astype(np.float64)
    vs = np.ones(hk) if vs is None else vs.astype(np.float64)
    for bi in range(b):
        s, h = divmod(bi, hk * g)
        head = h // g
        kv = s * hk + head
        L = int(F.clamped(c)[s])
        if W:
            mask = window_ref.window_mask(nq, cap, L, W, lo_shift=-1 if mut == "window_lo" else 0)
            if mut == "tile_unmasked":
                pos = (L - nq + np.arange(nq))[:, None]
                j = np.arange(cap)[None, :]
                mask = (j >= np.maximum(pos - W + 1, 0) // 64 * 64) & (j <= pos) & (pos >= 0) & (j < L)
        else:
            mask = ragged_ref.ragged_mask(nq, cap, L, c["mode"] == "tail")
        has = mask.any(axis=1)
        if not has.any():
            continue
        cols = np.nonzero(mask.any(axis=0))[0]
        j0, j1 = int(cols[0]), int(cols[-1]) + 1
        mask = mask[:, j0:j1]
        k = fp8_ref.decode(p["K"][kv][:, j0:j1]) if fp8 else p["K"][kv][:, j0:j1].astype(np.float64)
        v = fp8_ref.decode(p["V"][kv][:, j0:j1]) if fp8 else p["V"][kv][:, j0:j1].astype(np.float64)
        k = k * (2.0 ** score_ramp.kv8_split(ks[head])[0] if mut == "k_pow2" else ks[head])
        v = v * vs[0 if mut == "scale_head" else head]
        with np.errstate(invalid="ignore"):
            sc = np.where(mask, (p["Q"][bi].astype(np.float64).T @ k) / math.sqrt(d), -np.inf)
            parts = []
            for k0 in range(j0 // chunk * chunk, j1, chunk):
                sl = slice(max(k0, j0) - j0, min(k0 + chunk, j1) - j0)
                mc = sc[:, sl].max(axis=1)
                pc = np.where((mc > -np.inf)[:, None], np.exp(sc[:, sl] - np.where(mc > -np.inf, mc, 0.0)[:, None]), 0.0)
                parts.append((mc, pc.sum(axis=1), v[:, sl] @ pc.T))
            if mut == "merge_count" and len(parts) >= 2:
                parts = parts[:-1]
            M = np.max([x[0] for x in parts], axis=0)
            has = has & (M > -np.inf)
            lsum, osum = np.zeros(nq), np.zeros((vd, nq))
            for mc, lc, oc in parts:
                live = mc > -np.inf
                w = np.where(live & has, np.exp(np.where(live, mc, 0.0) - np.where(has, M, 0.0)), 0.0)
                lsum, osum = lsum + w * lc, osum + np.where(w > 0, w * oc, 0.0)
            m16 = np.where(has, M, 0.0).astype(np.float16)
            l32 = (lsum * np.exp(np.where(has, M, 0.0) - m16.astype(np.float64))).astype(np.float32)
            o16 = (osum / np.where(has & (lsum > 0), lsum, 1.0)).astype(np.float16)
        o[bi][:, has], l[bi][has], m[bi][has] = o16[:, has], l32[has], m16[has]
    return o, l, m


def _rejected(c, p, got):
    """True / False: the checks of the GPU sweep reject / accept the result."""
    got = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in got)
    try:
        rg._check_empty(got, F.empty_rows(c))
        if c["W"]:
            gw._check_window(got, p["Q"], p["Kd"], p["Vd"], p["kv_lens"], c["g"], c["W"])
        else:
            rg._check_ref(got, p["Q"], p["Kd"], p["Vd"], p["kv_lens"], c["g"], c["mode"] == "tail")
    except AssertionError:
        return True
    return False


def _applies(c, mut):
    live = F.clamped(c)
    if mut == "window_lo":
        return c["W"] and not F.delegated(c) and c["W"] <= 32 and max(_lo(c)) >= 1
    if mut == "tile_unmasked":
        return c["W"] and not F.delegated(c) and c["W"] <= 64 and any(lo % 64 for lo in _lo(c))
    if mut == "merge_count":
        return max(_live_chunks(c)) >= 2
    if mut == "k_pow2":
        return c["scales"] == "real" and live.max() >= 1 and \
            all(abs(math.log2(float(score_ramp.kv8_split(s)[1]))) >= 0.25 for s in c["k_scale"])
    return c["scales"] == "real" and c["hk"] >= 2 and live.max() >= 1 and \
        all(abs(s / c["v_scale"][0] - 1.0) >= 0.1 for s in c["v_scale"][1:])


def _small(c):
    return c["seqs"] * c["hk"] * c["g"] * c["nq"] * c["cap"] <= 400_000


# of the first 8 small default-range cases a mutation applies to, how many the checkers must reject
MUST_REJECT = {"window_lo": 8, "tile_unmasked": 8, "merge_count": 8, "k_pow2": 8, "scale_head": 8}


@pytest.mark.parametrize("mut", MUTATIONS)
def test_checkers_reject_a_wrong_model(mut):
    cases = [c for c in DRAWS if _applies(c, mut) and _small(c)][:8]
    assert len(cases) == 8
    verdicts = {}
    for c in cases:
        p = F.build(c)
        verdicts[c["seed"]] = _rejected(c, p, _model(c, p, mut))
    print(mut, verdicts)
    assert sum(verdicts.values()) >= MUST_REJECT[mut], f"{mut}: accepted on cases {[s for s, r in verdicts.items() if not r]}"


def _twelve():
    """12 small default-range cases: the first with k_scale clamped at e = -8 and at e = 7 (beyond the clamp, so r
    leaves [2^-0.5, 2^0.5)), the first at W = 1 and at W >= 512, and the first two of each (cache, mode)."""
    small = [c for c in DRAWS if _small(c) and F.clamped(c).max() >= 1]
    first = lambda f: next(c for c in small if f(c))  # noqa: E731
    picks = [first(lambda c: c["scales"] == "real" and min(c["k_scale"]) < 2.0 ** -8.5 and c["W"] and not F.delegated(c)),
             first(lambda c: c["scales"] == "real" and max(c["k_scale"]) >= 2.0 ** 7.5),
             first(lambda c: c["W"] == 1 and c["cap"] > 64), first(lambda c: 512 <= c["W"] < c["cap"])]
    for combo in F.COMBOS:
        picks += [c for c in small if (c["cache"], c["mode"]) == combo and c not in picks][:2]
    return picks


def test_checkers_accept_the_correct_model_and_the_documented_rounding():
    cases = _twelve()
    assert len(cases) == 12 and {c["form"] for c in cases} == {"ragged", "paged"}
    worst = {}
    for c in cases:
        p = F.build(c)
        assert not _rejected(c, p, _model(c, p)), c["seed"]
        ks, vs = F.scale_arrays(c)
        emulated = score_ramp.emulate_cache_f16(p["Q"], p["K"], p["V"], p["kv_lens"], c["g"], c["mode"] == "tail", c["W"],
                                                ks, vs, c["hk"])
        assert not _rejected(c, p, emulated), c["seed"]
        ref = window_ref.forward_f64(p["Q"], p["Kd"], p["Vd"], p["kv_lens"], c["W"], c["g"]) if c["W"] else \
            ragged_ref.forward_f64(p["Q"], p["Kd"], p["Vd"], p["kv_lens"], c["g"], c["mode"] == "tail")
        assert np.array_equal(~ref[3], F.empty_rows(c))
        worst[c["seed"]] = c["k_scale"]
    print(worst)


def test_the_emulation_without_window_or_fp8_is_the_decode_sweeps():
    c = next(c for c in DRAWS if c["cache"] == "fp16" and _small(c) and F.clamped(c).max() >= 1)
    p = F.build(c)
    finite = np.where(np.isnan(p["K"]), np.float16(0), p["K"]), np.where(np.isnan(p["V"]), np.float16(0), p["V"])
    for tail in (False, True):
        a = score_ramp.emulate_cache_f16(p["Q"], *finite, p["kv_lens"], c["g"], tail)
        b = score_ramp.emulate_ragged_f16(p["Q"], *finite, p["kv_lens"], c["g"], tail)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ------------------------------------------------------------------ the record of a GPU run
def _table(files):
    worst, n = {}, Counter()
    for name in files:
        with open(name) as f:
            for line in f:
                r = json.loads(line)
                key = (r["D"], "fast" if r["fast"] else "elem", r["form"], r["cache"], r["mode"])
                n[key] += 1
                w = worst.setdefault(key, dict(O=0.0, l=0.0, m=0.0))
                for k in w:
                    w[k] = max(w[k], r.get(k, 0.0))
    yield f"{'D':>3s} {'staging':7s} {'form':6s} {'cache':5s} {'mode':6s} {'cases':>5s} {'O':>6s} {'l':>6s} {'m':>6s}"
    for key in sorted(worst):
        w = worst[key]
        yield f"{key[0]:3d} {key[1]:7s} {key[2]:6s} {key[3]:5s} {key[4]:6s} {n[key]:5d} {w['O']:6.3f} {w['l']:6.3f} {w['m']:6.3f}"
    yield f"all: {sum(n.values())} cases, worst O {max(w['O'] for w in worst.values()):.3f}, l " \
          f"{max(w['l'] for w in worst.values()):.3f}, m {max(w['m'] for w in worst.values()):.3f}"


if __name__ == "__main__":
    print("\n".join(_table(sys.argv[1:])))
