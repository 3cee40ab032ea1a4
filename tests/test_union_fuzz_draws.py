"""CPU tests of the combined / grouped gradient sweep (tests/test_gpu_union_fuzz.py): its default range is not hollow,
and its gate rejects wrong models of the two operations.  Nothing here runs a kernel; the plan functions are host
arithmetic.

Coverage: over draw(0 .. 239) every cell the sweep exists for occurs at least twice: combined cases of every dtype x
channel class (<= 64, 65..128, 129..256, 288) x {1d, 2d}; every policy as a part in every dtype; parts of one case under
different sync modes; 8 parts; a row empty in one part but not in the union; a row empty in the union; offsets 6 or
more apart between two parts that share a non-empty row; v_d != d in fp16; a part that takes the split-key forward, the
backward's key-chunk dQ plan, the backward's query-chunk plan; grouped cases fused and expanded, of each dtype, in 2d,
with Hk = 1, with v_d != d, with a leading batch axis.  If a cell falls short the draw's weights or PRIME change, never
a seed.

Mutations: five wrong results, computed in float64 from the reference's own pieces and rounded to the case's types,
go through test_gpu_union_fuzz.check, the gate the GPU results go through:
  a  every part's gradients from that part's own (l_i, m_i): the composition of the parts' forwards with constant
     weights, whose gradient through each normaliser is dropped (test_gpu_merge's
     test_user_composition_drops_the_normaliser_gradient)
  b  dQ without the last non-empty part's dQ_i
  c  the rules of parts 0 and 1 exchanged (part 0's rule on part 1's keys and the reverse)
  d  grouped: query head h reads K/V head h % Hk, not h // g
  e  grouped: dK / dV without the group's last member
a, b and c apply to a case with two parts that share a non-empty row (c also needs the exchange to change the mask), d
and e to every grouped case (g >= 2), d only with Hk >= 2.  The unmutated reference, rounded the same way, passes in
every case, and every mutation is rejected in at least half of the default cases it applies to, per dtype.  The half is
a floor, not a measurement: a part 12 below another in score hides under the absolute tolerance, legitimately.
Measured shares of rejected / applicable cases over the default range (printed by test_mutations_are_rejected):
  a  fp16 48/56  fp32 27/27  fp64 29/29        d  fp16 38/38  fp32 17/17  fp64 19/19
  b  fp16 48/56  fp32 26/27  fp64 29/29        e  fp16 60/60  fp32 30/30  fp64 30/30
  c  fp16 41/43  fp32 25/25  fp64 19/19

`python -m tests.test_union_fuzz_draws STATS.jsonl [MORE.jsonl ...]` prints the table of
profiles/union_fuzz_default.txt from the files FA_UNION_FUZZ_STATS names."""
import ctypes
import functools
import json
import sys
from collections import Counter

import numpy as np

from tests import test_gpu_union_fuzz as F
from tests import union_ref
from tf_flash_attention_amd import _lib

N = 240
DRAWS = [F.draw(i) for i in range(N)]
COMBINED = [c for c in DRAWS if c["kind"] == "combined"]
GROUPED = [c for c in DRAWS if c["kind"] == "grouped"]
DTYPES = (np.float16, np.float32, np.float64)
_name = lambda t: np.dtype(t).name  # noqa: E731


def _rows(c):
    """bool [parts, nq]: the rows with a key, per part"""
    return np.stack([mk.any(axis=1) for mk in F.masks(c)])


def _shared(c):
    """the pairs of parts that share a non-empty row"""
    rows = _rows(c)
    return [(i, j) for i in range(len(rows)) for j in range(i + 1, len(rows)) if (rows[i] & rows[j]).any()]


def _plans(c, part):
    """(split-key forward chunks, key-chunk dQ chunks, query-chunk dK/dV chunks) of one part's own problem"""
    L = _lib.lib()
    dt = {np.float16: _lib.F16, np.float32: _lib.F32, np.float64: _lib.F64}[c["dtype"]]
    prob = _lib.make_problem(dt, {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}[part["policy"]], c["seq"],
                             {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}[part["mode"]],
                             F.slices(c), c["qs"], part["ks"], c["d"], c["vd"], part["ws"], part["ls"], part["causal"])
    out = []
    for fn in (L.fa_forward_split_plan, L.fa_backward_split_plan, L.fa_backward_split_q_plan):
        buf = (ctypes.c_int32 * 4)()
        assert fn(prob, buf) == _lib.FA_OK, _lib.last_error()
        out.append(int(buf[0]))
    return tuple(out)


# ------------------------------------------------------------------ the draws
def test_every_case_is_what_the_sweep_says():
    for i, c in enumerate(DRAWS):
        assert c["seed"] == i and F.draw(i) == c
        assert c["kind"] == ("combined", "grouped")[i % 2] and c["dtype"] == F.DTYPES[(i // 2) % 4]
        assert c["d"] in F.CH and c["vd"] in F.CH and F.ch_class(c["vd"]) <= F.ch_class(c["d"])
        assert len(c["qs"]) == c["seq"] and all(len(p["ks"]) == c["seq"] and min(p["ks"]) >= 1 for p in c["parts"])
        assert c["split"] or (1 <= c["qs"][0] <= 300 if c["seq"] == 1 else 1 <= min(c["qs"]) and max(c["qs"]) <= 16)
        assert F.work(c) <= F.MAX_WORK, (i, F.work(c))
        if c["kind"] == "combined":
            assert 1 <= len(c["parts"]) <= 8 and len(c["batch"]) == 1 and c["batch"][0] in (1, 2)
            assert any(p["delta"] == 0 for p in c["parts"]) and all(p["delta"] in F.DELTAS for p in c["parts"])
            if c["split"]:
                assert c["dtype"] == np.float16 and max(c["d"], c["vd"]) <= 64 and c["batch"] == (1,) and c["seq"] == 1
                assert (c["qs"], 2100) == ((33,), max(p["ks"][0] for p in c["parts"])) if c["split"] == "k" else \
                    c["qs"] == (2300,) and any(p["ks"] == (16,) and p["policy"] == "full" for p in c["parts"])
        else:
            assert c["g"] in F.GROUPS and c["hk"] in (1, 2, 3) and len(c["deltas"]) == c["hk"] and len(c["parts"]) == 1
            assert c["batch"] in ((), (1,), (2,))
            assert (F.grouped_plan_chunks(c) > 0) == c["fused"], i    # the library's plan agrees with the draw
        if c["d"] == 1:
            assert all(p["delta"] == 0 for p in c["parts"]) and not any(c.get("deltas", []))


def test_the_weights_are_the_issues():
    assert sum(c["dtype"] == np.float16 for c in DRAWS) == N // 2 and sum(c["dtype"] == np.float32 for c in DRAWS) == N // 4
    assert 0.6 <= sum(c["seq"] == 1 for c in DRAWS) / N <= 0.8
    assert 0.08 <= sum(c["misalign"] for c in DRAWS) / N <= 0.22
    assert 0.3 <= sum(c["d"] != c["vd"] for c in DRAWS) / N <= 0.5
    assert 0 < sum(bool(c["split"]) for c in DRAWS) < 0.1 * N
    n = Counter(len(c["parts"]) for c in COMBINED)
    assert n[8] >= 0.05 * len(COMBINED) and n[2] + n[3] >= 0.5 * len(COMBINED) and set(n) == set(range(1, 9))
    assert 0.35 <= sum(len(c["batch"]) == 1 for c in GROUPED) / len(GROUPED) <= 0.65
    assert {c["g"] for c in GROUPED} == set(F.GROUPS)
    offsets = Counter(abs(p["delta"]) for c in COMBINED for p in c["parts"])
    assert set(offsets) == {0, 1, 3, 6, 12}


def test_the_inputs_carry_the_offsets():
    for c in (COMBINED[3], COMBINED[8], GROUPED[4], GROUPED[9]):
        p = F.build(c)
        assert all(x.dtype == c["dtype"] for x in [p["Q"], p["dO"]] + p["Ks"] + p["Vs"])
        lead = len(c["batch"]) + (c["kind"] == "grouped")
        Q, Ks = F._flat(p["Q"], lead).astype(np.float64), [F._flat(x, lead).astype(np.float64) for x in p["Ks"]]
        assert np.abs(Q).max() <= 2 and np.abs(p["dO"].astype(np.float64)).max() <= 2
        if c["d"] == 1:
            continue
        assert (Q[:, 0] == 2).all()
        for j, K in enumerate(Ks):
            deltas = np.repeat([c["parts"][j]["delta"]], K.shape[0]) if c["kind"] == "combined" else \
                np.tile(c["deltas"], K.shape[0] // c["hk"])
            shift = 2 * K[:, 0] / np.sqrt(c["d"])                  # what channel 0 adds to every score of the slice
            assert np.allclose(shift, deltas[:, None], rtol=2.0 ** -10, atol=0)
            assert np.abs(K[:, 1:]).max() <= 2


def test_combined_cells():
    cells = Counter((_name(c["dtype"]), F.ch_class(max(c["d"], c["vd"])), c["seq"]) for c in COMBINED)
    for dt in DTYPES:
        for cls in range(4):
            for seq in (1, 2):
                assert cells[(_name(dt), cls, seq)] >= 2, (_name(dt), cls, seq, cells[(_name(dt), cls, seq)])
    pols = Counter((_name(c["dtype"]), pol) for c in COMBINED for pol in {p["policy"] for p in c["parts"]})
    assert all(pols[(_name(dt), pol)] >= 2 for dt in DTYPES for pol in F.POLICIES), pols
    assert sum(len({p["mode"] for p in c["parts"]}) >= 2 for c in COMBINED) >= 2
    assert sum(len(c["parts"]) == 8 for c in COMBINED) >= 2
    rows = [_rows(c) for c in COMBINED]
    assert sum(bool(((~r).any(axis=0) & r.any(axis=0)).any()) for r in rows) >= 2    # empty in one part, not in the union
    assert sum(bool((~r.any(axis=0)).any()) for r in rows) >= 2                        # empty in the union
    apart = lambda c: any(abs(c["parts"][i]["delta"] - c["parts"][j]["delta"]) >= 6 for i, j in _shared(c))  # noqa: E731
    assert sum(apart(c) for c in COMBINED) >= 2
    assert sum(c["dtype"] == np.float16 and c["d"] != c["vd"] for c in COMBINED) >= 2


def test_split_cells():
    plans = [_plans(c, p) for c in COMBINED if c["split"] for p in c["parts"]]
    for k, name in enumerate(("fa_forward_split_plan", "fa_backward_split_plan", "fa_backward_split_q_plan")):
        assert sum(pl[k] >= 2 for pl in plans) >= 2, (name, plans)


def test_grouped_cells():
    assert sum(c["fused"] for c in GROUPED) >= 2 and sum(not c["fused"] for c in GROUPED) >= 2
    # ... and the expanded cases of the fused forward's own kind (fp16, at most 128 channels) lie past the envelope
    assert sum(not c["fused"] and c["dtype"] == np.float16 and max(c["d"], c["vd"]) <= 128 for c in GROUPED) >= 2
    for dt in DTYPES:
        assert sum(c["dtype"] == dt for c in GROUPED) >= 2
    assert sum(c["seq"] == 2 for c in GROUPED) >= 2 and sum(c["hk"] == 1 for c in GROUPED) >= 2
    assert sum(c["hk"] >= 2 for c in GROUPED) >= 2 and sum(c["d"] != c["vd"] for c in GROUPED) >= 2
    assert sum(len(c["batch"]) == 1 for c in GROUPED) >= 2 and sum(c["batch"] == (2,) for c in GROUPED) >= 2
    assert sum(c["fused"] and c["seq"] == 2 for c in GROUPED) >= 1 and sum(len(set(c["deltas"])) >= 2 for c in GROUPED) >= 2


# ------------------------------------------------------------------ wrong models of the operations
MUTATIONS = ("a", "b", "c", "d", "e")


def _as_result(c, r, dQ=None, dKs=None, dVs=None):
    """a float64 reference (or pieces of one) as the result a kernel would store for it"""
    T = c["dtype"]
    o, l, m = union_ref.stored(r, T)
    cast = lambda xs: [x.astype(T) for x in xs]  # noqa: E731
    return dict(O=o, l=l, m=m, dQ=(r["dQ"] if dQ is None else dQ).astype(T), dKs=cast(r["dKs"] if dKs is None else dKs),
                dVs=cast(r["dVs"] if dVs is None else dVs))


def _swapped_masks(c):
    """mutation c: part 0's rule on part 1's keys and the reverse; None where that changes nothing"""
    if len(c["parts"]) < 2:
        return None
    p0, p1 = c["parts"][:2]
    from oracle import fa_oracle as O
    mk = F.masks(c)
    new = [O.problem_mask(F.problem(c, p1), c["qs"], p0["ks"]), O.problem_mask(F.problem(c, p0), c["qs"], p1["ks"])] + mk[2:]
    return None if all(np.array_equal(x, y) for x, y in zip(new, mk)) else new


def applies(c, mut):
    if mut in "abc":
        return c["kind"] == "combined" and bool(_shared(c)) and (mut != "c" or _swapped_masks(c) is not None)
    return c["kind"] == "grouped" and c["g"] >= 2 and (mut == "e" or c["hk"] >= 2)


def mutated(c, p, ref, mut):
    """the mutated result of a case the mutation applies to, in check()'s shapes"""
    T = c["dtype"]
    lead = len(c["batch"]) + (c["kind"] == "grouped")
    Q, dO = F._flat(p["Q"], lead), F._flat(p["dO"], lead).astype(np.float64)
    Ks, Vs = [F._flat(x, lead) for x in p["Ks"]], [F._flat(x, lead) for x in p["Vs"]]
    if mut == "a":
        mk = F.masks(c)
        dQ, dKs, dVs = np.zeros_like(ref["dQ"]), [], []
        safe = np.where(ref["ha"][None, :], ref["L"], 1.0)
        for K, V, m_ in zip(Ks, Vs, mk):
            _, Li, Mi, hai = union_ref.part_statistics(Q, K, V, m_)
            w = np.where(hai[None, :], Li * np.exp(np.where(hai[None, :], Mi - ref["M"], 0.0)), 0.0) / safe
            r = union_ref.union(Q, [K], [V], w[:, None, :] * dO, [m_], 0.0, 0.0)
            dQ += r["dQ"]; dKs.append(r["dKs"][0]); dVs.append(r["dVs"][0])
        return _as_result(c, ref, dQ, dKs, dVs)
    if mut == "b":
        last = int(np.nonzero(_rows(c).any(axis=1))[0][-1])
        return _as_result(c, ref, ref["dQ"] - ref["dQ_parts"][last])
    if mut == "c":
        return _as_result(c, union_ref.union(Q, Ks, Vs, dO, _swapped_masks(c), 0.0, 0.0))
    g, hk = c["g"], c["hk"]
    if mut == "d":
        s = np.arange(Q.shape[0])
        kv = s // (hk * g) * hk + s % (hk * g) % hk             # the K/V slice Q slice s wrongly reads
        r = union_ref.union(Q, [Ks[0][kv]], [Vs[0][kv]], dO, F.masks(c), 0.0, 0.0)
        dK, dV = np.zeros(Ks[0].shape), np.zeros(Vs[0].shape)
        np.add.at(dK, kv, r["dKs"][0]); np.add.at(dV, kv, r["dVs"][0])
        return _as_result(c, r, dKs=[dK], dVs=[dV])
    return _as_result(c, ref, dKs=[ref["dK"] - ref["dKe"][:, g - 1]], dVs=[ref["dV"] - ref["dVe"][:, g - 1]])


def _rejected(c, ref, got):
    try:
        F.check(c, ref, got)
    except AssertionError:
        return True
    return False


@functools.lru_cache(maxsize=None)
def verdicts():
    """{"ref": [the cases whose unmutated reference the gate rejects], mutation: {dtype: [rejected, applicable]}}"""
    out = {"ref": [], **{mut: {_name(dt): [0, 0] for dt in DTYPES} for mut in MUTATIONS}}
    for c in DRAWS:
        p = F.build(c)
        ref = F.reference(c, p)
        if _rejected(c, ref, _as_result(c, ref)):
            out["ref"].append(c["seed"])
        for mut in MUTATIONS:
            if applies(c, mut):
                tally = out[mut][_name(c["dtype"])]
                tally[1] += 1
                tally[0] += _rejected(c, ref, mutated(c, p, ref, mut))
    return out


def test_the_unmutated_reference_passes_in_every_case():
    assert verdicts()["ref"] == []


def test_mutations_are_rejected():
    v = verdicts()
    for mut in MUTATIONS:
        print(mut, "  ".join(f"{dt} {r}/{n}" for dt, (r, n) in v[mut].items()))
    for mut in MUTATIONS:
        for dt, (r, n) in v[mut].items():
            assert n >= 8, (mut, dt, n)
            assert 2 * r >= n, f"mutation {mut}, {dt}: rejected in {r} of {n} cases"


# ------------------------------------------------------------------ the record of a GPU run
TENSORS = ("O", "l", "l_plain", "m", "dQ", "dK", "dV")


def _table(files):
    worst, n = {}, Counter()
    for name in files:
        with open(name) as f:
            for line in f:
                r = json.loads(line)
                key = (r["kind"], r["dtype"])
                n[key] += 1
                w = worst.setdefault(key, {k: (0.0, -1) for k in TENSORS + ("dQ_slope", "dK_slope", "dV_slope")})
                for k in w:
                    if abs(r.get(k, 0.0)) > abs(w[k][0]):
                        w[k] = (r[k], r["seed"])
    yield "worst error / bound of every tensor and worst slope of every gradient, with the seed it occurred at"
    yield f"{'kind':8s} {'dtype':7s} {'cases':>5s} " + " ".join(f"{k:>14s}" for k in TENSORS) + " " + \
        " ".join(f"{k + ' slope':>18s}" for k in ("dQ", "dK", "dV"))
    for key in sorted(worst):
        w = worst[key]
        yield f"{key[0]:8s} {key[1]:7s} {n[key]:5d} " + " ".join(f"{w[k][0]:6.3f} @{w[k][1]:<6d}" for k in TENSORS) + " " + \
            " ".join(f"{w[k + '_slope'][0]:10.2e} @{w[k + '_slope'][1]:<6d}" for k in ("dQ", "dK", "dV"))
    yield f"all: {sum(n.values())} cases"


if __name__ == "__main__":
    print("\n".join(_table(sys.argv[1:])))
