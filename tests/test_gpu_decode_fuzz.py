"""Seeded random sweep over the few-query decode forwards against float64: fa_forward_ragged, fa_forward_paged and
(at a lower rate) fa_forward_grouped, the three entry points on the shared key loop of csrc/fa_fwd_f16_core.h.

Every case is drawn from its own seed and lies inside the fused envelope by construction (g first, then nq from the
values with g * pitch <= 128), so no case is skipped or redrawn.  A case draws the entry point, the tail-causal
flag, misaligned pointers, the fold (g, nq: pitches 1 .. 128, all three wave layouts), 1 .. 3 sequences of 1 or 2
K/V heads, d and v_d in 1 .. 128, a capacity up to 2700 keys (half of them multiples of 8; a paged capacity is
page * max_pages) and one length per sequence from a mixture of edges: 0, 1, the capacity, past it, +-1 around a
tile, a planned chunk and a page, nq - 1 and nq under the tail rule.  K and V past each length are NaN: a correct
kernel never lets them through and the reference never reads them.  (Two sequences that share a prefix page keep
its keys finite up to the longer of their lengths.)

The ragged and paged cases go through test_gpu_ragged._check_ref (tests/ragged_ref.py, for the paged form on the
paged_ref.gather'ed cache) and _check_empty; the paged cases are also bitwise fa_forward_ragged on the padded
cache.  The grouped cases go through test_gpu_grouped._grouped_case: run_case's oracle on expanded K / V.

FA_DECODE_FUZZ_N sets the number of cases (300 by default; tests/test_decode_fuzz_draws.py proves on the CPU that
this range holds every kernel instance, staging, pitch class and edge) and FA_DECODE_FUZZ_START the first case of a
slice of a long sweep; FA_DECODE_FUZZ_STATS names a file that receives each case's worst error / allowance
(profiles/decode_fuzz20000.txt)."""
import json
import os

import numpy as np
import pytest

from tests import paged_ref
from tests.test_gpu_fuzz import CHANNELS

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("FA_DECODE_FUZZ_N", "300"))
START = int(os.environ.get("FA_DECODE_FUZZ_START", "0"))
GROUPS = [1, 2, 3, 4, 5, 8, 16, 32, 128]
PAGES = [64, 128, 192, 256]
MAX_CAP = 2700
SPARE = 3                                  # pool pages that no sequence owns
JUNK = [-2 ** 31, -1, 2 ** 31 - 1]         # entries of table pages without a live key
INSTANCES = (32, 64, 128)


def pitch_of(nq):
    p = 1
    while p < nq:
        p *= 2
    return p


def plan(nq, cap, g):
    """(chunks, chunk, pitch) of a ragged / paged call: the chunk formula of include/fa_api.h over keys [0, cap)
    (tests/test_grouped_plan._chunks, which tests/test_ragged_plan.py holds fa_forward_ragged_plan to)."""
    pitch = pitch_of(nq)
    capped = -(-(-(-cap // 64)) // 64) * 64
    chunk = max(capped, 512 if g * pitch <= 64 else 1024)
    return max(-(-cap // chunk), 1), chunk, pitch


def instance_of(d, vd):
    """The D instance that serves (d, v_d)."""
    return next(D for D in INSTANCES if max(d, vd) <= D)


def fast_staging(c):
    """16-byte staging: d == v_d == D, a capacity that is a multiple of 8, aligned K and V."""
    return c["d"] == c["vd"] and c["d"] in INSTANCES and c["cap"] % 8 == 0 and not c["misalign"]


def _length(rng, kind, c, chunk):
    cap, nq, page = c["cap"], c["nq"], c["page"]
    around = lambda unit: unit * int(rng.integers(1, max(cap // unit, 1) + 1)) + int(rng.integers(-1, 2))  # noqa: E731
    if kind == "zero":
        return 0
    if kind == "one":
        return 1
    if kind == "cap":
        return cap
    if kind == "past":
        return cap + int(rng.integers(1, 100))
    if kind == "tile":
        return around(64)
    if kind == "chunk":
        return around(chunk)
    if kind == "page":
        return around(page)
    if kind == "tailq":
        return nq - int(rng.integers(0, 2))
    return int(rng.integers(0, cap + 1))


def draw(i):
    rng = np.random.default_rng(1_000_003 * (i + 1))
    entry = ["ragged", "paged", "grouped"][int(rng.choice(3, p=[0.44, 0.44, 0.12]))]
    tail = bool(rng.random() < 0.5)          # grouped: the causal rule
    misalign = bool(rng.random() < 0.15)
    # g first (g = 1 and 2, the only groups that reach pitches 128 and 64, weighted up), then nq by its pitch
    # class among those with g * pitch <= 128 (the two large classes weighted up), then nq within the class
    lo = 1 if entry == "grouped" else 0
    gw = np.array([3, 2, 1, 1, 1, 1, 1, 1, 1][lo:], dtype=np.float64)
    g = int(GROUPS[lo + int(rng.choice(len(gw), p=gw / gw.sum()))])
    pitches = [p for p in (1, 2, 4, 8, 16, 32, 64, 128) if g * p <= 128]
    pw = np.array([{64: 3.0, 128: 4.0}.get(p, 1.0) for p in pitches])
    pitch = int(pitches[int(rng.choice(len(pitches), p=pw / pw.sum()))])
    nq = int(rng.integers(pitch // 2 + 1, pitch + 1))
    seqs = int(rng.integers(1, 4))
    hk = int(rng.integers(1, 3))
    chans = CHANNELS[:12]
    if rng.random() < 0.4:                   # the 16-byte staging needs d == v_d == D
        d = vd = int(INSTANCES[rng.integers(3)])
    else:                                    # (v_d == d in about 60 % of all cases)
        d = int(chans[rng.integers(len(chans))])
        vd = d if rng.random() < 0.35 else int(chans[rng.integers(len(chans))])
    if entry == "paged":
        page = int(PAGES[rng.integers(len(PAGES))])
        max_pages = int(rng.integers(1, MAX_CAP // page + 1))
        cap = page * max_pages
    else:
        page, max_pages = 0, 0
        cap = int(rng.integers(1, MAX_CAP + 1))
        if rng.random() < (0.75 if d == vd and d in INSTANCES else 0.5):
            cap = max(cap // 8 * 8, 8)
    c = dict(entry=entry, tail=tail, misalign=misalign, g=g, nq=nq, seqs=seqs, hk=hk, d=d, vd=vd, cap=cap, page=page,
             max_pages=max_pages, seed=i)
    chunk = plan(nq, cap, g)[1]
    kinds = ["zero", "one", "cap", "past", "tile", "chunk", "uniform", "uniform", "uniform"]
    kinds += ["page", "page"] if entry == "paged" else []
    kinds += ["tailq", "tailq"] if tail else []
    c["kinds"] = [kinds[rng.integers(len(kinds))] for _ in range(seqs)]
    c["lens"] = [max(_length(rng, k, c, chunk), 0) for k in c["kinds"]]
    c["shared"] = bool(entry == "paged" and seqs >= 2 and rng.random() < 0.35)
    c["mode"] = ["none_front", "scale_end"][int(rng.integers(2))]   # grouped causal rule only
    return c


def _id(i):
    c = draw(i)
    return (f"{i}-{c['entry']}{'-tail' if c['tail'] else ''}-g{c['g']}q{c['nq']}-d{c['d']}v{c['vd']}-s{c['seqs']}x{c['hk']}"
            f"-cap{c['cap']}" + (f"-p{c['page']}" if c["page"] else "")
            + ("" if c["entry"] == "grouped" else "-L" + "_".join(map(str, c["lens"])))
            + ("-shared" if c["shared"] else "") + ("-mis" if c["misalign"] else ""))


def clamped(c):
    return np.clip(np.asarray(c["lens"]), 0, c["cap"])


def build(c):
    """The inputs of a ragged / paged case as numpy arrays: Q [seqs * hk * g, d, nq]; the padded K / V caches
    [seqs * hk, ., cap], NaN past each length; kv_lens, one (unclamped) length per K/V slice; and for the paged form
    the pools, the table the device gets (junk in the entries of pages without a live key) and the table of the
    reference (a valid page in every entry)."""
    rng = np.random.default_rng(c["seed"])
    g, nq, seqs, hk, d, vd, cap, page = (c[n] for n in ("g", "nq", "seqs", "hk", "d", "vd", "cap", "page"))
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    Q, K, V = mk(seqs * hk * g, d, nq), mk(seqs * hk, d, cap), mk(seqs * hk, vd, cap)
    live = clamped(c)
    if c["shared"]:                          # sequences 0 and 1 share their first page
        K[hk:2 * hk, :, :page], V[hk:2 * hk, :, :page] = K[:hk, :, :page], V[:hk, :, :page]
    past = np.arange(cap)[None, :] >= live[:, None]                        # [seqs, cap]
    if c["shared"]:
        past[:2, :page] = np.arange(page)[None, :] >= live[:2].max()
    past = np.repeat(past, hk, axis=0)[:, None, :]
    K, V = np.where(past, np.float16(np.nan), K), np.where(past, np.float16(np.nan), V)
    out = dict(Q=Q, K=K, V=V, kv_lens=np.repeat(np.asarray(c["lens"]), hk))
    if c["entry"] != "paged":
        return out
    max_pages = c["max_pages"]
    num_pages = seqs * max_pages + SPARE
    table = rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)

    def scatter(cache):
        pool = np.full((num_pages, hk, cache.shape[1], page), np.nan, np.float16)
        pool[table] = cache.reshape(seqs, hk, cache.shape[1], max_pages, page).transpose(0, 3, 1, 2, 4)
        return pool

    Kp, Vp = scatter(K), scatter(V)
    if c["shared"]:
        Kp[table[1, 0]] = Vp[table[1, 0]] = np.nan    # sequence 1's own copy is named by no entry any more
        table[1, 0] = table[0, 0]
    dead = np.arange(max_pages)[None, :] >= -(-live // page)[:, None]
    junk = np.asarray(JUNK, dtype=np.int64)[rng.integers(0, 3, table.shape)]
    out.update(Kp=Kp, Vp=Vp, table_ref=table, table_dev=np.where(dead, junk, table).astype(np.int32))
    return out


def empty_rows(c):
    """bool [b, nq], from the definition: the rows of a sequence of (clamped) length L that see no key."""
    L = np.repeat(clamped(c), c["hk"] * c["g"])[:, None]
    last_key = L - c["nq"] + np.arange(c["nq"])[None, :] if c["tail"] else np.broadcast_to(L - 1, (L.shape[0], c["nq"]))
    return (last_key < 0) | (L == 0)


def _grouped(monkeypatch, c):
    from tests.test_gpu_grouped import _grouped_case
    rng = np.random.default_rng(c["seed"])
    g, nq, bkv, d, vd, cap = c["g"], c["nq"], c["seqs"] * c["hk"], c["d"], c["vd"], c["cap"]
    mk = lambda *s: rng.uniform(-2, 2, s).astype(np.float16)  # noqa: E731
    inputs = (mk(bkv * g, d, nq), mk(bkv, d, cap), mk(bkv, vd, cap), np.zeros((bkv * g, vd, nq), np.float16))
    policy, mode = ("causal", c["mode"]) if c["tail"] else ("full", "none_front")
    return _grouped_case(monkeypatch, policy, mode, g, (nq,), (cap,), d, vd, bkv=bkv, misalign=c["misalign"], inputs=inputs)


def run(monkeypatch, i):
    from tests import test_gpu_paged as pg
    from tests import test_gpu_ragged as rg
    c = draw(i)
    if c["entry"] == "grouped":
        return c, _grouped(monkeypatch, c)
    p = build(c)
    g, hk, tail, mis = c["g"], c["hk"], c["tail"], c["misalign"]
    tq = rg._dev(p["Q"], mis)
    if c["entry"] == "ragged":
        st, *got = rg._abi(g, tq, rg._dev(p["K"], mis), rg._dev(p["V"], mis), c["lens"], kv_per_len=hk, tail=tail)
        assert st == 0
        K, V = p["K"], p["V"]
    else:
        st, *got = pg._abi(g, tq, rg._dev(p["Kp"], mis), rg._dev(p["Vp"], mis), p["table_dev"], c["lens"], tail=tail)
        assert st == 0
        K, V = paged_ref.gather(p["Kp"], p["table_ref"], c["page"]), paged_ref.gather(p["Vp"], p["table_ref"], c["page"])
        st, *same = rg._abi(g, tq, rg._dev(K, mis), rg._dev(V, mis), c["lens"], kv_per_len=hk, tail=tail)
        assert st == 0
        assert rg._same(got, same), "paged != ragged on the gathered cache"
    rg._check_empty(got, empty_rows(c))
    return c, rg._check_ref(got, p["Q"], K, V, p["kv_lens"], g, tail)


def _record(c, res):
    stats_file = os.environ.get("FA_DECODE_FUZZ_STATS")
    if stats_file and res:
        with open(stats_file, "a") as f:
            f.write(json.dumps(dict(seed=c["seed"], entry=c["entry"], tail=c["tail"], **{k: float(v) for k, v in res.items()})) + "\n")


@pytest.mark.parametrize("i", range(START, N_CASES), ids=_id)
def test_decode_fuzz_case(monkeypatch, i):
    _record(*run(monkeypatch, i))
