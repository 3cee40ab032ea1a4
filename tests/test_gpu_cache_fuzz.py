"""Seeded random sweep over the FP8-cache and sliding-window decode forwards against float64: the six forms of
{ragged, paged} x {fp16 cache, FP8 cache} x {full, tail, window} that tests/test_gpu_decode_fuzz.py does not draw
(fa_forward_ragged_fp8 / fa_forward_paged_fp8 and the four fa_forward_*_window* entry points).

Every case is drawn from its own seed and lies inside the fused envelope by construction, so no case is skipped or
redrawn.  Case i has form and (cache, mode) number i % 8, so that each of the eight occurs equally often; everything
else is drawn: misaligned pointers (fp16 by one element, FP8 by one byte), the fold (g, nq: pitches 1 .. 128), 1 .. 3
sequences of 1 .. 3 K/V heads, d and v_d in 1 .. 128, a capacity of 1 .. 2700 keys (a paged one is page * max_pages),
the window W from a mixture of edges (1 .. 3, a tile, a chunk of the WINDOWED plan, W + nq - 1 == capacity,
capacity - 1, and the delegated capacity, capacity + 17 and 2^31 - 1), one length per sequence from the decode
sweep's mixture plus, under a window, W - 1 .. W + nq and lengths that put lo = L - nq - W + 1 on a tile edge, a chunk
edge or one key below it, and for an FP8 cache the scales: null pointers, device arrays of 1.0, or per-head values with
k_scale log-uniform in [2^-13, 2^8.5] and v_scale in [2^-8, 2^9].

Inputs: Q ~ U(-2, 2).  With real scales the true K and V ~ U(-2, 2) are quantized by tests/fp8_ref.py and the
reference runs on the dequantized bytes; with unit scales the bytes are test_gpu_fp8_cache._case's "wide" ones (every
exponent code, subnormals included).  Un-windowed, everything at or past each clamped length is poison (NaN; FP8:
0x7F or 0xFF).  Windowed, the keys below floor(lo / 64) * 64 and at or past L are poison and the keys in
[floor(lo / 64) * 64, lo), which the kernels load and mask, stay finite as the contract requires.  Spare pool pages
hold poison; the table entries of pages without a staged key are INT32_MIN, -1 or INT32_MAX.  Half of the eligible
fp16 windowed cases carry window_ref.plant_beacons' keys, planted after the poison.

Checks: status 0; test_gpu_window._check_window (windowed) or test_gpu_ragged._check_ref (un-windowed) against float64
on the cache the kernel sees, and _check_empty on the rows the definition leaves empty: no new tolerance; a paged
result is bitwise the ragged form on the gathered cache; an FP8 result at unit scales is bitwise the fp16 twin on the
converted cache; W >= capacity reports `delegated` and is bitwise the un-windowed tail call; every output of a row
with a key is finite.

FA_CACHE_FUZZ_N sets the number of cases (480 by default; tests/test_cache_fuzz_draws.py proves on the CPU that this
range holds every kernel instance and edge), FA_CACHE_FUZZ_START the first case of a slice of a long sweep, and
FA_CACHE_FUZZ_STATS names a file that receives one JSON line per case (profiles/cache_fuzz_default.txt)."""
import json
import os

import numpy as np
import pytest

from tests import fp8_ref
from tests import paged_ref
from tests import test_gpu_decode_fuzz as D
from tests import window_ref
from tests.test_gpu_fuzz import CHANNELS

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("FA_CACHE_FUZZ_N", "480"))
START = int(os.environ.get("FA_CACHE_FUZZ_START", "0"))
GROUPS, PAGES, MAX_CAP, SPARE, JUNK, INSTANCES = D.GROUPS, D.PAGES, D.MAX_CAP, D.SPARE, D.JUNK, D.INSTANCES
pitch_of, instance_of = D.pitch_of, D.instance_of
COMBOS = [("fp16", "window"), ("fp8", "window"), ("fp8", "full"), ("fp8", "tail")]
MAX_WORK = 750_000                         # seqs * hk * g * nq * cap: the float64 reference's score entries
INT32_MAX = 2 ** 31 - 1
SEED_MUL = 8_000_009                       # (with these weights every cell of test_cache_fuzz_draws.py is met)
K_LOG2, V_LOG2 = (-13.0, 8.5), (-8.0, 9.0)  # the real scales are 2^U of these ranges


def window_plan(nq, cap, g, window):
    """(n_launch, chunk, span_w, cap_chunks, pitch, rows, delegated, 0) of a windowed call: the arithmetic that
    tests/test_window_plan.py holds fa_forward_*_window_plan to, and the twin's plan for W >= capacity."""
    pitch = pitch_of(nq)
    if window >= cap:
        chunks, chunk, _ = D.plan(nq, cap, g)
        return chunks, chunk, cap, chunks, pitch, g * pitch, 1, 0
    span = min(cap, window + nq - 1)
    chunk = max(512 if g * pitch <= 64 else 1024, -(-(-(-span // 64)) // 64) * 64)
    cap_chunks = -(-cap // chunk)
    return min(cap_chunks, (span + chunk - 2) // chunk + 1), chunk, span, cap_chunks, pitch, g * pitch, 0, 0


def case_chunk(c):
    """the chunk of the plan the case runs under"""
    return window_plan(c["nq"], c["cap"], c["g"], c["W"])[1] if c["W"] else D.plan(c["nq"], c["cap"], c["g"])[1]


def fast_staging(c):
    """16-byte (FP8: 8-byte) staging: d == v_d == D, a row stride that is a multiple of 8 keys, aligned K and V."""
    return D.fast_staging(c)


def cell(c):
    """(D instance, fast staging, form, cache, mode); one query under the tail rule runs the full form"""
    mode = "full" if c["mode"] == "tail" and c["nq"] == 1 else c["mode"]
    return instance_of(c["d"], c["vd"]), fast_staging(c), c["form"], c["cache"], mode


def _window(rng, kind, cap, nq, chunk):
    w = {"1": 1, "2": 2, "3": 3, "63": 63, "64": 64, "65": 65, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1,
         "span": cap - nq + 1, "cap-1": cap - 1, "cap": cap, "cap+17": cap + 17, "max": INT32_MAX}.get(kind)
    if w is None:
        w = int(rng.integers(1, max(cap, 2)))
    return max(int(w), 1)


W_KINDS = ["1", "2", "3", "63", "64", "65", "chunk-1", "chunk", "chunk+1", "span", "span", "cap-1", "cap-1", "cap", "cap+17",
           "max", "uniform", "uniform", "uniform", "uniform", "uniform", "uniform"]
WIN_LENGTHS = ["w-1", "w", "w+1", "w+nq-1", "w+nq", "lo_tile", "lo_tile", "lo_chunk", "lo_chunk", "lo_chunk-1", "lo_chunk-1"]


def _length(rng, kind, c, chunk):
    cap, nq, W = c["cap"], c["nq"], c["W"]
    if kind in ("w-1", "w", "w+1", "w+nq-1", "w+nq"):
        return W + {"w-1": -1, "w": 0, "w+1": 1, "w+nq-1": nq - 1, "w+nq": nq}[kind]
    if kind.startswith("lo_"):               # lo = L - nq - W + 1 on a tile edge, a chunk edge or one key below it
        unit = 64 if kind == "lo_tile" else chunk
        room = (cap - nq - W + 1 + (kind == "lo_chunk-1")) // unit
        if room < 1:
            return int(rng.integers(0, cap + 1))
        return unit * int(rng.integers(1, room + 1)) - (kind == "lo_chunk-1") + nq + W - 1
    return D._length(rng, kind, c, chunk)


def draw(i):
    rng = np.random.default_rng(SEED_MUL * (i + 1))
    form = ["ragged", "paged"][i % 2]
    cache, mode = COMBOS[(i // 2) % 4]
    misalign = bool(rng.random() < 0.15)
    gw = np.array([3, 2, 1, 1, 1, 1, 1, 1, 1], dtype=np.float64)
    g = int(GROUPS[int(rng.choice(len(gw), p=gw / gw.sum()))])
    pitches = [p for p in (1, 2, 4, 8, 16, 32, 64, 128) if g * p <= 128]
    pw = np.array([{64: 3.0, 128: 4.0}.get(p, 1.0) for p in pitches])
    pitch = int(pitches[int(rng.choice(len(pitches), p=pw / pw.sum()))])
    nq = int(rng.integers(pitch // 2 + 1, pitch + 1))
    seqs = int(rng.integers(1, 4))
    hk = int(rng.integers(1, 4))
    chans = CHANNELS[:12]
    if rng.random() < 0.4:                   # the fast staging needs d == v_d == D
        d = vd = int(INSTANCES[rng.integers(3)])
    else:
        d = int(chans[rng.integers(len(chans))])
        vd = d if rng.random() < 0.35 else int(chans[rng.integers(len(chans))])
    if form == "paged":
        page = int(PAGES[rng.integers(len(PAGES))])
        max_pages = int(rng.integers(1, MAX_CAP // page + 1))
        cap = page * max_pages
    else:
        page, max_pages = 0, 0
        cap = int(rng.integers(1, MAX_CAP + 1))
        if rng.random() < (0.75 if d == vd and d in INSTANCES else 0.5):
            cap = max(cap // 8 * 8, 8)
    while seqs * hk * g * nq * cap > MAX_WORK and seqs > 1:   # the reference's work, capped in the draw
        seqs -= 1
    while seqs * hk * g * nq * cap > MAX_WORK and hk > 1:
        hk -= 1
    c = dict(form=form, cache=cache, mode=mode, misalign=misalign, g=g, nq=nq, seqs=seqs, hk=hk, d=d, vd=vd, cap=cap,
             page=page, max_pages=max_pages, seed=i, W=0, w_kind="")
    if mode == "window":
        wchunk = 512 if g * pitch <= 64 else 1024    # (the windowed plan's chunk at capacities up to 4096 keys)
        c["w_kind"] = W_KINDS[rng.integers(len(W_KINDS))]
        c["W"] = _window(rng, c["w_kind"], cap, nq, wchunk)
    chunk = case_chunk(c)
    kinds = ["zero", "one", "cap", "past", "tile", "chunk", "uniform", "uniform", "uniform"]
    kinds += ["page", "page"] if form == "paged" else []
    kinds += ["tailq", "tailq"] if mode != "full" else []
    kinds += WIN_LENGTHS if mode == "window" else []
    c["kinds"] = [kinds[rng.integers(len(kinds))] for _ in range(seqs)]
    c["lens"] = [min(max(_length(rng, k, c, chunk), 0), cap + 99) for k in c["kinds"]]
    c["poison"] = int([0x7F, 0xFF][rng.integers(2)])
    c["scales"], c["k_scale"], c["v_scale"] = "", [], []
    if cache == "fp8":
        c["scales"] = ["null", "null", "ones", "real", "real", "real"][rng.integers(6)]
        if c["scales"] == "real":            # (stored as the float32 values the kernels read)
            c["k_scale"] = [float(np.float32(2.0 ** rng.uniform(*K_LOG2))) for _ in range(hk)]
            c["v_scale"] = [float(np.float32(2.0 ** rng.uniform(*V_LOG2))) for _ in range(hk)]
    eligible = cache == "fp16" and all(c["W"] + nq <= L < cap for L in c["lens"])
    c["beacons"] = bool(rng.random() < 0.5) and eligible
    return c


def _id(i):
    c = draw(i)
    return (f"{i}-{c['form']}-{c['cache']}-{c['mode']}" + (f"-W{c['W']}" if c["W"] else "")
            + f"-g{c['g']}q{c['nq']}-d{c['d']}v{c['vd']}-s{c['seqs']}x{c['hk']}-cap{c['cap']}"
            + (f"-p{c['page']}" if c["page"] else "") + "-L" + "_".join(map(str, c["lens"]))
            + (f"-{c['scales']}" if c["scales"] else "") + ("-beacons" if c["beacons"] else "") + ("-mis" if c["misalign"] else ""))


def clamped(c):
    return np.clip(np.asarray(c["lens"]), 0, c["cap"])


def delegated(c):
    return c["mode"] == "window" and c["W"] >= c["cap"]


def lo64(c):
    """per sequence, the first key a windowed kernel stages: lo rounded down to the 64-key tile (0 without a window)"""
    if c["mode"] != "window":
        return np.zeros(c["seqs"], np.int64)
    return np.array([window_ref.window_lo(L, c["nq"], c["W"], c["cap"]) // 64 * 64 for L in c["lens"]], np.int64)


def scale_arrays(c):
    """(k_scale, v_scale) as the call gets them: None (null pointers) or float32 [hk]"""
    if c["scales"] == "real":
        return np.asarray(c["k_scale"], np.float32), np.asarray(c["v_scale"], np.float32)
    if c["scales"] == "ones":
        return np.ones(c["hk"], np.float32), np.ones(c["hk"], np.float32)
    return None, None


def f16_of(b8):
    """an FP8 cache converted to fp16 (exact; the NaN codes stay NaN)"""
    return fp8_ref.decode(b8).astype(np.float16)


def build(c):
    """The inputs of a case as numpy arrays: Q [seqs * hk * g, d, nq] fp16; the padded caches K / V [seqs * hk, ., cap]
    as the kernel's type (fp16, or e4m3fn bytes) with poison where the docstring of this file says; Kd / Vd, what
    the reference reads (the fp16 cache itself, or the dequantized float64 one); kv_lens, one (unclamped) length per
    K/V slice; and for the paged form the pools, the table the device gets (junk in the entries of pages without a
    staged key) and the table of the reference (a valid page in every entry)."""
    rng = np.random.default_rng(c["seed"])
    g, nq, seqs, hk, d, vd, cap, page = (c[n] for n in ("g", "nq", "seqs", "hk", "d", "vd", "cap", "page"))
    Q = rng.uniform(-2, 2, (seqs * hk * g, d, nq)).astype(np.float16)
    live, first = clamped(c), lo64(c)
    j = np.arange(cap)[None, :]
    dead = np.repeat((j < first[:, None]) | (j >= live[:, None]), hk, axis=0)[:, None, :]      # [seqs * hk, 1, cap]
    kv_lens = np.repeat(np.asarray(c["lens"]), hk)
    if c["cache"] == "fp16":
        K, V = (rng.uniform(-2, 2, (seqs * hk, ch, cap)).astype(np.float16) for ch in (d, vd))
        K, V = np.where(dead, np.float16(np.nan), K), np.where(dead, np.float16(np.nan), V)
        if c["beacons"]:
            K, V, _ = window_ref.plant_beacons(Q, K, V, kv_lens, c["W"], g)
        Kd, Vd = K, V
    else:
        K64, V64 = (rng.uniform(-2, 2, (seqs * hk, ch, cap)) for ch in (d, vd))
        byhead = lambda x: x.reshape((seqs, hk) + x.shape[1:])  # noqa: E731
        if c["scales"] == "real":
            K = fp8_ref.quantize(byhead(K64), c["k_scale"], 1).reshape(K64.shape)
            V = fp8_ref.quantize(byhead(V64), c["v_scale"], 1).reshape(V64.shape)
        else:                                # test_gpu_fp8_cache._case's "wide" bytes: every exponent code
            K = fp8_ref.encode(K64.astype(np.float16).astype(np.float64) * np.exp2(-rng.integers(0, 10, K64.shape)))
            V = fp8_ref.encode(V64.astype(np.float16).astype(np.float64) * np.exp2(rng.integers(-8, 8, V64.shape)))
        K, V = np.where(dead, np.uint8(c["poison"]), K), np.where(dead, np.uint8(c["poison"]), V)
        ks, vs = scale_arrays(c)
        one = np.ones(hk, np.float32)
        Kd = fp8_ref.dequantize(byhead(K), one if ks is None else ks, 1).reshape(K.shape)
        Vd = fp8_ref.dequantize(byhead(V), one if vs is None else vs, 1).reshape(V.shape)
    out = dict(Q=Q, K=K, V=V, Kd=Kd, Vd=Vd, kv_lens=kv_lens)
    if c["form"] != "paged":
        return out
    max_pages = c["max_pages"]
    num_pages = seqs * max_pages + SPARE
    table = rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    fill = np.float16(np.nan) if c["cache"] == "fp16" else np.uint8(c["poison"])

    def scatter(cache):
        pool = np.full((num_pages, hk, cache.shape[1], page), fill, cache.dtype)
        pool[table] = cache.reshape(seqs, hk, cache.shape[1], max_pages, page).transpose(0, 3, 1, 2, 4)
        return pool

    p = np.arange(max_pages)[None, :]
    unstaged = ((p + 1) * page <= first[:, None]) | (p * page >= live[:, None])
    junk = np.asarray(JUNK, dtype=np.int64)[rng.integers(0, 3, table.shape)]
    out.update(Kp=scatter(K), Vp=scatter(V), table_ref=table, table_dev=np.where(unstaged, junk, table).astype(np.int32),
               unstaged=unstaged)
    return out


def empty_rows(c):
    """bool [b, nq], from the definition: the rows of a sequence of (clamped) length L that see no key."""
    L = np.repeat(clamped(c), c["hk"] * c["g"])[:, None]
    last_key = np.broadcast_to(L - 1, (L.shape[0], c["nq"])) if c["mode"] == "full" else L - c["nq"] + np.arange(c["nq"])[None, :]
    return (last_key < 0) | (L == 0)


# ------------------------------------------------------------------ the GPU side
def _forward(c, form, cache, window, tail, tq, K, V, table, ks, vs):
    """One of the eight entry points on numpy caches / pools: (O, l, m) device tensors; status 0 asserted."""
    import torch
    from tests import test_gpu_ragged as rg
    from tf_flash_attention_amd import _lib
    L = _lib.lib()
    mis, g, hk = c["misalign"], c["g"], c["hk"]
    b, d, nq = tq.shape
    tk, tv = rg._dev(np.ascontiguousarray(K), mis), rg._dev(np.ascontiguousarray(V), mis)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=tq.device)
    vd = V.shape[-2]
    prob = rg._problem(nq, c["cap"], d, vd, b)
    if form == "ragged":
        shape = []
        need = L.fa_forward_ragged_window_workspace_bytes(prob, g, window) if window else L.fa_forward_ragged_workspace_bytes(prob, g)
    else:
        tt = torch.tensor(np.asarray(table), dtype=torch.int32, device=tq.device)
        shape = [tt.data_ptr(), c["max_pages"], c["page"], K.shape[0]]
        need = L.fa_forward_paged_window_workspace_bytes(prob, g, c["page"], window) if window else \
            L.fa_forward_paged_workspace_bytes(prob, g, c["page"])
    need = int(need)
    O_ = torch.empty((b, vd, nq), dtype=torch.float16, device=tq.device)
    l = torch.empty((b, nq), dtype=torch.float32, device=tq.device)
    m = torch.empty((b, nq), dtype=torch.float16, device=tq.device)
    for t in (O_, l, m):
        t.view(torch.uint8).fill_(0x5A)
    ws = torch.full((max(need, 64),), 0xFF, dtype=torch.uint8, device=tq.device)
    sc = []
    if cache == "fp8":
        tks, tvs = (None if s is None else torch.tensor(s, dtype=torch.float32, device=tq.device) for s in (ks, vs))
        sc = [None if tks is None else tks.data_ptr(), None if tvs is None else tvs.data_ptr()]
    fn = getattr(L, f"fa_forward_{form}" + ("_window" if window else "") + ("_fp8" if cache == "fp8" else ""))
    st = fn(torch.cuda.current_stream().cuda_stream, prob, g, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), *sc, *shape,
            lens.data_ptr(), hk, int(window if window else tail), O_.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == 0, _lib.last_error()
    return O_, l, m


def run(i):
    from tests import test_gpu_ragged as rg
    from tests import test_gpu_window as gw
    c = draw(i)
    p = build(c)
    form, cache, W, g, hk = c["form"], c["cache"], c["W"], c["g"], c["hk"]
    tail = c["mode"] == "tail"
    ks, vs = scale_arrays(c)
    tq = rg._dev(p["Q"], c["misalign"])
    if W:                                    # the plan the call runs under is the one the draw assumed
        assert gw._plan(c["nq"], c["cap"], c["d"], c["vd"], g, W, c["page"] or None) == window_plan(c["nq"], c["cap"], g, W)
    stores = (p["K"], p["V"], None) if form == "ragged" else (p["Kp"], p["Vp"], p["table_dev"])
    got = _forward(c, form, cache, W, tail, tq, *stores, ks, vs)
    if form == "paged":
        same = _forward(c, "ragged", cache, W, tail, tq, paged_ref.gather(p["Kp"], p["table_ref"], c["page"]),
                        paged_ref.gather(p["Vp"], p["table_ref"], c["page"]), None, ks, vs)
        assert rg._same(got, same), "paged != ragged on the gathered cache"
    if cache == "fp8" and c["scales"] != "real":
        twin = _forward(c, form, "fp16", W, tail, tq, f16_of(stores[0]), f16_of(stores[1]), stores[2], None, None)
        assert rg._same(got, twin), "FP8 at unit scales != the fp16 twin on the converted cache"
    if delegated(c):
        assert window_plan(c["nq"], c["cap"], g, W)[6] == 1
        assert rg._same(got, _forward(c, form, cache, 0, True, tq, *stores, ks, vs)), "W >= capacity != the tail call"
    empty = empty_rows(c)
    rg._check_empty(got, empty)
    if W:
        res = gw._check_window(got, p["Q"], p["Kd"], p["Vd"], p["kv_lens"], g, W)
    else:
        res = rg._check_ref(got, p["Q"], p["Kd"], p["Vd"], p["kv_lens"], g, tail)
    o, l, m = (t.float().cpu().numpy() for t in got)
    assert np.isfinite(np.moveaxis(o, 1, 2)[~empty]).all() and np.isfinite(l[~empty]).all() and np.isfinite(m[~empty]).all()
    return c, res


def _record(c, res):
    stats_file = os.environ.get("FA_CACHE_FUZZ_STATS")
    if stats_file and res:
        D_, fast, form, cache, mode = cell(c)
        with open(stats_file, "a") as f:
            f.write(json.dumps(dict(seed=c["seed"], D=D_, fast=fast, form=form, cache=cache, mode=mode,
                                    **{k: float(v) for k, v in res.items()})) + "\n")


@pytest.mark.parametrize("i", range(START, N_CASES), ids=_id)
def test_cache_fuzz_case(i):
    _record(*run(i))
