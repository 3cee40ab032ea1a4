#!/usr/bin/env python3
"""Compare two builds of the library over the host side of the C ABI: every *_plan and *_workspace_bytes export, and
the forward, backward-split and append entry points called only in ways that return before any device call (b == 0, a
bad argument, a null or one-byte-short workspace, a null k_lens / table / pool / mask, a misaligned pool).  Per call:
the status (or size), the fa_last_error() text of a refusal, and the whole out[].  Needs no GPU.

    tools/abi_parity.py OLD.so [NEW.so]      (NEW: the library beside the package; exit status 1 on any difference)

The grid is dtype x seq_dims x policy x nq x nk x group x page x window x (d, v_d) x b below, whole for every plan and
workspace export of an fp16 / 1d / full problem.  Outside fp16 / 1d / full the decode and MLA exports refuse on that
axis, so there the inner axes are thinned (THIN) instead of repeating the refusal; the forwards run their modes
(DECODE_MODES, MLA_MODES) over a thinned window and (d, v_d) axis, all of them at b == group and two at the other b.
The sweep is split over the CPUs; it stops at 20 differences.
"""
import ctypes
import itertools
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tf_flash_attention_amd import _lib  # noqa: E402

P, ODD = ctypes.c_void_p(256), ctypes.c_void_p(264)  # a pointer no call here may follow, and a misaligned one
NQ = (0, 1, 2, 3, 5, 16, 17, 64, 65, 128, 129, 2048, 2049, 100000)
NK = (0, 1, 63, 64, 65, 511, 512, 513, 1024, 2047, 2048, 2049, 4160, 65536, 1 << 20, 1 << 30)
GROUP = (0, 1, 2, 3, 8, 16, 17, 64, 128, 129)
PAGE = (0, 1, 32, 64, 128, 192)
DV = ((64, 64), (128, 64), (64, 128), (192, 128), (576, 512), (600, 512), (96, 96), (512, 576))
THIN = dict(nq=(0, 1, 129), nk=(0, 2048, 4160), g=(0, 1, 3), dv=DV[:1] + DV[4:5], page=(0, 64))
# the ways a forward is called, each refused (or empty) before the launch whatever else holds: a null workspace, one a
# byte short, or a null / misaligned pointer.  (workspace, bytes short, ...pointers, ..., max_pages off by, num_pages)
DECODE_MODES = (  # (.., k_lens, table, pools, mask, kv_per_len, ..)
    (None, 0, P, P, P, P, 1, 0, 9), (P, 1, P, P, P, P, 1, 0, 9), (P, 0, None, P, P, P, 1, 0, 9), (None, 0, P, P, P, P, 3, 0, 9),
    (P, 0, P, None, P, P, 1, 0, 9), (P, 0, P, P, None, P, 1, 0, 9), (P, 0, P, P, P, None, 1, 0, 9), (None, 0, P, P, P, P, 1, 1, 9),
    (None, 0, P, P, P, P, 1, 0, 0))
MLA_MODES = (  # (.., Q, k_lens, table, pool, softmax_scale, tail_causal, mask, ..)
    (None, 0, P, P, P, P, .1, 1, None, 0, 9), (P, 1, P, P, P, P, .1, 1, None, 0, 9), (P, 0, None, P, P, P, .1, 1, None, 0, 9),
    (P, 0, P, None, P, P, .1, 1, None, 0, 9), (P, 0, P, P, None, P, .1, 1, None, 0, 9), (P, 0, P, P, P, None, .1, 1, None, 0, 9),
    (P, 0, P, P, P, ODD, .1, 1, None, 0, 9), (None, 0, P, P, P, P, 0., 1, None, 0, 9), (None, 0, P, P, P, P, float("inf"), 1, None, 0, 9),
    (None, 0, P, P, P, P, float("nan"), 1, None, 0, 9), (None, 0, P, P, P, P, .1, 0, P, 0, 9), (None, 0, P, P, P, P, .1, 1, P, 0, 9),
    (None, 0, P, P, P, P, .1, 1, None, 1, 9), (None, 0, P, P, P, P, .1, 1, None, 0, 0))
calls, diffs, SHARD = 0, [], (0, 1)


def both(libs, fn, *args, out=False):
    """Call fn in both libraries and record a difference in (result, refusal text, out[])."""
    global calls
    got = []
    for L in libs:
        f = getattr(L, fn)
        buf = (ctypes.c_int32 * 8)(*[-7] * 8) if out else ()
        r = f(*args, buf) if out else f(*args)
        got.append((r, L.fa_last_error() if r != 0 and f.restype is ctypes.c_int else b"", tuple(buf)))
    calls += 1
    if got[0] != got[1]:
        show = [tuple(getattr(a, n) if n[1:] != "_seq" else tuple(getattr(a, n)) for n, _ in a._fields_)
                if isinstance(a, _lib.FaProblem) else getattr(a, "value", a) for a in args]
        diffs.append(f"{fn}{tuple(show)}: {got[0]} != {got[1]}")
        if len(diffs) == 20:
            report("stopped at 20 differences")
    # (the smaller size and plan of the two: a "short" workspace or an "active" plan then is so in both libraries)
    return min(got[0][0], got[1][0]), got[0][1], tuple(map(min, got[0][2], got[1][2]))


class Stop(Exception):
    pass


def report(how):
    raise Stop(how)


def mine(items):
    """this process's share of a sweep: every SHARD[1]-th item from the SHARD[0]-th"""
    return itertools.islice(items, SHARD[0], None, SHARD[1])


def windows(nk, thin):
    return sorted({0, 64, nk} if thin else {0, 1, 63, 64, 1000, nk - 1, nk, nk + 1})


def problems(libs, core_only=False):
    """(problem, is_core) over dtype x dims x policy x nq x nk x (d, v_d); LOCAL takes the window axis as window_size."""
    for dt, dims, pol in itertools.product((_lib.F16, _lib.F32), (1, 2), (_lib.FULL, _lib.CAUSAL, _lib.LOCAL)):
        core = dt == _lib.F16 and dims == 1 and pol == _lib.FULL
        if core_only is not None and core_only != core:
            continue
        ax = THIN if core_only is False else dict(nq=NQ, nk=NK, dv=DV)
        for (d, vd), nq, nk in mine(itertools.product(ax["dv"], ax["nq"], ax["nk"])):
            for w in (windows(nk, core_only is False) if pol == _lib.LOCAL else (1,)):
                yield _lib.make_problem(dt, pol, dims, _lib.NONE_FRONT, 1, (nq,) if dims == 1 else (2, nq),
                                        (nk,) if dims == 1 else (2, nk), d, vd, window_size=w), core


def with_b(p, g):
    for b in (0, max(g, 0), max(g, 0) + 1):
        p.b = b
        yield b


def sweep_dense(libs):
    """The split, split-backward and grouped exports, which take every dtype, dims and policy."""
    for p, _ in problems(libs, None):
        plans = [both(libs, f, p, out=True) for f in ("fa_forward_split_plan", "fa_backward_split_plan", "fa_backward_split_q_plan")]
        for b in with_b(p, 1):
            both(libs, "fa_forward_workspace_bytes", p)
            need = both(libs, "fa_backward_split_workspace_bytes", p)[0]
            if b == 0 or plans[0][2][0] > 0:  # (no plan and b > 0: the plain forward, which launches)
                both(libs, "fa_forward_ws", None, p, *[None] * 6, P, max(both(libs, "fa_forward_workspace_bytes", p)[0] - 1, 0))
            if b == 0 or plans[1][2][0] > 0 or plans[2][2][0] > 0:
                both(libs, "fa_backward_split", None, p, *[None] * 10, P, max(need - 1, 0))
                both(libs, "fa_backward_split", None, p, *[None] * 10, None, need)
        for g in GROUP:
            both(libs, "fa_forward_grouped_plan", p, g, out=True)
            for b in with_b(p, g):
                need = both(libs, "fa_forward_grouped_workspace_bytes", p, g)[0]
                if b == 0 or g >= 2:  # (kv_group == 1 is fa_forward_ws, above)
                    both(libs, "fa_forward_grouped", None, p, g, *[None] * 6, P, max(need - 1, 0))
                    both(libs, "fa_forward_grouped", None, p, g, *[None] * 6, None, need)


def paged_axis(p, thin):
    """(page, max_pages) with the capacity as it is and, where it differs, rounded up to a multiple of the page"""
    nk = p.k_seq[0]
    for page in (THIN["page"] if thin else PAGE):
        for cap in sorted({nk, -(-nk // page) * page if page else nk}):
            if cap > 1 << 30:  # (fa_validate's next_pow2 does not return for an extent in (2^30, 2^31), in either library)
                continue
            p.k_seq[0] = cap
            yield page, cap // page if page else 1
    p.k_seq[0] = nk


def sweep_decode(libs, p, thin):
    """The twelve decode forwards' exports, and both MLA forms', over group x page x window x b."""
    for cache, form, g in itertools.product(_lib.DECODE_CACHES, _lib.DECODE_FORMS, THIN["g"] if thin else GROUP):
        plan, ws, fwd = _lib.decode_entry_points(cache, form, False)
        for page, maxp in (paged_axis(p, thin) if cache == "paged" else ((None, None),)):
            for w in (windows(p.k_seq[0], False) if "window" in form else (None,)):
                own = (p, g) + ((page,) if page is not None else ()) + ((w,) if w is not None else ())
                both(libs, plan, *own, out=True)
                light = w in (None, 0, 64, p.k_seq[0]) and (p.d, p.v_d) in (DV[0], DV[3], DV[4])  # (the forwards' thinner grid)
                for b in with_b(p, g):
                    need = both(libs, ws, *own)[0]
                    modes = () if not light else DECODE_MODES if b == g else DECODE_MODES[:3:2]
                    for fp8, (ws_p, short, lens, table, pool, mask, kvpl, dmax, nump) in itertools.product((False, True), modes):
                        if (page is None and (table is None or pool is None or dmax or not nump)) or (form != "tree" and mask is None):
                            continue  # (a mode of another cache or form: here it would reach the launch)
                        tab = (table, maxp + dmax, page, nump) if page is not None else ()
                        both(libs, fwd + ("_fp8" if fp8 else ""), None, p, g, P, pool, pool, *((None, None) if fp8 else ()), *tab, lens,
                             kvpl, mask if form == "tree" else 1 if w is None else w, P, P, P, ws_p, max(need - short, 0))
    for blocked, heads in itertools.product((False, True), THIN["g"] if thin else GROUP):
        stem = "fa_forward_mla_paged" + ("_prefill" if blocked else "")
        for page, maxp in paged_axis(p, thin):
            both(libs, stem + "_plan", p, heads, page, out=True)
            for b in with_b(p, heads):
                need = both(libs, stem + "_workspace_bytes", p, heads, page)[0]
                modes = MLA_MODES if b == heads and (p.d >= 512 or (p.d, p.v_d) == DV[0]) else MLA_MODES[:4:3]
                for fp8, (ws_p, short, q, lens, table, pool, scale, tail, mask, dmax, nump) in itertools.product((False, True), modes):
                    if mask is not None and not blocked:
                        continue
                    both(libs, stem + ("_fp8" if fp8 else ""), None, p, heads, q, pool, table, maxp + dmax, page, nump, lens, tail,
                         scale, *((None,) if fp8 else ()), *((mask,) if blocked else ()), P, P, P, ws_p, max(need - short, 0))


def sweep_append(libs):
    """The six appends: a null K_new, k_lens or table refuses every call that is not refused or empty before."""
    for seqs, heads, (d, vd), n_new, nk, page, nump, (new, lens, table) in mine(itertools.product(
            (-1, 0, 3), (0, 1, 8), DV[:2] + ((0, 0),), (-1, 0, 1, 17), NK, PAGE, (0, 9), ((None, P, P), (P, None, P), (P, P, None)))):
        maxp = nk // page if page else 1
        for fp8 in (False, True):
            sc, x = ((None, None) if fp8 else ()), "_fp8" if fp8 else ""
            if page == 64 and nump and table is not None:
                both(libs, "fa_append_ragged" + x, None, seqs, heads, d, vd, n_new, nk, new, new, P, P, *sc, lens, P)
            both(libs, "fa_append_paged" + x, None, seqs, heads, d, vd, n_new, nk, new, new, P, P, *sc, table, maxp, page, nump, lens, P)
            both(libs, "fa_append_mla_paged" + x, None, seqs, d, n_new, nk, new, P, *sc[:1], table, maxp, page, nump, lens, P)


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    jobs = min(16, os.cpu_count() or 1)
    with multiprocessing.Pool(jobs) as pool:  # (the sweep is Python-bound: one share of every axis product a process)
        parts = pool.map(work, [(i, jobs) for i in range(jobs)])
    found = [d for _, ds, _ in parts for d in ds]
    print(f"{sum(n for n, _, _ in parts)} calls compared ({', '.join(sorted({how for _, _, how in parts}))}), {len(found)} differences")
    print("\n".join(found[:20]))
    sys.exit(1 if found else 0)


def work(shard):
    global SHARD
    SHARD = shard
    try:
        with _lib.using(sys.argv[1]) as old, _lib.using(sys.argv[2] if len(sys.argv) == 3 else _lib.LIB_PATH) as new:
            libs = (old, new)
            sweep_dense(libs)
            for thin in (False, True):
                for p, _ in problems(libs, not thin):
                    sweep_decode(libs, p, thin)
            sweep_append(libs)
            for nq, cap, seqs in mine(iter(((2048, 4096, 1 << 22), (1, 65536, 1 << 26)))):  # a launch grid of 2^31 workgroups or more
                p = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, seqs * 16, (nq,), (cap,), 576, 512)
                for stem in ("fa_forward_mla_paged", "fa_forward_mla_paged_prefill"):
                    both(libs, stem, None, p, 16, None, None, None, cap // 64, 64, 9, None, 1, .07,
                         *((None,) if "prefill" in stem else ()), None, None, None, ctypes.c_void_p(1), 1 << 62)
        return calls, diffs, "the whole grid"
    except Stop as s:
        return calls, diffs, str(s)


if __name__ == "__main__":
    main()
