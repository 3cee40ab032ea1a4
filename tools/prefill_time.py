"""Query-blocked paged forward against what a caller ran before it, one process, §3.10's method.

For each shape (16 sequences of Hk = 2 K/V heads, capacity 16384, d in {64, 128}, g in {1, 4, 8}, nq in {32, 128, 512}
where one block does not hold the queries, and the b_kv = 1024 control at nq = 128), each page size and each set of
lengths, the same seeded device inputs go alternately through three runs, `--repeats` times each after a warm-up of
all:
  prefill        (a) one fa_forward_paged_prefill call under the tail rule;
  loop           (b) the loop of ceil(nq / P_b) fa_forward_paged calls (the un-blocked twin, whose code is the parent
                 commit's) on Q slices that were made contiguous OUTSIDE the window, each after one device op that
                 shifts k_lens by the queries behind the slice.  The outputs stay in per-slice buffers (a caller
                 would still have to interleave them);
  loop_copy      (b) with the contiguous copy of every Q slice inside the window.
Lengths: every length at the capacity ("full"), and §3.9's seeded uniform lengths ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, loop / prefill, whether (a) beats (b) without the
copies by more than twice the larger of the two spreads (the criterion), the workspace bytes of (a) against the sum
of (b)'s, and whether block qb of (a) has the bits of call qb of (b) where the two plans cut the same chunks.

`--yardstick` adds, at L = nq = cap = 4096, g = 1, the same call against the dense causal forward on the same
values: a ratio, of which nothing is required (the dense forward knows no lengths, table, FP8 cache or GQA fold).

The pools rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.

    python tools/prefill_time.py [--out profiles/prefill_time.json] [--repeats 7] [--window-ms 20] [--yardstick]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import _lib  # noqa: E402

LLC_BYTES = 256 << 20
CAP = 16384
PAGES = (64, 256)
RUNS = ("prefill", "loop", "loop_copy")


def problem(b, nq, cap, d):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, d)


def prefill_plan(g, nq, cap, d, page):
    """(chunks, chunk, P_b, rows, nqb, delegated) of fa_forward_paged_prefill_plan."""
    out = (ctypes.c_int32 * 8)()
    st = _lib.lib().fa_forward_paged_prefill_plan(problem(g, nq, cap, d), g, page, out)
    assert st == 0, _lib.last_error()
    return tuple(out)[:6]


def shapes():
    """The issue's grid without the combinations that one block holds (those calls ARE the twin), then the control."""
    grid = [dict(seqs=16, hk=2, g=g, nq=nq, d=d) for d in (64, 128) for g in (1, 4, 8) for nq in (32, 128, 512)]
    grid = [s for s in grid if not prefill_plan(s["g"], s["nq"], CAP, s["d"], PAGES[0])[5]]
    return grid + [dict(seqs=512, hk=2, g=4, nq=128, d=d, control=True) for d in (64, 128)]


def summarise(times):
    """times: {run: [ms per call of every repeat]} -> the per-run statistics and the criterion."""
    med = {r: statistics.median(v) for r, v in times.items()}
    spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
    out = {r + "_ms": dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r]) for r in times}
    gain = med["loop"] / med["prefill"] - 1.0
    out.update(loop_over_prefill=med["loop"] / med["prefill"], loop_copy_over_prefill=med["loop_copy"] / med["prefill"],
               twice_the_larger_spread=2 * max(spread["prefill"], spread["loop"]),
               prefill_beats_loop=bool(gain > 2 * max(spread["prefill"], spread["loop"])))
    return out


def time_case(s, page, repeats, window_ms):
    import torch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, g, nq, d, control = s["seqs"], s["hk"], s["g"], s["nq"], s["d"], bool(s.get("control", False))
    bkv, b, max_pages = seqs * hk, seqs * hk * g, CAP // page
    chunks, chunk, pb, rows, nqb, delegated = prefill_plan(g, nq, CAP, d, page)
    assert not delegated and nq % pb == 0
    prob = problem(b, nq, CAP, d)
    tprob = problem(b, pb, CAP, d)
    tplan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_paged_plan(tprob, g, page, tplan) == 0 and tplan[0] >= 1
    ws_bytes = int(L.fa_forward_paged_prefill_workspace_bytes(prob, g, page))
    tws_bytes = int(L.fa_forward_paged_workspace_bytes(tprob, g, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * CAP * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    P0 = (rnd(num_pages, hk, d, page), rnd(num_pages, hk, d, page))
    pools = [P0] + [(P0[0].clone(), P0[1].clone()) for _ in range(copies - 1)]
    Q = rnd(b, d, nq)
    Qs = [Q[:, :, q0:q0 + pb].contiguous() for q0 in range(0, nq, pb)]   # made outside the window
    Qc = torch.empty((b, d, pb), dtype=torch.float16, device=dev)        # the copy inside the window
    lens_np = np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    shifted = torch.empty((seqs,), dtype=torch.int32, device=dev)
    out = (torch.empty((b, d, nq), dtype=torch.float16, device=dev), torch.empty((b, nq), dtype=torch.float32, device=dev),
           torch.empty((b, nq), dtype=torch.float16, device=dev))
    touts = [(torch.empty((b, d, pb), dtype=torch.float16, device=dev), torch.empty((b, pb), dtype=torch.float32, device=dev),
              torch.empty((b, pb), dtype=torch.float16, device=dev)) for _ in range(nqb)]
    ws = torch.empty(max(ws_bytes, tws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(run, it, kl):
        Kp, Vp = pools[it % copies]
        if run == "prefill":
            st = L.fa_forward_paged_prefill(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                            max_pages, page, num_pages, kl.data_ptr(), hk, 1, out[0].data_ptr(),
                                            out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws_bytes)
            if st != 0:
                raise RuntimeError(_lib.last_error())
            return
        for qb in range(nqb):
            q0 = qb * pb
            torch.sub(kl, nq - q0 - pb, out=shifted)
            if run == "loop_copy":
                Qc.copy_(Q[:, :, q0:q0 + pb])
                q = Qc
            else:
                q = Qs[qb]
            o, l, m = touts[qb]
            st = L.fa_forward_paged(stream, tprob, g, q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(), max_pages,
                                    page, num_pages, shifted.data_ptr(), hk, 1, o.data_ptr(), l.data_ptr(), m.data_ptr(),
                                    ws.data_ptr(), tws_bytes)
            if st != 0:
                raise RuntimeError(_lib.last_error())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(run, iters, kl):
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            call(run, i, kl)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    res = []
    for name, kl in lens.items():
        iters = {}
        for run in RUNS:  # warm-up of every run, and the calls per window from a first estimate
            window(run, 2, kl)
            iters[run] = max(3, min(400, int(window_ms / max(window(run, 2, kl), 1e-3)) + 1))
        times = {run: [] for run in RUNS}
        for _ in range(repeats):
            for run in RUNS:
                times[run].append(window(run, iters[run], kl))
        call("prefill", 0, kl)
        call("loop", 0, kl)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(out[k][..., qb * pb:(qb + 1) * pb].contiguous().view(torch.uint8),
                                    touts[qb][k].view(torch.uint8))) for qb in range(nqb) for k in range(3))
        res.append(dict(
            sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, control=control, page=page,
            lengths=name, chunks=chunks, chunk_keys=chunk, block_queries=pb, rows=rows, query_blocks=nqb,
            twin_chunks=int(tplan[0]), twin_chunk_keys=int(tplan[1]), kv_copies=copies, calls_per_window=iters,
            **summarise(times), workspace_bytes=ws_bytes, loop_workspace_bytes_sum=nqb * tws_bytes,
            same_chunks=bool(chunk == tplan[1]), block_bits_are_the_loops=same))
    return res


def yardstick(d, repeats, window_ms):
    """L = nq = cap = 4096, g = 1: fa_forward_paged_prefill (tail) against the dense causal forward."""
    import torch
    from tf_flash_attention_amd import flash_attention as fa
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, page, seqs, hk = 4096, 64, 16, 2
    b, max_pages = seqs * hk, n // page
    prob = problem(b, n, n, d)
    gen = torch.Generator(device=dev).manual_seed(77)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    Q, K, V = rnd(b, d, n), rnd(b, d, n), rnd(b, d, n)
    table = torch.arange(seqs * max_pages, dtype=torch.int32, device=dev).reshape(seqs, max_pages)
    to_pool = lambda c: c.view(seqs, hk, d, max_pages, page).permute(0, 3, 1, 2, 4).reshape(-1, hk, d, page).contiguous()  # noqa: E731
    Kp, Vp = to_pool(K), to_pool(V)
    kl = torch.full((seqs,), n, dtype=torch.int32, device=dev)
    ws_bytes = int(L.fa_forward_paged_prefill_workspace_bytes(prob, 1, page))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    out = (torch.empty((b, d, n), dtype=torch.float16, device=dev), torch.empty((b, n), dtype=torch.float32, device=dev),
           torch.empty((b, n), dtype=torch.float16, device=dev))
    stream = torch.cuda.current_stream().cuda_stream

    def call(run):
        if run == "prefill":
            st = L.fa_forward_paged_prefill(stream, prob, 1, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                            max_pages, page, seqs * max_pages, kl.data_ptr(), hk, 1, out[0].data_ptr(),
                                            out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws_bytes)
            if st != 0:
                raise RuntimeError(_lib.last_error())
        else:
            fa.attention_forward("causal", 1, Q, K, V, "none_front")

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(run, iters):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            call(run)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    runs = ("prefill", "dense_causal")
    iters = {}
    for run in runs:
        window(run, 2)
        iters[run] = max(3, min(400, int(window_ms / max(window(run, 2), 1e-3)) + 1))
    times = {run: [] for run in runs}
    for _ in range(repeats):
        for run in runs:
            times[run].append(window(run, iters[run]))
    med = {r: statistics.median(v) for r, v in times.items()}
    dense = fa.attention_forward("causal", 1, Q, K, V, "none_front")[0]
    call("prefill")
    torch.cuda.synchronize()
    return dict(yardstick=True, d=d, n=n, b=b, page=page, plan=prefill_plan(1, n, n, d, page),
                prefill_ms=dict(median=med["prefill"], spread=(max(times["prefill"]) - min(times["prefill"])) / med["prefill"]),
                dense_causal_ms=dict(median=med["dense_causal"],
                                     spread=(max(times["dense_causal"]) - min(times["dense_causal"])) / med["dense_causal"]),
                prefill_over_dense=med["prefill"] / med["dense_causal"],
                max_abs_difference_of_O=float((out[0].float() - dense.float()).abs().max()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--only", help="g,nq,d: one shape of the grid")
    a = ap.parse_args(argv)
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("prefill_time.py: no GPU; timings are only taken on the device")
    res, yard = [], []
    grid = shapes()
    if a.only:
        g, nq, d = (int(x) for x in a.only.split(","))
        grid = [s for s in grid if (s["g"], s["nq"], s["d"]) == (g, nq, d) and not s.get("control")]
    for s in grid:
        for page in PAGES:
            for r in time_case(s, page, a.repeats, a.window_ms):
                res.append(r)
                print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.yardstick:
        for d in (64, 128):
            yard.append(yardstick(d, a.repeats, a.window_ms))
            print(json.dumps(yard[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=res, yardstick=yard,
                           cases_that_miss_the_criterion=[(r["kv_group"], r["nq"], r["d"], r["page"], r["lengths"], r["control"])
                                                          for r in res if not r["prefill_beats_loop"]]), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
