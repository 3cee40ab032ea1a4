"""Sliding-window prefill over the paged cache against what a caller had before it, one process,
§3.10's method.

For each shape (16 sequences of Hk = 2 K/V heads, capacity 16384, d in {64, 128}, g in {1, 4, 8}, nq in {128, 512,
2048} where one block does not hold the queries, W in {1024, 4096}, and the b_kv = 1024 control at g = 4, nq = 128),
each page size and each set of lengths, the same seeded device inputs go alternately through five runs, `--repeats`
times each after a warm-up of all:
  window_prefill  one fa_forward_paged_window_prefill call;
  loop            (a) the loop of nq / P_b fa_forward_paged_window calls on Q slices that were made contiguous OUTSIDE
                  the timed window, each after one device op that shifts k_lens by the queries behind the slice: the
                  correct-result baseline a caller has without the new call.  The outputs stay in per-slice buffers;
  loop_copy       (a) with the contiguous copy of every Q slice inside the timed window;
  prefill         (b) the un-windowed fa_forward_paged_prefill tail call at the same lengths.  It computes a DIFFERENT
                  result (every query sees the whole prefix) and is there only as the price of not having the window;
  window_cap      (c) fa_forward_paged_window_prefill at W = capacity - 1, which cuts nothing where the lengths stay
                  below the capacity: against (b) it is the overhead of the windowed form.
Lengths: every length at the capacity - 1 ("full"), and §3.9's seeded uniform lengths ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, the ratios loop / window_prefill,
loop_copy / window_prefill, prefill / window_prefill and window_cap / prefill, the tool's run-to-run spread (the larger
of the spreads of window_prefill and loop), whether window_prefill is not slower than (a) without the copies by more
than that spread (the acceptance condition, required where there are at least 4 query blocks), the workspace bytes, and
whether block qb of the new call has the bits of call qb of (a) where the two plans cut the same chunks.

The pools rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.

    python tools/window_prefill_time.py [--out profiles/window_prefill_time.json] [--repeats 7] [--window-ms 20]
                                        [--only g,nq,d,W] [--no-control]

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
WINDOWS = (1024, 4096)
RUNS = ("window_prefill", "loop", "loop_copy", "prefill", "window_cap")


def problem(b, nq, cap, d):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (cap,), d, d)


def plan(g, nq, cap, d, page, window):
    """(launched, chunk, span_w, cap_chunks, P_b, rows, nqb, delegated) of fa_forward_paged_window_prefill_plan."""
    out = (ctypes.c_int32 * 8)()
    st = _lib.lib().fa_forward_paged_window_prefill_plan(problem(g, nq, cap, d), g, page, window, out)
    assert st == 0, _lib.last_error()
    return tuple(out)


def shapes():
    """The issue's grid without the combinations that one block holds (those calls ARE the windowed twin), then the
    control."""
    grid = [dict(seqs=16, hk=2, g=g, nq=nq, d=d, window=w) for d in (64, 128) for g in (1, 4, 8) for nq in (128, 512, 2048)
            for w in WINDOWS]
    grid = [s for s in grid if not plan(s["g"], s["nq"], CAP, s["d"], PAGES[0], s["window"])[7]]
    return grid + [dict(seqs=512, hk=2, g=4, nq=128, d=d, window=1024, control=True) for d in (64, 128)]


def summarise(times, query_blocks):
    """times: {run: [ms per call of every repeat]} -> the per-run statistics, the ratios and the acceptance condition."""
    med = {r: statistics.median(v) for r, v in times.items()}
    spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
    out = {r + "_ms": dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r]) for r in times}
    tool = max(spread["window_prefill"], spread["loop"])
    out.update(loop_over_window_prefill=med["loop"] / med["window_prefill"],
               loop_copy_over_window_prefill=med["loop_copy"] / med["window_prefill"],
               prefill_over_window_prefill=med["prefill"] / med["window_prefill"],
               window_cap_over_prefill=med["window_cap"] / med["prefill"],
               run_to_run_spread=tool,
               not_slower_than_loop=bool(med["window_prefill"] <= med["loop"] * (1.0 + tool)),
               condition_applies=bool(query_blocks >= 4))
    return out


def time_case(s, page, repeats, window_ms):
    import torch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, g, nq, d, W, control = s["seqs"], s["hk"], s["g"], s["nq"], s["d"], s["window"], bool(s.get("control", False))
    bkv, b, max_pages = seqs * hk, seqs * hk * g, CAP // page
    launched, chunk, span_w, cap_chunks, pb, rows, nqb, delegated = plan(g, nq, CAP, d, page, W)
    assert not delegated and nq % pb == 0
    cplan = plan(g, nq, CAP, d, page, CAP - 1)
    assert not cplan[7]
    prob, tprob = problem(b, nq, CAP, d), problem(b, pb, CAP, d)
    tplan = (ctypes.c_int32 * 8)()
    assert L.fa_forward_paged_window_plan(tprob, g, page, W, tplan) == 0 and tplan[0] >= 1 and tplan[6] == 0
    pplan = (ctypes.c_int32 * 8)()
    assert L.fa_forward_paged_prefill_plan(prob, g, page, pplan) == 0 and pplan[0] >= 1
    ws_bytes = int(L.fa_forward_paged_window_prefill_workspace_bytes(prob, g, page, W))
    cws_bytes = int(L.fa_forward_paged_window_prefill_workspace_bytes(prob, g, page, CAP - 1))
    tws_bytes = int(L.fa_forward_paged_window_workspace_bytes(tprob, g, page, W))
    pws_bytes = int(L.fa_forward_paged_prefill_workspace_bytes(prob, g, page))

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
    Qs = [Q[:, :, q0:q0 + pb].contiguous() for q0 in range(0, nq, pb)]   # made outside the timed window
    Qc = torch.empty((b, d, pb), dtype=torch.float16, device=dev)        # the copy inside it
    lens_np = np.random.default_rng(4321).integers(1, CAP, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP - 1, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    shifted = torch.empty((seqs,), dtype=torch.int32, device=dev)
    out = (torch.empty((b, d, nq), dtype=torch.float16, device=dev), torch.empty((b, nq), dtype=torch.float32, device=dev),
           torch.empty((b, nq), dtype=torch.float16, device=dev))
    touts = [(torch.empty((b, d, pb), dtype=torch.float16, device=dev), torch.empty((b, pb), dtype=torch.float32, device=dev),
              torch.empty((b, pb), dtype=torch.float16, device=dev)) for _ in range(nqb)]
    ws = torch.empty(max(ws_bytes, cws_bytes, tws_bytes, pws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def check(st):
        if st != 0:
            raise RuntimeError(_lib.last_error())

    def call(run, it, kl):
        Kp, Vp = pools[it % copies]
        where = (Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(), max_pages, page, num_pages)
        outs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr())
        if run == "window_prefill":
            return check(L.fa_forward_paged_window_prefill(stream, prob, g, Q.data_ptr(), *where, kl.data_ptr(), hk, W, *outs, ws_bytes))
        if run == "window_cap":
            return check(L.fa_forward_paged_window_prefill(stream, prob, g, Q.data_ptr(), *where, kl.data_ptr(), hk, CAP - 1, *outs,
                                                           cws_bytes))
        if run == "prefill":
            return check(L.fa_forward_paged_prefill(stream, prob, g, Q.data_ptr(), *where, kl.data_ptr(), hk, 1, *outs, pws_bytes))
        for qb in range(nqb):
            q0 = qb * pb
            torch.sub(kl, nq - q0 - pb, out=shifted)
            if run == "loop_copy":
                Qc.copy_(Q[:, :, q0:q0 + pb])
                q = Qc
            else:
                q = Qs[qb]
            o, l, m = touts[qb]
            check(L.fa_forward_paged_window(stream, tprob, g, q.data_ptr(), *where, shifted.data_ptr(), hk, W, o.data_ptr(),
                                            l.data_ptr(), m.data_ptr(), ws.data_ptr(), tws_bytes))

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
        call("loop", 0, kl)
        call("window_prefill", 0, kl)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(out[k][..., qb * pb:(qb + 1) * pb].contiguous().view(torch.uint8),
                                    touts[qb][k].view(torch.uint8))) for qb in range(nqb) for k in range(3))
        res.append(dict(
            sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, window=W, control=control, page=page,
            lengths=name, launched_chunks=launched, chunk_keys=chunk, span_w=span_w, cap_chunks=cap_chunks, block_queries=pb,
            rows=rows, query_blocks=nqb, twin_chunks=int(tplan[0]), twin_chunk_keys=int(tplan[1]),
            prefill_chunks=int(pplan[0]), prefill_chunk_keys=int(pplan[1]), kv_copies=copies, calls_per_window=iters,
            **summarise(times, nqb), workspace_bytes=ws_bytes, loop_workspace_bytes_sum=nqb * tws_bytes,
            prefill_workspace_bytes=pws_bytes, same_chunks=bool(chunk == tplan[1]), block_bits_are_the_loops=same))
    return res


def write_out(path, head, res):
    """The JSON file, kept small: the head's fields, the cases' field names once (nested ones dotted) and one row of
    values per case with its times and ratios at four significant digits, then the cases that miss the condition and
    what was not measured.  load() gives the cases back as dicts."""
    def flat(x, pre=""):
        for k, v in x.items():
            if isinstance(v, dict):
                yield from flat(v, pre + k + ".")
            else:
                yield pre + k, float(f"{v:.4g}") if isinstance(v, float) else v
    rows = [dict(flat(r)) for r in res]
    fields = list(rows[0]) if rows else []
    key = lambda r: (r["kv_group"], r["nq"], r["d"], r["window"], r["page"], r["lengths"], r["control"])  # noqa: E731
    tail = dict(cases_that_miss_the_condition=[key(r) for r in res if r["condition_applies"] and not r["not_slower_than_loop"]],
                not_measured=["the ragged entry points", "the FP8 pools", "the call inside a captured graph"])
    with open(path, "w") as f:
        f.write(json.dumps(dict(head, fields=fields))[:-1] + ', "cases": [\n')
        f.write(",\n".join(" " + json.dumps([r[k] for k in fields]) for r in rows))
        f.write("\n], " + json.dumps(tail)[1:] + "\n")


def load(path):
    """The cases of a file that write_out wrote, as the dicts that time_case made (rounded)."""
    with open(path) as f:
        data = json.load(f)
    out = []
    for row in data["cases"]:
        case = {}
        for k, v in zip(data["fields"], row):
            at = case
            *outer, last = k.split(".")
            for o in outer:
                at = at.setdefault(o, {})
            at[last] = v
        out.append(case)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--only", help="g,nq,d,W: one shape of the grid")
    ap.add_argument("--no-control", action="store_true", help="leave the b_kv = 1024 control out")
    a = ap.parse_args(argv)
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    only = None
    if a.only:
        try:
            only = tuple(int(x) for x in a.only.split(","))
        except ValueError:
            only = ()
        if len(only) != 4:
            ap.error("--only takes g,nq,d,W")
    import torch
    if not torch.cuda.is_available():
        sys.exit("window_prefill_time.py: no GPU; timings are only taken on the device")
    res = []
    grid = shapes()
    if only:
        grid = [s for s in grid if (s["g"], s["nq"], s["d"], s["window"]) == only and not s.get("control")]
    if a.no_control:
        grid = [s for s in grid if not s.get("control")]
    for s in grid:
        for page in PAGES:
            for r in time_case(s, page, a.repeats, a.window_ms):
                res.append(r)
                print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        write_out(a.out, dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, window_ms=a.window_ms), res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
