"""Query-blocked and tree-masked MLA attention (mla_paged_prefill_1d) against what a caller could run before it
(DESIGN.md 3.22), by 3.10's method: the runs of a case alternate in ONE process, each timed over windows of whole
calls between two events, `repeats` windows a run, medians and spreads ((max - min) / median) reported.

C / v = 576 / 512, capacity 16384, pages of 64 and 256, a randomly permuted block table, lengths full and random, the
pool rotated over copies that together pass the last-level cache.  Runs of a case:
  new       mla_paged_prefill_1d (with a forest mask where the case has one, else under the tail rule);
  loop      the unmasked tail rule as a loop of mla_paged_1d calls on Q slices of 512 / Hq queries with lengths shifted
            on the device, each slice's O copied into place: what a caller could run before (for a masked case this
            is the cost of the CHAIN of the same length, the nearest thing the loop can compute);
  full      the new call with tail_causal=False (unmasked cases): new / full is what the block ends buy.
The torch composition for a mask (context call + masked attention over the drafts + merge_partials) is not timed here.

    python tools/mla_prefill_time.py [--out profiles/mla_prefill_time.json] [--repeats 5] [--window-ms 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import flash_attention as fa  # noqa: E402

LLC_BYTES = 256 << 20
CAP = 16384
PAGES = (64, 256)
C, V = 576, 512
SCALE = 1.0 / math.sqrt(192)

SHAPES = ([dict(seqs=16, hq=hq, nq=nq, mask=True) for hq in (16, 128) for nq in (8, 64)]
          + [dict(seqs=16, hq=16, nq=nq, mask=False) for nq in (128, 2048)]
          + [dict(seqs=512, hq=16, nq=8, mask=True, control=True)])


def time_case(s, page, repeats, window_ms):
    dev = torch.device("cuda:0")
    seqs, hq, nq, masked = s["seqs"], s["hq"], s["nq"], s["mask"]
    max_pages = CAP // page
    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)
    copies = max(1, min(4, -(-2 * LLC_BYTES // (num_pages * C * page * 2))))
    rng = np.random.default_rng(99)
    table = torch.from_numpy(rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)).to(dev)
    Q = rnd(seqs, hq, C, nq)
    pools = [rnd(num_pages, C, page)]
    pools += [pools[0].clone() for _ in range(copies - 1)]
    mask = None
    if masked:
        parents = np.stack([[rng.integers(-1, i) for i in range(nq)] for _ in range(seqs)])
        mask = fa.draft_mask_from_parents(torch.from_numpy(parents).to(dev))
    step = min(nq, 512 // hq)
    O_loop = torch.empty((seqs, hq, V, nq), dtype=torch.float16, device=dev)
    out = []
    for name, ln in (("full", np.full(seqs, CAP, np.int32)), ("random", rng.integers(nq, CAP + 1, seqs).astype(np.int32))):
        kl = torch.from_numpy(ln).to(dev)

        def call(run, it):
            pool = pools[it % copies]
            if run == "new":
                return fa.mla_paged_prefill_1d(Q, pool, table, kl, V, tail_causal=True, softmax_scale=SCALE, draft_mask=mask)
            if run == "full":
                return fa.mla_paged_prefill_1d(Q, pool, table, kl, V, tail_causal=False, softmax_scale=SCALE)
            for q0 in range(0, nq, step):
                q1 = min(q0 + step, nq)
                O_loop[..., q0:q1] = fa.mla_paged_1d(Q[..., q0:q1], pool, table, kl - (nq - q1), V, tail_causal=True,
                                                     softmax_scale=SCALE)
            return O_loop

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(run, iters):
            torch.cuda.synchronize()
            e0.record()
            for i in range(iters):
                call(run, i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        runs = ("new", "loop") + (() if masked else ("full",))
        iters = {}
        for run in runs:  # warm-up, and the calls per window from a first estimate
            window(run, 1)
            iters[run] = max(2, min(200, int(window_ms / max(window(run, 1), 1e-3)) + 1))
        times = {run: [] for run in runs}
        for _ in range(repeats):
            for run in runs:
                times[run].append(window(run, iters[run]))
        med = {r: statistics.median(v) for r, v in times.items()}
        stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]),  # noqa: E731
                               spread=(max(times[r]) - min(times[r])) / med[r])
        rec = dict(sequences=seqs, heads=hq, nq=nq, masked=masked, control=bool(s.get("control", False)), capacity=CAP,
                   c=C, v=V, page=page, lengths=name, loop_calls=-(-nq // step), pool_copies=copies, calls_per_window=iters,
                   new_ms=stats("new"), loop_ms=stats("loop"), loop_over_new=med["loop"] / med["new"])
        if not masked:
            rec.update(full_ms=stats("full"), new_over_full=med["new"] / med["full"],
                       max_abs_o_difference_new_loop=float((call("new", 0).float() - call("loop", 0).float()).abs().max()))
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("mla_prefill_time.py: no GPU; timings are only taken on the device")
    res = []
    with torch.no_grad():
        for s in SHAPES:
            for page in PAGES:
                for r in time_case(s, page, a.repeats, a.window_ms):
                    res.append(r)
                    print(json.dumps(r), flush=True)
                    if a.out:  # (rewritten after every case: a run that is cut short keeps what it measured)
                        with open(a.out, "w") as f:
                            f.write('{"device": ' + json.dumps(torch.cuda.get_device_name(0)) + ', "cases": [\n')
                            f.write(",\n".join(json.dumps(c) for c in res) + "\n]}\n")
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
