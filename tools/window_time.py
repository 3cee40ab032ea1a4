"""Sliding-window paged decode against what exists without it, one process.

For each shape of §3.10 (16 sequences of Hk = 2 K/V heads, capacity 16384, and the b_kv = 1024 control), each page
size, each window W and each set of lengths, the same seeded device inputs go alternately through three runs,
`--repeats` times each after a warm-up of all:
  window         (a) fa_forward_paged_window on the pools through a randomly permuted block table;
  paged_tail     (b) fa_forward_paged with tail_causal = 1 at the same lengths: it attends every key below the
                 length, so it does MORE work and gives a DIFFERENT result; it is the cost yardstick that shows
                 whether (a)'s time follows the window or the capacity plan;
  gather_ragged  (c) what a caller runs today: inside the window, from the device lengths and table, the positions
                 of each sequence's last W + nq - 1 keys, a torch gather of those keys from the pools into a padded
                 slab [seq, head, c, W + nq - 1 rounded up to 8], and fa_forward_ragged with the tail rule on it.
                 For nq = 1 that is (a)'s result, and the tool checks O against (a)'s under the fp16 forward gate
                 (1e-3 * max(|O|, 1) + 1e-3 * |O|).  For nq > 1 the tail rule on the slab lets query i see i keys
                 more than its window, so (c) is then only close to (a); the worst error / allowance is recorded,
                 not asserted.
Lengths: every length at the capacity ("full"), and §3.9's seeded uniform lengths ("random").
A price check runs W = capacity - 1 at full lengths, (a) against (b) only: the interval form and the relative chunk
index with nothing skipped.
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, (a) / (b), (c) / (a) and whether (a) beats (c) by
more than twice the larger of the two spreads.

The pools rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.

    python tools/window_time.py [--out profiles/window_time.json] [--repeats 7] [--window-ms 20]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import _lib  # noqa: E402

LLC_BYTES = 256 << 20
CAP = 16384
PAGES = (64, 256)
WINDOWS = (1024, 4096)

SHAPES = (
    [dict(seqs=16, hk=2, g=g, nq=nq, d=d) for d in (64, 128) for g in (1, 4, 8) for nq in (1, 4)]
    + [dict(seqs=512, hk=2, g=4, nq=4, d=d, control=True) for d in (64, 128)]
)


def time_case(s, page, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, g, nq, d, control = s["seqs"], s["hk"], s["g"], s["nq"], s["d"], bool(s.get("control", False))
    bkv, b, max_pages = seqs * hk, seqs * hk * g, CAP // page
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (CAP,), d, d)
    twin = (ctypes.c_int32 * 6)()
    assert L.fa_forward_paged_plan(prob, g, page, twin) == 0 and twin[0] >= 1, "shape is outside the fused envelope"
    twin_ws = int(L.fa_forward_paged_workspace_bytes(prob, g, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * CAP * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    table64 = table.long()
    Q = rnd(b, d, nq)
    P0 = (rnd(num_pages, hk, d, page), rnd(num_pages, hk, d, page))
    pools = [P0] + [(P0[0].clone(), P0[1].clone()) for _ in range(copies - 1)]
    lens_np = np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    runs = ["window", "paged_tail", "gather_ragged"]
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in runs}
    l = {r: torch.empty((b, nq), dtype=torch.float32, device=dev) for r in runs}
    m = {r: torch.empty((b, nq), dtype=torch.float16, device=dev) for r in runs}
    stream = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []

    for W in WINDOWS + (CAP - 1,):
        price_check = W == CAP - 1
        plan = (ctypes.c_int32 * 8)()
        assert L.fa_forward_paged_window_plan(prob, g, page, W, plan) == 0 and plan[0] >= 1 and plan[6] == 0
        win_ws = int(L.fa_forward_paged_window_workspace_bytes(prob, g, page, W))
        ws = torch.empty(max(win_ws, twin_ws, 1), dtype=torch.uint8, device=dev)
        span = min(CAP, W + nq - 1)
        span_pad = -(-span // 8) * 8
        slab_prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (span_pad,), d, d)
        slab_ws = int(L.fa_forward_ragged_workspace_bytes(slab_prob, g))
        ws_slab = torch.empty(max(slab_ws, 1), dtype=torch.uint8, device=dev)
        if not price_check:
            Kg = torch.zeros((seqs, hk, d, span_pad), dtype=torch.float16, device=dev)
            Vg = torch.zeros_like(Kg)
        t_idx = torch.arange(span_pad, device=dev)[None, :]

        def gather_call(it, kl):
            Kp, Vp = pools[it % copies]
            start = (kl.long() - span).clamp_(min=0)[:, None]
            pos = (start + t_idx).clamp_(max=CAP - 1)                 # [seqs, span_pad]
            pg = table64.gather(1, pos // page)                       # the pool page of each key
            off = pos % page
            Kg.copy_(Kp[pg, :, :, off].permute(0, 2, 3, 1))           # [seqs, span_pad, hk, d] -> [seqs, hk, d, span_pad]
            Vg.copy_(Vp[pg, :, :, off].permute(0, 2, 3, 1))
            kl2 = kl.clamp(max=span)
            return L.fa_forward_ragged(stream, slab_prob, g, Q.data_ptr(), Kg.data_ptr(), Vg.data_ptr(), kl2.data_ptr(), hk, 1,
                                       O["gather_ragged"].data_ptr(), l["gather_ragged"].data_ptr(),
                                       m["gather_ragged"].data_ptr(), ws_slab.data_ptr(), slab_ws)

        def call(run, it, kl):
            Kp, Vp = pools[it % copies]
            if run == "window":
                st = L.fa_forward_paged_window(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                               max_pages, page, num_pages, kl.data_ptr(), hk, W, O[run].data_ptr(),
                                               l[run].data_ptr(), m[run].data_ptr(), ws.data_ptr(), win_ws)
            elif run == "paged_tail":
                st = L.fa_forward_paged(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                        max_pages, page, num_pages, kl.data_ptr(), hk, 1, O[run].data_ptr(), l[run].data_ptr(),
                                        m[run].data_ptr(), ws.data_ptr(), twin_ws)
            else:
                st = gather_call(it, kl)
            if st != 0:
                raise RuntimeError(_lib.last_error())

        def window(run, iters, kl):
            torch.cuda.synchronize()
            e0.record()
            for i in range(iters):
                call(run, i, kl)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        case_runs = runs[:2] if price_check else runs
        for name, kl in lens.items():
            if price_check and name != "full":
                continue
            iters = {}
            for run in case_runs:  # warm-up of every run, and the calls per window from a first estimate
                window(run, 3, kl)
                iters[run] = max(5, min(400, int(window_ms / max(window(run, 3, kl), 1e-3)) + 1))
            times = {run: [] for run in case_runs}
            for _ in range(repeats):
                for run in case_runs:
                    times[run].append(window(run, iters[run], kl))
            for run in case_runs:
                call(run, 0, kl)
            torch.cuda.synchronize()
            med = {r: statistics.median(v) for r, v in times.items()}
            spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
            stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r])  # noqa: E731
            kl_np = np.full(seqs, CAP, np.int64) if name == "full" else lens_np.astype(np.int64)
            live = int(np.minimum(kl_np, span).sum())  # the keys inside the sequences' windows
            rec = dict(
                sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, control=control, page=page,
                window=W, price_check=price_check, lengths=name, launched_chunks=int(plan[0]), chunk_keys=int(plan[1]),
                span_w=int(plan[2]), capacity_chunks=int(plan[3]), twin_chunks=int(twin[0]), twin_chunk_keys=int(twin[1]),
                workspace_bytes=win_ws, twin_workspace_bytes=twin_ws, kv_copies=copies, calls_per_window=iters,
                **{r + "_ms": stats(r) for r in case_runs},
                window_over_paged_tail=med["window"] / med["paged_tail"],
                kv_bytes_in_windows=2 * hk * d * 2 * live,
                window_bytes_per_s=2 * hk * d * 2 * live / (med["window"] * 1e-3),
            )
            if not price_check:
                ref = O["window"].float()
                err = (O["gather_ragged"].float() - ref).abs()
                allow = 1e-3 * max(float(ref.abs().max()), 1.0) + 1e-3 * ref.abs()
                worst = float((err / allow).max())
                margin = 2 * max(spread["window"], spread["gather_ragged"])
                rec.update(
                    gather_ragged_over_window=med["gather_ragged"] / med["window"],
                    window_beats_gather_by_more_than_twice_the_larger_spread=bool(
                        med["window"] < med["gather_ragged"] * (1.0 - margin)),
                    gather_is_the_same_rule=nq == 1,
                    gather_worst_error_over_allowance=worst,
                    gather_finite=bool(torch.isfinite(O["gather_ragged"].float()).all()),
                )
            out.append(rec)
        del ws, ws_slab
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("window_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        for page in PAGES:
            for r in time_case(s, page, a.repeats, a.window_ms):
                res.append(r)
                print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=res), f, indent=1)
            f.write("\n")
    # (c) with one query is (a)'s rule: it must agree under the gate
    same = [r for r in res if r.get("gather_is_the_same_rule")]
    return 0 if all(r["gather_worst_error_over_allowance"] <= 1.0 and r["gather_finite"] for r in same) else 1


if __name__ == "__main__":
    sys.exit(main())
