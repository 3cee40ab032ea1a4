"""Paged few-query forward against the ragged forward on a gathered cache, one process.

For each shape of §3.9 (16 sequences of Hk = 2 K/V heads, capacity 16384, and the b_kv = 1024 control), each page
size and each set of lengths, the same seeded device inputs go alternately through three runs, `--repeats` times
each after a warm-up of all:
  paged          (a) fa_forward_paged on the pools through a randomly permuted block table;
  ragged         (b) fa_forward_ragged on the ALREADY gathered padded cache: the same plan, tiles and staged values,
                 so (a) / (b) is the price of the table, and the results are compared bit for bit;
  gather_ragged  (c) what a caller runs today: the gather inside the window — torch.index_select of every
                 sequence's pages from the pools and the layout copy [seq, page, head, c, key] -> [seq, head, c,
                 page, key] into the padded cache — then (b).  The index tensor is built outside the window.
Lengths: every length at the capacity ("full"), and §3.9's seeded uniform lengths ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, (a) / (b) and whether it stays within twice the
larger of the two spreads, (c) / (a), and whether (a)'s bits are (b)'s.

The pools and the padded caches rotate over several copies, so a call does not find its keys in the 256 MB
last-level cache left by the call before.

    python tools/paged_time.py [--out profiles/paged_time.json] [--repeats 7] [--window-ms 30]

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
    plan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_paged_plan(prob, g, page, plan) == 0 and plan[0] >= 1, "shape is outside the fused envelope"
    ws_bytes = int(L.fa_forward_paged_workspace_bytes(prob, g, page))
    assert ws_bytes == int(L.fa_forward_ragged_workspace_bytes(prob, g))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * CAP * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    index = table.reshape(-1).long()

    def to_pool(cache):  # [bkv, d, CAP] -> [num_pages, hk, d, page] through the table
        pool = torch.zeros((num_pages, hk, d, page), dtype=torch.float16, device=dev)
        pool[index] = cache.view(seqs, hk, d, max_pages, page).permute(0, 3, 1, 2, 4).reshape(-1, hk, d, page)
        return pool

    Q = rnd(b, d, nq)
    K0, V0 = rnd(bkv, d, CAP), rnd(bkv, d, CAP)
    padded = [(K0, V0)] + [(K0.clone(), V0.clone()) for _ in range(copies - 1)]
    P0 = (to_pool(K0), to_pool(V0))
    pools = [P0] + [(P0[0].clone(), P0[1].clone()) for _ in range(copies - 1)]
    Kg, Vg = torch.empty_like(K0), torch.empty_like(V0)  # the gather's output
    lens_np = np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    runs = ["paged", "ragged", "gather_ragged"]
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in runs}
    l = {r: torch.empty((b, nq), dtype=torch.float32, device=dev) for r in runs}
    m = {r: torch.empty((b, nq), dtype=torch.float16, device=dev) for r in runs}
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def ragged(run, K, V, kl):
        return L.fa_forward_ragged(stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), kl.data_ptr(), hk, 0,
                                   O[run].data_ptr(), l[run].data_ptr(), m[run].data_ptr(), ws.data_ptr(), ws_bytes)

    def gather(pool, out):
        out.view(seqs, hk, d, max_pages, page).copy_(
            pool.index_select(0, index).view(seqs, max_pages, hk, d, page).permute(0, 2, 3, 1, 4))

    def call(run, it, kl):
        if run == "paged":
            Kp, Vp = pools[it % copies]
            st = L.fa_forward_paged(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(), max_pages,
                                    page, num_pages, kl.data_ptr(), hk, 0, O[run].data_ptr(), l[run].data_ptr(),
                                    m[run].data_ptr(), ws.data_ptr(), ws_bytes)
        elif run == "ragged":
            st = ragged(run, *padded[it % copies], kl)
        else:
            Kp, Vp = pools[it % copies]
            gather(Kp, Kg)
            gather(Vp, Vg)
            st = ragged(run, Kg, Vg, kl)
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

    out = []
    for name, kl in lens.items():
        iters = {}
        for run in runs:  # warm-up of every run, and the calls per window from a first estimate
            window(run, 3, kl)
            iters[run] = max(5, min(400, int(window_ms / max(window(run, 3, kl), 1e-3)) + 1))
        times = {run: [] for run in runs}
        for _ in range(repeats):
            for run in runs:
                times[run].append(window(run, iters[run], kl))
        for run in runs:
            call(run, 0, kl)
        torch.cuda.synchronize()
        bits = lambda x, y: all(bool(torch.equal(t[x].view(torch.uint8), t[y].view(torch.uint8))) for t in (O, l, m))  # noqa: E731
        med = {r: statistics.median(v) for r, v in times.items()}
        spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
        stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r])  # noqa: E731
        price = med["paged"] / med["ragged"] - 1.0
        live = CAP * seqs if name == "full" else int(lens_np.astype(np.int64).sum())
        out.append(dict(
            sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, control=control, page=page,
            max_pages=max_pages, num_pages=num_pages, lengths=name, chunks=int(plan[0]), chunk_keys=int(plan[1]),
            kv_copies=copies, calls_per_window=iters, **{r + "_ms": stats(r) for r in runs},
            paged_over_ragged=med["paged"] / med["ragged"], table_price=price,
            price_within_twice_the_larger_spread=bool(price <= 2 * max(spread["paged"], spread["ragged"])),
            gather_ragged_over_paged=med["gather_ragged"] / med["paged"],
            paged_beats_gather_ragged=bool(med["paged"] < med["gather_ragged"]),
            paged_bits_are_ragged=bits("paged", "ragged"), gathered_bits_are_ragged=bits("gather_ragged", "ragged"),
            kv_bytes_below_lengths=2 * hk * d * 2 * live,
            paged_live_bytes_per_s=2 * hk * d * 2 * live / (med["paged"] * 1e-3),
        ))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("paged_time.py: no GPU; timings are only taken on the device")
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
    return 0 if all(r["paged_bits_are_ragged"] and r["gathered_bits_are_ragged"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
