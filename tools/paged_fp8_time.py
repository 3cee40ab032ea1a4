"""Paged few-query forward over FP8 (e4m3fn) pools against the fp16 pools, one process.

tools/paged_time.py's method on §3.10's shapes (16 sequences of Hk = 2 K/V heads, capacity 16384, and the b_kv = 1024
controls): for each shape, page size and set of lengths, the same keys go alternately through three runs,
`--repeats` times each after a warm-up of all:
  fp8      (a) fa_forward_paged_fp8 on the FP8 pools, k_scale and v_scale read from device arrays;
  fp16     (b) fa_forward_paged on fp16 pools that hold the same values (the FP8 pools converted, which is exact);
  dequant  (c) what a caller with an FP8 cache runs today: the pools converted to fp16 in torch inside the window
           (one dtype-converting copy per pool into a preallocated fp16 pool), then (b) on the result.
The scales are 1.0 in both arrays, so that (a)'s bits can be checked against (b)'s; the kernels load and apply them
whatever their value.  A caller with real scales needs a multiply after the conversion as well; (c) leaves it out,
in (c)'s favour.
Lengths: every length at the capacity ("full"), and §3.9's seeded uniform lengths ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, (a) / (b) and (c) / (a), and whether each difference
exceeds twice the larger of the two spreads (the project's rule for a difference that counts).

The pools rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the call
before; the FP8 pools are half the bytes, so they rotate over twice as many.

    python tools/paged_fp8_time.py [--out profiles/paged_fp8_time.json] [--repeats 7] [--window-ms 30]

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
from tf_flash_attention_amd.flash_attention import quantize_kv_fp8  # noqa: E402

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

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv16_bytes = 2 * bkv * d * CAP * 2
    copies16 = max(1, min(8, -(-2 * LLC_BYTES // kv16_bytes)))
    copies8 = max(1, min(16, -(-4 * LLC_BYTES // kv16_bytes)))
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    index = table.reshape(-1).long()
    ones = torch.ones(hk, dtype=torch.float32, device=dev)

    def to_pool8(cache):  # fp16 [bkv, d, CAP] -> e4m3fn [num_pages, hk, d, page] through the table, at scale 1.0
        c8, _ = quantize_kv_fp8(cache.view(seqs, hk, d, CAP), head_axis=1, scale=ones)
        pool = torch.zeros((num_pages, hk, d, page), dtype=torch.uint8, device=dev)
        pool[index] = c8.view(torch.uint8).view(seqs, hk, d, max_pages, page).permute(0, 3, 1, 2, 4).reshape(-1, hk, d, page)
        return pool.view(torch.float8_e4m3fn)

    Q = rnd(b, d, nq)
    P8 = (to_pool8(rnd(bkv, d, CAP)), to_pool8(rnd(bkv, d, CAP)))
    pools8 = [P8] + [(P8[0].clone(), P8[1].clone()) for _ in range(copies8 - 1)]
    P16 = (P8[0].to(torch.float16), P8[1].to(torch.float16))  # the same keys: e4m3fn -> fp16 is exact
    pools16 = [P16] + [(P16[0].clone(), P16[1].clone()) for _ in range(copies16 - 1)]
    Kd, Vd = torch.empty_like(P16[0]), torch.empty_like(P16[1])  # the dequantization's output
    lens_np = np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    runs = ["fp8", "fp16", "dequant"]
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in runs}
    l = {r: torch.empty((b, nq), dtype=torch.float32, device=dev) for r in runs}
    m = {r: torch.empty((b, nq), dtype=torch.float16, device=dev) for r in runs}
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def paged16(run, Kp, Vp, kl):
        return L.fa_forward_paged(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(), max_pages,
                                  page, num_pages, kl.data_ptr(), hk, 0, O[run].data_ptr(), l[run].data_ptr(),
                                  m[run].data_ptr(), ws.data_ptr(), ws_bytes)

    def call(run, it, kl):
        if run == "fp8":
            Kp, Vp = pools8[it % copies8]
            st = L.fa_forward_paged_fp8(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), ones.data_ptr(),
                                        ones.data_ptr(), table.data_ptr(), max_pages, page, num_pages, kl.data_ptr(), hk, 0,
                                        O[run].data_ptr(), l[run].data_ptr(), m[run].data_ptr(), ws.data_ptr(), ws_bytes)
        elif run == "fp16":
            st = paged16(run, *pools16[it % copies16], kl)
        else:
            Kp, Vp = pools8[it % copies8]
            Kd.copy_(Kp)
            Vd.copy_(Vp)
            st = paged16(run, Kd, Vd, kl)
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
        live = CAP * seqs if name == "full" else int(lens_np.astype(np.int64).sum())
        out.append(dict(
            sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, control=control, page=page,
            max_pages=max_pages, num_pages=num_pages, lengths=name, chunks=int(plan[0]), chunk_keys=int(plan[1]),
            fp8_copies=copies8, fp16_copies=copies16, calls_per_window=iters, **{r + "_ms": stats(r) for r in runs},
            fp8_over_fp16=med["fp8"] / med["fp16"],
            fp8_beats_fp16_by_twice_the_larger_spread=bool(1.0 - med["fp8"] / med["fp16"] > 2 * max(spread["fp8"], spread["fp16"])),
            dequant_over_fp8=med["dequant"] / med["fp8"],
            fp8_beats_dequant_by_twice_the_larger_spread=bool(1.0 - med["fp8"] / med["dequant"] > 2 * max(spread["fp8"], spread["dequant"])),
            fp8_bits_are_fp16=bits("fp8", "fp16"), dequant_bits_are_fp16=bits("dequant", "fp16"),
            fp8_kv_bytes_below_lengths=2 * hk * d * live,
            fp8_live_bytes_per_s=2 * hk * d * live / (med["fp8"] * 1e-3),
            fp16_live_bytes_per_s=2 * hk * d * 2 * live / (med["fp16"] * 1e-3),
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
        sys.exit("paged_fp8_time.py: no GPU; timings are only taken on the device")
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
    return 0 if all(r["fp8_bits_are_fp16"] and r["dequant_bits_are_fp16"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
