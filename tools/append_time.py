"""The fused K/V append against what a caller ran before it, one process, §3.9's method.

For each row (16 sequences of Hk = 2 K/V heads, capacity 16384, d = v_d in {64, 128}, page in {64, 256}, an fp16 or an
FP8 pool, n_new in {1, 128, 2048}, seeded uniform lengths; and the control of 512 sequences at n_new = 1) the same
seeded device inputs go alternately through two runs, `--repeats` times each after a warm-up of both:
  fused    (a) one fa_append_paged / fa_append_paged_fp8 call, K and V together;
  recipe   (b) the recipe of the paged_1d docstring for a whole batch, in torch: the positions, the table gather and
           the page offsets are built INSIDE the window, because they depend on k_lens; then one index_put for K and
           one for V.  For an FP8 pool quantize_kv_fp8 with the pool's scales comes first.
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  The pools and the new
tokens rotate over several copies (as many as 16 GiB of pools allow), so a call does not find its lines in the 256 MB
last-level cache left by the call before.  Reported per row: median / min / max and spread ((max - min) / median) of
each run in microseconds, recipe / fused, whether (a) beats (b) by more than twice the larger spread (the criterion),
whether both wrote the same bytes, for n_new = 2048 the bytes (a) reads plus writes per second against the 6.29 TB/s
copy rate, and for n_new = 1 (a) as a share of fa_forward_paged's time on the shape (g = 1, nq = 1,
random lengths, an fp16 pool).

    python tools/append_time.py [--out profiles/append_time.json] [--repeats 7] [--window-ms 30] [--only d,page,fp8,n_new]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import _lib  # noqa: E402

LLC_BYTES = 256 << 20
POOL_BUDGET = 16 << 30
COPY_RATE = 6.29e12  # bytes per second, the float4 copy of the README
CAP = 16384
RUNS = ("fused", "recipe")
# fa_forward_paged, g = 1, nq = 1, random lengths, 16 sequences x Hk = 2: (d, page) -> microseconds
FORWARD_US = {(64, 64): 48.0, (64, 256): 47.4, (128, 64): 99.5, (128, 256): 99.5}


def rows():
    """The issue's grid, then the control."""
    grid = [dict(seqs=16, hk=2, d=d, page=page, fp8=fp8, n_new=n)
            for d in (64, 128) for page in (64, 256) for fp8 in (False, True) for n in (1, 128, 2048)]
    return grid + [dict(seqs=512, hk=2, d=d, page=64, fp8=fp8, n_new=1, control=True) for d in (64, 128) for fp8 in (False, True)]


def moved_bytes(r):
    """Bytes one fused call reads (fp16 tokens) plus writes (the cache's elements), K and V together."""
    elems = r["seqs"] * r["hk"] * 2 * r["d"] * r["n_new"]
    return elems * 2 + elems * (1 if r["fp8"] else 2)


def summarise(times, r):
    """times: {run: [microseconds per call of every repeat]} -> the per-run statistics, the criterion and the rates."""
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    out = {k + "_us": dict(median=med[k], min=min(times[k]), max=max(times[k]), spread=spread[k]) for k in times}
    gain = med["recipe"] / med["fused"] - 1.0
    out.update(recipe_over_fused=med["recipe"] / med["fused"], twice_the_larger_spread=2 * max(spread.values()),
               fused_beats_recipe=bool(gain > 2 * max(spread.values())))
    if r["n_new"] == 2048:
        rate = moved_bytes(r) / (med["fused"] * 1e-6)
        out.update(fused_bytes=moved_bytes(r), fused_bytes_per_second=rate, fused_share_of_copy_rate=rate / COPY_RATE)
    if r["n_new"] == 1 and not r.get("control"):
        out.update(forward_paged_us=FORWARD_US[(r["d"], r["page"])],
                   fused_share_of_forward_paged=med["fused"] / FORWARD_US[(r["d"], r["page"])])
    return out


def time_row(r, repeats, window_ms):
    import torch
    from tf_flash_attention_amd import flash_attention as fa
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, d, page, fp8, n_new = r["seqs"], r["hk"], r["d"], r["page"], r["fp8"], r["n_new"]
    max_pages = CAP // page
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    esize = 1 if fp8 else 2
    pool_bytes = 2 * num_pages * hk * d * page * esize
    copies = max(1, min(8, POOL_BUDGET // pool_bytes))
    new_bytes = 2 * seqs * hk * d * n_new * 2
    new_copies = max(1, min(16, -(-2 * LLC_BYTES // new_bytes)))
    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    cache_dtype = torch.uint8 if fp8 else torch.float16
    pools = [(torch.zeros((num_pages, hk, d, page), dtype=cache_dtype, device=dev),
              torch.zeros((num_pages, hk, d, page), dtype=cache_dtype, device=dev)) for _ in range(copies)]
    news = [(rnd(seqs, hk, d, n_new), rnd(seqs, hk, d, n_new))]
    news += [(news[0][0].clone(), news[0][1].clone()) for _ in range(new_copies - 1)]
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    lens = torch.from_numpy(np.random.default_rng(4321).integers(n_new, CAP + 1, seqs).astype(np.int32)).to(dev)
    ks = torch.tensor([0.011, 0.017], dtype=torch.float32, device=dev) if fp8 else None
    vs = torch.tensor([0.009, 0.013], dtype=torch.float32, device=dev) if fp8 else None
    slots = torch.arange(n_new, dtype=torch.int32, device=dev)  # (does not depend on k_lens: built once)
    stream = torch.cuda.current_stream().cuda_stream
    entry = getattr(L, _lib.append_entry_point("paged", fp8))
    scale_ptrs = (ks.data_ptr(), vs.data_ptr()) if fp8 else ()

    def call(run, it, target=None):
        Kp, Vp = target or pools[it % copies]
        Kn, Vn = news[it % new_copies]
        if run == "fused":
            st = entry(stream, seqs, hk, d, d, n_new, CAP, Kn.data_ptr(), Vn.data_ptr(), Kp.data_ptr(), Vp.data_ptr(),
                       *scale_ptrs, table.data_ptr(), max_pages, page, num_pages, lens.data_ptr(), None)
            if st != 0:
                raise RuntimeError(_lib.last_error())
            return
        pos = (lens[:, None] - n_new + slots[None, :]).long()        # [S, n_new]
        pg = torch.gather(table, 1, pos // page).long()              # K_pool[block_table[s, pos // page], :, :, pos % page]
        off = pos % page
        if fp8:
            Kn = fa.quantize_kv_fp8(Kn, head_axis=1, scale=ks)[0].view(torch.uint8)
            Vn = fa.quantize_kv_fp8(Vn, head_axis=1, scale=vs)[0].view(torch.uint8)
        Kp[pg, :, :, off] = Kn.permute(0, 3, 1, 2)
        Vp[pg, :, :, off] = Vn.permute(0, 3, 1, 2)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(run, iters):
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            call(run, i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    iters = {}
    for run in RUNS:  # warm-up of both, and the calls per window from a first estimate
        window(run, 2)
        iters[run] = max(3, min(10000,int(window_ms * 1e3 / max(window(run, 3), 1.0)) + 1))
    times = {run: [] for run in RUNS}
    for _ in range(repeats):
        for run in RUNS:
            times[run].append(window(run, iters[run]))
    # the two write the same bytes
    a = (torch.zeros_like(pools[0][0]), torch.zeros_like(pools[0][1]))
    call("fused", 0, a)
    b = pools[0]
    b[0].zero_()
    b[1].zero_()
    call("recipe", 0, b)
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[0].any()))
    return dict(sequences=seqs, kv_heads=hk, d=d, page=page, fp8=fp8, n_new=n_new, capacity=CAP,
                control=bool(r.get("control", False)), pool_copies=int(copies), token_copies=int(new_copies),
                calls_per_window=iters, **summarise(times, r), same_bytes=same)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--only", help="d,page,fp8,n_new: one row of the grid (fp8 as 0 or 1)")
    a = ap.parse_args(argv)
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    grid = rows()
    if a.only:
        try:
            d, page, fp8, n_new = (int(x) for x in a.only.split(","))
        except ValueError:
            ap.error("--only takes d,page,fp8,n_new")
        grid = [r for r in grid if (r["d"], r["page"], int(r["fp8"]), r["n_new"]) == (d, page, fp8, n_new) and not r.get("control")]
        if not grid:
            ap.error("--only names no row of the grid")
    import torch
    if not torch.cuda.is_available():
        sys.exit("append_time.py: no GPU; timings are only taken on the device")
    res = []
    for r in grid:
        res.append(time_row(r, a.repeats, a.window_ms))
        print(json.dumps(res[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=res,
                           rows_that_miss_the_criterion=[(r["d"], r["page"], r["fp8"], r["n_new"], r["control"])
                                                         for r in res if not r["fused_beats_recipe"]]), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
