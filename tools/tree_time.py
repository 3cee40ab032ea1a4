"""Tree-masked paged draft attention against what exists without it, one process.

For each shape of §3.10 (16 sequences of Hk = 2 K/V heads, capacity 16384, and the b_kv = 1024 control), each page
size and each set of lengths, the same seeded device inputs go alternately through four runs, `--repeats` times each
after a warm-up of all:
  tree         (a) fa_forward_paged_tree on the pools through a randomly permuted block table, the draft masks those
               of random forests (every token sees itself and its ancestors);
  tree_chain   (a') the same entry point with the lower-triangular mask: bitwise the next run's result;
  paged_tail   (i) fa_forward_paged with tail_causal = 1 at the same lengths: (a') / (i) is the price of the mask;
  composed     (ii) what a caller runs today: fa_forward_paged over the context (the lengths minus nq, formed on the
               device), a torch gather of the nq draft keys and values out of the pools (positions and pages from the
               device lengths and table), masked attention over them in torch with (O, l, m) formed as the library
               stores them, and fa_merge_partials of the two.  The tool checks its O against (a)'s under the fp16
               forward gate (1e-3 * max(|O|, 1) + 1e-3 * |O|) and fails if it does not hold.
Lengths: every length at the capacity ("full"), and seeded uniform lengths in [nq, capacity] ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, (a') / (i), (a) / (i) and (ii) / (a), and whether
(a) beats (ii) by more than twice the larger of the two spreads.

The pools rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.  The tool loads the product library and reads no environment variable.

    python tools/tree_time.py [--out profiles/tree_time.json] [--repeats 7] [--window-ms 20]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import _lib  # noqa: E402
from tf_flash_attention_amd import flash_attention as fa  # noqa: E402

LLC_BYTES = 256 << 20
CAP = 16384
PAGES = (64, 256)

# nq in {8, 32, 64} at g in {1, 4, 8} where g * next_pow2(nq) <= 128
SHAPES = (
    [dict(seqs=16, hk=2, g=g, nq=nq, d=d) for d in (64, 128) for nq in (8, 32, 64) for g in (1, 4, 8) if g * nq <= 128]
    + [dict(seqs=512, hk=2, g=4, nq=8, d=d, control=True) for d in (64, 128)]
)
RUNS = ("tree", "tree_chain", "paged_tail", "composed")


def time_case(s, page, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, g, nq, d, control = s["seqs"], s["hk"], s["g"], s["nq"], s["d"], bool(s.get("control", False))
    bkv, b, max_pages, words = seqs * hk, seqs * hk * g, CAP // page, (nq + 31) // 32
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (CAP,), d, d)
    plan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_paged_tree_plan(prob, g, page, plan) == 0 and plan[0] >= 1, "shape is outside the fused envelope"
    ws_bytes = int(L.fa_forward_paged_tree_workspace_bytes(prob, g, page))
    assert ws_bytes == int(L.fa_forward_paged_workspace_bytes(prob, g, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * CAP * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    rng = np.random.default_rng(99)
    table = torch.from_numpy(rng.permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)).to(dev)
    table64 = table.long()
    Q = rnd(b, d, nq)
    Q5 = Q.view(seqs, hk, g, d, nq)
    P0 = (rnd(num_pages, hk, d, page), rnd(num_pages, hk, d, page))
    pools = [P0] + [(P0[0].clone(), P0[1].clone()) for _ in range(copies - 1)]
    lens_np = np.random.default_rng(4321).integers(nq, CAP + 1, seqs).astype(np.int32)
    lens = {"full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev), "random": torch.from_numpy(lens_np).to(dev)}
    parents = torch.from_numpy(np.stack([[rng.integers(-1, i) for i in range(nq)] for _ in range(seqs)]).astype(np.int32)).to(dev)
    masks = {"tree": fa.draft_mask_from_parents(parents),
             "tree_chain": fa.draft_mask_from_parents(torch.arange(-1, nq - 1, dtype=torch.int32, device=dev).expand(seqs, nq))}
    j = torch.arange(nq, device=dev)
    sees = ((masks["tree"].long()[:, :, j >> 5] >> (j & 31)) & 1).bool()  # [seqs, query, slot]: the caller's own mask
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in RUNS + ("context", "draft")}
    l = {r: torch.empty((b, nq), dtype=torch.float32, device=dev) for r in RUNS + ("context", "draft")}
    m = {r: torch.empty((b, nq), dtype=torch.float16, device=dev) for r in RUNS + ("context", "draft")}
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    scale = 1.0 / math.sqrt(d)
    parts = {k: _lib.pointer_array([t["context"].data_ptr(), t["draft"].data_ptr()]) for k, t in (("O", O), ("l", l), ("m", m))}

    def paged(run, Kp, Vp, kl, tail):
        return L.fa_forward_paged(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(), max_pages,
                                  page, num_pages, kl.data_ptr(), hk, tail, O[run].data_ptr(), l[run].data_ptr(),
                                  m[run].data_ptr(), ws.data_ptr(), ws_bytes)

    def composed(Kp, Vp, kl):
        base = kl.long() - nq                                             # (the lengths here are >= nq)
        st = paged("context", Kp, Vp, base.int(), 0)
        pos = base[:, None] + j[None, :]                                  # [seqs, nq]: the draft keys' positions
        pg, off = table64.gather(1, pos // page), pos % page
        Kd, Vd = Kp[pg, :, :, off], Vp[pg, :, :, off]                     # [seqs, nq, hk, d]
        sc = torch.einsum("shgcq,skhc->shgqk", Q5.float(), Kd.float()) * scale
        sc = sc.masked_fill(~sees[:, None, None], float("-inf"))
        mx = sc.amax(-1).half()                                           # the stored m: the row max in fp16
        p = torch.exp(sc - mx.float()[..., None])
        lsum = p.sum(-1)
        o = torch.einsum("shgqk,skhc->shgcq", p, Vd.float()) / lsum[:, :, :, None, :]
        O["draft"].copy_(o.reshape(b, d, nq))
        l["draft"].copy_(lsum.reshape(b, nq))
        m["draft"].copy_(mx.reshape(b, nq))
        st |= L.fa_merge_partials(stream, _lib.F16, b, nq, d, 2, parts["O"], parts["l"], parts["m"], O["composed"].data_ptr(),
                                  l["composed"].data_ptr(), m["composed"].data_ptr())
        return st

    def call(run, it, kl):
        Kp, Vp = pools[it % copies]
        if run in masks:
            st = L.fa_forward_paged_tree(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                         max_pages, page, num_pages, kl.data_ptr(), hk, masks[run].data_ptr(),
                                         O[run].data_ptr(), l[run].data_ptr(), m[run].data_ptr(), ws.data_ptr(), ws_bytes)
        elif run == "paged_tail":
            st = paged(run, Kp, Vp, kl, 1)
        else:
            st = composed(Kp, Vp, kl)
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

    out = []
    for name, kl in lens.items():
        iters = {}
        for run in RUNS:  # warm-up of every run, and the calls per window from a first estimate
            window(run, 3, kl)
            iters[run] = max(5, min(400, int(window_ms / max(window(run, 3, kl), 1e-3)) + 1))
        times = {run: [] for run in RUNS}
        for _ in range(repeats):
            for run in RUNS:
                times[run].append(window(run, iters[run], kl))
        for run in RUNS:
            call(run, 0, kl)
        torch.cuda.synchronize()
        med = {r: statistics.median(v) for r, v in times.items()}
        spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
        stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r])  # noqa: E731
        ref = O["tree"].float()
        allow = 1e-3 * max(float(ref.abs().max()), 1.0) + 1e-3 * ref.abs()
        worst = float(((O["composed"].float() - ref).abs() / allow).max())
        chain_same = all(torch.equal(t["tree_chain"].view(torch.uint8), t["paged_tail"].view(torch.uint8)) for t in (O, l, m))
        live = int(np.full(seqs, CAP, np.int64).sum() if name == "full" else lens_np.astype(np.int64).sum())
        margin = 2 * max(spread["tree"], spread["composed"])
        out.append(dict(
            sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, mask_words=words, capacity=CAP, d=d, control=control,
            page=page, lengths=name, chunks=int(plan[0]), chunk_keys=int(plan[1]), workspace_bytes=ws_bytes,
            kv_copies=copies, calls_per_window=iters, **{r + "_ms": stats(r) for r in RUNS},
            chain_over_paged_tail=med["tree_chain"] / med["paged_tail"], tree_over_paged_tail=med["tree"] / med["paged_tail"],
            composed_over_tree=med["composed"] / med["tree"],
            tree_beats_composed_by_more_than_twice_the_larger_spread=bool(med["tree"] < med["composed"] * (1.0 - margin)),
            chain_is_bitwise_paged_tail=bool(chain_same), composed_worst_error_over_allowance=worst,
            composed_finite=bool(torch.isfinite(O["composed"].float()).all()),
            tree_bytes_per_s=2 * hk * d * 2 * live / (med["tree"] * 1e-3),
        ))
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
        sys.exit("tree_time.py: no GPU; timings are only taken on the device")
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
    ok = all(r["composed_worst_error_over_allowance"] <= 1.0 and r["composed_finite"] and r["chain_is_bitwise_paged_tail"]
             for r in res)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
