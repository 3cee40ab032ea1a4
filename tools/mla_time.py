"""MLA decode over a paged latent cache against the torch composition a caller could run before it (DESIGN.md
§3.20), one process, by §3.10's method.

For each shape (16 sequences, capacity 16384, Hq in {16, 128}, Nq in {1, 2}, C / v = 576 / 512, and a 512-sequence
control), each page size and each set of lengths, the same seeded device inputs go alternately through two runs,
`--repeats` times each after a warm-up of both:
  mla          fa_forward_mla_paged on the pool through a randomly permuted block table;
  composition  torch: index_select of the sequences' pages up to the longest length (known on the HOST here, which
               the kernel never needs), the layout copy into [seq, C, keys], fp16 matmul, a masked softmax in fp32
               and the fp16 matmul with the first v channels.  The index and the mask are built outside the window.
Lengths: every length at the capacity ("full"), and seeded uniform lengths ("random").
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, composition / mla, the largest |O| difference of
the two, and two floors computed from the shape: the live latent bytes over the measured 6.29 TB/s copy rate and
the launched tiles' MFMA work (68 32x32x16 MFMAs a wave, 4 waves, per 64-row block and live 64-key tile) over the
2516.6 TF/s fp16 MFMA peak.

The pool rotates over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.

    python tools/mla_time.py [--out profiles/mla_time.json] [--repeats 7] [--window-ms 30]

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

LLC_BYTES = 256 << 20
CAP = 16384
PAGES = (64, 256)
C, V = 576, 512
COPY_RATE = 6.29e12   # bytes / s: the project's measured device copy rate
MFMA_PEAK = 2516.6e12  # fp16 FLOP / s
SCALE = 1.0 / math.sqrt(192)

SHAPES = ([dict(seqs=16, hq=hq, nq=nq) for hq in (16, 128) for nq in (1, 2)]
          + [dict(seqs=512, hq=16, nq=1, control=True)])


def time_case(s, page, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hq, nq, control = s["seqs"], s["hq"], s["nq"], bool(s.get("control", False))
    b, max_pages = seqs * hq, CAP // page
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (CAP,), C, V)
    plan = (ctypes.c_int32 * 5)()
    assert L.fa_forward_mla_paged_plan(prob, hq, page, plan) == 0 and plan[0] >= 1, "shape is outside the envelope"
    ws_bytes = int(L.fa_forward_mla_paged_workspace_bytes(prob, hq, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)  # an eighth of the pool is free
    pool_bytes = num_pages * C * page * 2
    copies = max(1, min(4, -(-2 * LLC_BYTES // pool_bytes)))
    table_np = np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages].reshape(seqs, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    Q = rnd(seqs, hq, C, nq)
    pools = [rnd(num_pages, C, page)]
    pools += [pools[0].clone() for _ in range(copies - 1)]
    lens_np = {"full": np.full(seqs, CAP, np.int32),
               "random": np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)}
    O = {r: torch.empty((seqs, hq, V, nq), dtype=torch.float16, device=dev) for r in ("mla", "composition")}
    l = torch.empty((seqs, hq, nq), dtype=torch.float32, device=dev)
    m = torch.empty((seqs, hq, nq), dtype=torch.float16, device=dev)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    Qr = (Q.float() * SCALE).half().permute(0, 1, 3, 2).reshape(seqs, hq * nq, C)  # the composition's pre-scaled Q

    out = []
    for name, ln in lens_np.items():
        kl = torch.from_numpy(ln).to(dev)
        used = -(-int(ln.max()) // page)  # pages the composition gathers per sequence
        index = table[:, :used].reshape(-1).long()
        keys = torch.arange(used * page, device=dev)
        pos = kl.view(seqs, 1, 1, 1) - nq + torch.arange(nq, device=dev).view(1, 1, nq, 1)  # the tail rule (nq = 1: all)
        neg = torch.where(keys.view(1, 1, 1, -1) <= pos, 0.0, float("-inf")).expand(seqs, hq, nq, -1).reshape(seqs, hq * nq, -1)

        def call(run, it):
            pool = pools[it % copies]
            if run == "mla":
                st = L.fa_forward_mla_paged(stream, prob, hq, Q.data_ptr(), pool.data_ptr(), table.data_ptr(), max_pages,
                                            page, num_pages, kl.data_ptr(), 1, SCALE, O[run].data_ptr(), l.data_ptr(),
                                            m.data_ptr(), ws.data_ptr(), ws_bytes)
                if st != 0:
                    raise RuntimeError(_lib.last_error())
            else:
                K = pool.index_select(0, index).view(seqs, used, C, page).permute(0, 2, 1, 3).reshape(seqs, C, used * page)
                P = torch.softmax(torch.bmm(Qr, K).float() + neg, dim=-1).half()
                O[run].copy_(torch.bmm(P, K[:, :V, :].transpose(1, 2)).view(seqs, hq, nq, V).permute(0, 1, 3, 2))

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(run, iters):
            torch.cuda.synchronize()
            e0.record()
            for i in range(iters):
                call(run, i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        runs = ("mla", "composition")
        iters = {}
        for run in runs:  # warm-up of both runs, and the calls per window from a first estimate
            window(run, 2)
            iters[run] = max(3, min(400, int(window_ms / max(window(run, 2), 1e-3)) + 1))
        times = {run: [] for run in runs}
        for _ in range(repeats):
            for run in runs:
                times[run].append(window(run, iters[run]))
        for run in runs:
            call(run, 0)
        torch.cuda.synchronize()
        med = {r: statistics.median(v) for r, v in times.items()}
        stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]),  # noqa: E731
                               spread=(max(times[r]) - min(times[r])) / med[r])
        live = int(ln.astype(np.int64).sum())
        tiles = int(sum(-(-int(x) // 64) for x in ln))
        bytes_floor_ms = live * C * 2 / COPY_RATE * 1e3
        mfma_floor_ms = tiles * int(plan[4]) * 4 * 68 * (2 * 32 * 32 * 16) / MFMA_PEAK * 1e3
        out.append(dict(
            sequences=seqs, heads=hq, nq=nq, capacity=CAP, c=C, v=V, control=control, page=page, lengths=name,
            chunks=int(plan[0]), chunk_keys=int(plan[1]), rows=int(plan[3]), row_blocks=int(plan[4]), pool_copies=copies,
            calls_per_window=iters, mla_ms=stats("mla"), composition_ms=stats("composition"),
            composition_over_mla=med["composition"] / med["mla"], mla_beats_composition=bool(med["mla"] < med["composition"]),
            max_abs_o_difference=float((O["mla"].float() - O["composition"].float()).abs().max()),
            live_latent_bytes=live * C * 2, bytes_floor_ms=bytes_floor_ms, mfma_floor_ms=mfma_floor_ms,
            mla_over_bytes_floor=med["mla"] / bytes_floor_ms, mla_over_mfma_floor=med["mla"] / mfma_floor_ms,
            mla_live_bytes_per_s=live * C * 2 / (med["mla"] * 1e-3),
        ))
    return out


def write_results(f, device, cases):
    """One case a line: the file stays readable in a diff."""
    f.write('{"device": ' + json.dumps(device) + ', "cases": [\n')
    f.write(",\n".join(json.dumps(c) for c in cases))
    f.write("\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("mla_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        for page in PAGES:
            for r in time_case(s, page, a.repeats, a.window_ms):
                res.append(r)
                print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            write_results(f, torch.cuda.get_device_name(0), res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
