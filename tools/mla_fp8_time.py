"""MLA decode over an FP8 latent pool, and the latent pool's fused append, against what a caller runs without them
(DESIGN.md §3.21), one process, by §3.10's method and over tools/mla_time.py's shapes, pages and lengths.

Forward runs, alternated `--repeats` times each after a warm-up of all, on the same seeded values:
  fp8          fa_forward_mla_paged_fp8 on the e4m3fn pool (kv_scale 0.3);
  fp16         fa_forward_mla_paged on the fp16 pool of the values decode(byte): the twin, twice the cache bytes;
  dequant      torch: the whole FP8 pool converted to fp16, then fa_forward_mla_paged: today's route for an FP8 pool.
Append runs (one new token for every sequence, lengths "random"), alternated in the same way:
  append16 / append8   fa_append_mla_paged / fa_append_mla_paged_fp8;
  recipe16 / recipe8   the docstring's indexing recipe for the batch with the positions computed on the device
                       (recipe8: after quantize_kv_fp8's divide, clamp and cast).
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`; the pools rotate over
several copies so that a call does not find its keys in the last-level cache.  Reported: median / min / max / spread
of each run and the ratios of the medians.

    python tools/mla_fp8_time.py [--out profiles/mla_fp8_time.json] [--repeats 7] [--window-ms 30]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mla_time import CAP, LLC_BYTES, PAGES, SCALE, SHAPES, C, V, write_results  # noqa: E402
from tf_flash_attention_amd import _lib  # noqa: E402

KV_SCALE = 0.3


def time_case(s, page, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hq, nq = s["seqs"], s["hq"], s["nq"]
    max_pages = CAP // page
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, seqs * hq, (nq,), (CAP,), C, V)
    plan = (ctypes.c_int32 * 5)()
    assert L.fa_forward_mla_paged_plan(prob, hq, page, plan) == 0 and plan[0] >= 1, "shape is outside the envelope"
    ws_bytes = int(L.fa_forward_mla_paged_workspace_bytes(prob, hq, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    num_pages = seqs * max_pages + max(seqs * max_pages // 8, 1)
    copies = max(1, min(4, -(-2 * LLC_BYTES // (num_pages * C * page))))
    table = torch.from_numpy(np.random.default_rng(99).permutation(num_pages)[:seqs * max_pages]
                             .reshape(seqs, max_pages).astype(np.int32)).to(dev)
    Q = (torch.rand((seqs, hq, C, nq), generator=gen, device=dev) * 4 - 2).half()
    true = torch.rand((num_pages, C, page), generator=gen, device=dev) * 4 - 2
    pools8 = [(true / KV_SCALE).clamp(-448, 448).to(torch.float8_e4m3fn)]
    pools8 += [pools8[0].clone() for _ in range(copies - 1)]
    pools16 = [p.to(torch.float16) for p in pools8]  # decode(byte), exact: the twin's pool
    del true
    scale = torch.tensor([KV_SCALE], dtype=torch.float32, device=dev)
    new = (torch.rand((seqs, C, 1), generator=gen, device=dev) * 4 - 2).half()
    O = torch.empty((seqs, hq, V, nq), dtype=torch.float16, device=dev)
    l = torch.empty((seqs, hq, nq), dtype=torch.float32, device=dev)
    m = torch.empty((seqs, hq, nq), dtype=torch.float16, device=dev)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    rows = torch.arange(seqs, device=dev)
    lens_np = {"full": np.full(seqs, CAP, np.int32),
               "random": np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)}

    out = []
    for name, ln in lens_np.items():
        kl = torch.from_numpy(ln).to(dev)

        def forward(pool, fp8):
            head = (stream, prob, hq, Q.data_ptr(), pool.data_ptr(), table.data_ptr(), max_pages, page, num_pages,
                    kl.data_ptr(), 1, SCALE)
            tail = (O.data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
            st = L.fa_forward_mla_paged_fp8(*head, scale.data_ptr(), *tail) if fp8 else L.fa_forward_mla_paged(*head, *tail)
            if st != 0:
                raise RuntimeError(_lib.last_error())

        def append(pool, fp8):
            args = (stream, seqs, C, 1, CAP, new.data_ptr(), pool.data_ptr()) + ((scale.data_ptr(),) if fp8 else ())
            if getattr(L, "fa_append_mla_paged" + ("_fp8" if fp8 else ""))(
                    *args, table.data_ptr(), max_pages, page, num_pages, kl.data_ptr(), None) != 0:
                raise RuntimeError(_lib.last_error())

        def recipe(pool, fp8):
            pos = (kl - 1).long()
            x = new[:, :, 0]
            if fp8:
                x = (x.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
            pool[table[rows, pos // page].long(), :, pos % page] = x

        calls = {"fp8": lambda i: forward(pools8[i % copies], True),
                 "fp16": lambda i: forward(pools16[i % copies], False),
                 "dequant": lambda i: forward(pools8[i % copies].to(torch.float16), False)}
        if name == "random":
            calls.update({"append16": lambda i: append(pools16[i % copies], False),
                          "append8": lambda i: append(pools8[i % copies], True),
                          "recipe16": lambda i: recipe(pools16[i % copies], False),
                          "recipe8": lambda i: recipe(pools8[i % copies], True)})
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(run, iters):
            torch.cuda.synchronize()
            e0.record()
            for i in range(iters):
                calls[run](i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        iters = {}
        for run in calls:  # warm-up of every run, and the calls per window from a first estimate
            window(run, 2)
            iters[run] = max(3, min(400, int(window_ms / max(window(run, 2), 1e-3)) + 1))
        times = {run: [] for run in calls}
        for _ in range(repeats):
            for run in calls:
                times[run].append(window(run, iters[run]))
        med = {r: statistics.median(v) for r, v in times.items()}
        case = dict(sequences=seqs, heads=hq, nq=nq, capacity=CAP, c=C, v=V, control=bool(s.get("control", False)),
                    page=page, lengths=name, kv_scale=KV_SCALE, pool_copies=copies, calls_per_window=iters,
                    fp8_over_fp16=med["fp8"] / med["fp16"], dequant_over_fp8=med["dequant"] / med["fp8"])
        if name == "random":
            case.update(recipe16_over_append16=med["recipe16"] / med["append16"],
                        recipe8_over_append8=med["recipe8"] / med["append8"])
        for r in calls:
            case[r + "_ms"] = dict(median=med[r], min=min(times[r]), max=max(times[r]),
                                   spread=(max(times[r]) - min(times[r])) / med[r])
        out.append(case)
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
        sys.exit("mla_fp8_time.py: no GPU; timings are only taken on the device")
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
