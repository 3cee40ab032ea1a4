"""The 256-channel paged forward against what a caller runs without it, one process, by §3.10's
method.

For each shape (16 sequences x Hk in {4, 8} K/V heads, capacity 16384, d = v_d = 256, g in {2, 4}, Nq in {1, 4}), each
page size (64, 256), each set of lengths (all at the capacity: "full"; seeded uniform: "random") and each window
(none, 1024, 4096; always under the tail rule) the same seeded device inputs go alternately through three runs,
`--repeats` times each after a warm-up of all:
  wide         fa_forward_paged_wide on the pools through a randomly permuted block table;
  composition  torch, what a caller runs today: index_select of the pages between the lowest window start and the
               longest length (known on the HOST here, which the kernel never needs), the layout copies, fp16 matmul,
               a masked softmax in fp32 and the fp16 matmul with V.  The index and the mask are built outside the
               timed window;
  yardstick    fa_forward_paged (fa_forward_paged_window under a window) at d = v_d = 128 with twice the K/V heads:
               other numbers, the same bytes.
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per case:
median / min / max and spread ((max - min) / median) of each run, composition / wide and whether wide is faster by
more than the composition's own spread, yardstick / wide, the largest |O| difference of wide and composition, and the
live K/V bytes per second of wide against the measured 6.29 TB/s copy rate.

    python tools/paged_wide_time.py [--out profiles/paged_wide_time.json] [--repeats 7] [--window-ms 30]

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

CAP, SEQS, D = 16384, 16, 256
PAGES = (64, 256)
WINDOWS = (None, 1024, 4096)
COPY_RATE = 6.29e12  # bytes / s: the project's measured device copy rate
SHAPES = [dict(hk=hk, g=g, nq=nq) for hk in (4, 8) for g in (2, 4) for nq in (1, 4)]
RUNS = ("wide", "composition", "yardstick")


def time_case(s, page, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    hk, g, nq = s["hk"], s["g"], s["nq"]
    max_pages = CAP // page
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, SEQS * hk * g, (nq,), (CAP,), D, D)
    prob_y = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, SEQS * 2 * hk * g, (nq,), (CAP,), D // 2, D // 2)
    plan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_paged_wide_plan(prob, g, page, plan) == 0 and plan[0] >= 1, "shape is outside the envelope"
    ws_bytes = int(L.fa_forward_paged_wide_workspace_bytes(prob, g, page))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    num_pages = SEQS * max_pages + SEQS * max_pages // 8  # an eighth of the pool is free
    table_np = np.random.default_rng(99).permutation(num_pages)[:SEQS * max_pages].reshape(SEQS, max_pages).astype(np.int32)
    table = torch.from_numpy(table_np).to(dev)
    Q = rnd(SEQS, hk * g, D, nq)
    Kp, Vp = rnd(num_pages, hk, D, page), rnd(num_pages, hk, D, page)  # (2 x 1.2 GB at Hk = 8: past the 256 MB cache)
    Qy, Ky, Vy = Q.view(SEQS, 2 * hk * g, D // 2, nq), Kp.view(num_pages, 2 * hk, D // 2, page), Vp.view(num_pages, 2 * hk, D // 2, page)
    lens_np = {"full": np.full(SEQS, CAP, np.int32),
               "random": np.random.default_rng(4321).integers(nq, CAP + 1, SEQS).astype(np.int32)}
    O = {r: torch.empty((SEQS, hk * g, D, nq), dtype=torch.float16, device=dev) for r in RUNS}
    l = torch.empty((SEQS, 2 * hk * g, nq), dtype=torch.float32, device=dev)
    m = torch.empty((SEQS, 2 * hk * g, nq), dtype=torch.float16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    Qr = (Q.float() / math.sqrt(D)).half().view(SEQS * hk, g, D, nq).permute(0, 1, 3, 2).reshape(SEQS * hk, g * nq, D)

    out = []
    for name, ln in lens_np.items():
        kl = torch.from_numpy(ln).to(dev)
        for W in WINDOWS:
            lo = np.maximum(ln - nq - (W or CAP) + 1, 0)
            p0, p1 = int(lo.min()) // page, -(-int(ln.max()) // page)  # the pages the composition gathers
            index = table[:, p0:p1].reshape(-1).long()
            keys = torch.arange(p0 * page, p1 * page, device=dev).view(1, 1, -1)
            pos = (kl.view(SEQS, 1, 1) - nq + torch.arange(nq, device=dev).view(1, nq, 1))
            seen = (keys <= pos) & (keys > pos - (W or CAP))
            neg = torch.where(seen, 0.0, float("-inf")).view(SEQS, 1, 1, nq, -1).expand(SEQS, hk, g, nq, -1).reshape(SEQS * hk, g * nq, -1)
            if W is None:
                y_ws, y_fwd, y_own, y_arg = L.fa_forward_paged_workspace_bytes, L.fa_forward_paged, (prob_y, g, page), 1
            else:
                y_ws, y_fwd, y_own, y_arg = (L.fa_forward_paged_window_workspace_bytes, L.fa_forward_paged_window,
                                             (prob_y, g, page, W), W)
            yws_bytes = int(y_ws(*y_own))
            ws = torch.empty(max(ws_bytes, yws_bytes, 1), dtype=torch.uint8, device=dev)

            def call(run):
                if run == "wide":
                    st = L.fa_forward_paged_wide(stream, prob, g, Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), table.data_ptr(),
                                                 max_pages, page, num_pages, kl.data_ptr(), hk, 1, W or 0, O[run].data_ptr(),
                                                 l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
                elif run == "yardstick":
                    st = y_fwd(stream, prob_y, g, Qy.data_ptr(), Ky.data_ptr(), Vy.data_ptr(), table.data_ptr(), max_pages,
                               page, num_pages, kl.data_ptr(), 2 * hk, y_arg, O[run].data_ptr(), l.data_ptr(), m.data_ptr(),
                               ws.data_ptr(), yws_bytes)
                else:
                    st = 0
                    gather = lambda pool: (pool.index_select(0, index).view(SEQS, p1 - p0, hk, D, page)  # noqa: E731
                                           .permute(0, 2, 3, 1, 4).reshape(SEQS * hk, D, (p1 - p0) * page))
                    P = torch.softmax(torch.bmm(Qr, gather(Kp)).float() + neg, dim=-1).half()
                    O[run].copy_(torch.bmm(P, gather(Vp).transpose(1, 2)).view(SEQS, hk * g, nq, D).permute(0, 1, 3, 2))
                if st != 0:
                    raise RuntimeError(_lib.last_error())

            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def window(run, iters):
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters):
                    call(run)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters

            iters = {}
            for run in RUNS:  # warm-up of every run, and the calls per window from a first estimate
                window(run, 2)
                iters[run] = max(3, min(400, int(window_ms / max(window(run, 2), 1e-3)) + 1))
            times = {run: [] for run in RUNS}
            for _ in range(repeats):
                for run in RUNS:
                    times[run].append(window(run, iters[run]))
            med = {r: statistics.median(v) for r, v in times.items()}
            stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]),  # noqa: E731
                                   spread=(max(times[r]) - min(times[r])) / med[r])
            live_bytes = int((ln - lo // 64 * 64).astype(np.int64).sum()) * hk * 2 * D * 2
            comp = stats("composition")
            out.append(dict(
                sequences=SEQS, kv_heads=hk, g=g, nq=nq, capacity=CAP, d=D, v_d=D, page=page, lengths=name, window=W,
                chunks=int(plan[0]), chunk_keys=int(plan[1]), rows=int(plan[3]), row_blocks=int(plan[4]),
                calls_per_window=iters, wide_ms=stats("wide"), composition_ms=comp, yardstick_ms=stats("yardstick"),
                composition_over_wide=med["composition"] / med["wide"],
                wide_faster_by_more_than_the_composition_spread=bool(med["wide"] < comp["min"] - (comp["max"] - comp["min"])),
                yardstick_over_wide=med["yardstick"] / med["wide"],
                max_abs_o_difference=float((O["wide"].float() - O["composition"].float()).abs().max()),
                live_kv_bytes=live_bytes, wide_live_bytes_per_s=live_bytes / (med["wide"] * 1e-3),
                wide_share_of_copy_rate=live_bytes / (med["wide"] * 1e-3) / COPY_RATE,
            ))
            print(json.dumps(out[-1]), flush=True)
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
        sys.exit("paged_wide_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        for page in PAGES:
            res += time_case(s, page, a.repeats, a.window_ms)
            torch.cuda.empty_cache()
            if a.out:  # (rewritten after every shape: a run that is cut short keeps what it measured)
                with open(a.out, "w") as f:
                    f.write('{"device": ' + json.dumps(torch.cuda.get_device_name(0)) + ', "cases": [\n')
                    f.write(",\n".join(json.dumps(c) for c in res))
                    f.write("\n]}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
