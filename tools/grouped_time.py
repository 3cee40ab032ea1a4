"""Grouped-query forward against the ungrouped forward on expanded K / V, one process.

For each shape the same seeded device inputs go alternately through three runs, `--repeats` times each after
a warm-up of all:
  fused     fa_forward_grouped on K / V [b_kv] (the g heads of a group folded into one workgroup's rows);
  expanded  fa_forward_ws on K / V already repeated g times [b_kv * g] (the copy not timed);
  copy+exp  the repeat_interleave of K and V, then the same fa_forward_ws (what a caller without the grouped
            interface pays).
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per
shape: median / min / max and spread ((max - min) / median) of each run, the ratios, the K + V bytes the fused
run reads over its median time (and as a share of the 6.29 TB/s a device copy reaches,
profiles/combine_time.json), whether the fused run beats the expanded one by more than twice the larger of the
two spreads (the rule that keeps a (D, folded rows) class in the plan), and the largest |O_fused - O_expanded|
with the fp16 forward tolerance of tests/gate.py.

K and V rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.  The last shapes (b_kv = 1024) are the control: the GPU is full either way.

    python tools/grouped_time.py [--out profiles/grouped_time.json] [--repeats 7] [--window-ms 30]

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
from tests.gate import TOL  # noqa: E402
from tf_flash_attention_amd import _lib  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s of a device copy (profiles/combine_time.json)
LLC_BYTES = 256 << 20

SHAPES = (
    [dict(bkv=16, g=g, nq=nq, nk=16384, d=d) for d in (64, 128) for g in (4, 8) for nq in (1, 4, 16)]
    + [dict(bkv=1024, g=4, nq=8, nk=16384, d=d, control=True) for d in (64, 128)]
)
RUNS = ("fused", "expanded", "copy_expanded")


def time_shape(s, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    bkv, g, nq, nk, d = s["bkv"], s["g"], s["nq"], s["nk"], s["d"]
    b = bkv * g
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (nk,), d, d)
    plan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_grouped_plan(prob, g, plan) == 0 and plan[0] >= 1, "shape is outside the fused envelope"
    ws_g = int(L.fa_forward_grouped_workspace_bytes(prob, g))
    ws_e = int(L.fa_forward_workspace_bytes(prob))

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * nk * 2
    # the expanded tensors are g times as large: rotate both sets over enough copies to outrun the cache
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    copies_e = max(1, min(copies, -(-2 * LLC_BYTES // (kv_bytes * g))))
    Q = rnd(b, d, nq)
    KV = [(rnd(bkv, d, nk), rnd(bkv, d, nk))]
    KV += [(KV[0][0].clone(), KV[0][1].clone()) for _ in range(copies - 1)]
    KVe = [tuple(t.repeat_interleave(g, dim=0) for t in KV[0]) for _ in range(copies_e)]
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in RUNS}
    l = torch.empty((b, nq), dtype=torch.float32, device=dev)
    m = torch.empty((b, nq), dtype=torch.float16, device=dev)
    ws = torch.empty(max(ws_g, ws_e, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def expanded(K, V, out):
        return L.fa_forward_ws(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), out.data_ptr(), l.data_ptr(),
                               m.data_ptr(), ws.data_ptr(), ws_e)

    def call(run, i):
        if run == "fused":
            K, V = KV[i % copies]
            st = L.fa_forward_grouped(stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O[run].data_ptr(),
                                      l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_g)
        elif run == "expanded":
            st = expanded(*KVe[i % copies_e], O[run])
        else:
            K, V = KV[i % copies]
            st = expanded(K.repeat_interleave(g, dim=0), V.repeat_interleave(g, dim=0), O[run])
        if st != 0:
            raise RuntimeError(_lib.last_error())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(run, iters):
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            call(run, i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    iters = {}
    for run in RUNS:  # warm-up of every run, and the calls per window from a first estimate
        window(run, 3)
        iters[run] = max(5, min(400, int(window_ms / max(window(run, 3), 1e-3)) + 1))
    times = {run: [] for run in RUNS}
    for _ in range(repeats):
        for run in RUNS:
            times[run].append(window(run, iters[run]))

    for run in RUNS:
        call(run, 0)
    torch.cuda.synchronize()
    ref, got = O["expanded"].double().cpu().numpy(), O["fused"].double().cpu().numpy()
    rtol, atol = TOL[np.float16]["fwd"]
    scale = max(float(np.abs(ref).max()), 1.0)
    err = np.abs(got - ref)
    within = bool((err <= 2 * (atol * scale + rtol * np.abs(ref))).all())  # (both sides carry the tolerance)

    med = {r: statistics.median(v) for r, v in times.items()}
    spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
    stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r])  # noqa: E731
    gain = 1.0 - med["fused"] / med["expanded"]
    return dict(
        b_kv=bkv, kv_group=g, nq=nq, nk=nk, d=d, control=bool(s.get("control", False)),
        chunks=int(plan[0]), chunk_keys=int(plan[1]), pitch=int(plan[4]), folded_rows=int(plan[5]),
        kv_copies=copies, kv_copies_expanded=copies_e, calls_per_window=iters,
        fused_ms=stats("fused"), expanded_ms=stats("expanded"), copy_expanded_ms=stats("copy_expanded"),
        speedup_over_expanded=med["expanded"] / med["fused"],
        speedup_over_copy_expanded=med["copy_expanded"] / med["fused"],
        # the rule of the plan: faster than the expanded run by more than twice the larger spread
        gain_over_expanded=gain, beats_expanded=bool(gain > 2 * max(spread["fused"], spread["expanded"])),
        kv_bytes=kv_bytes, fused_kv_bytes_per_s=kv_bytes / (med["fused"] * 1e-3),
        fused_share_of_copy_rate=kv_bytes / (med["fused"] * 1e-3) / COPY_RATE,
        expanded_kv_bytes_per_s=kv_bytes * g / (med["expanded"] * 1e-3),
        workspace_bytes=ws_g, workspace_traffic_share=2 * ws_g / kv_bytes,
        max_abs_diff_O=float(err.max()), fp16_fwd_bound_min=atol * scale, within_twice_fp16_fwd_tol=within,
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("grouped_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        r = time_shape(s, a.repeats, a.window_ms)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), copy_rate_bytes_per_s=COPY_RATE, shapes=res), f, indent=1)
            f.write("\n")
    return 0 if all(r["within_twice_fp16_fwd_tol"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
