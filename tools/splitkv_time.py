"""Split-key forward against the query-outer forward on few-query shapes, one process.

For each shape the same seeded device inputs go alternately through fa_forward (one workgroup per
slice for these shapes: the path every caller took before the split-key kernels) and fa_forward_ws (the
split path), `--repeats` times each after a warm-up of both.  Every repeat is a HIP-event window over
enough back-to-back calls to last about `--window-ms`.  Reported per shape: the median / min / max time
of both paths, their ratio, the algorithmic K + V + Q + O bytes over the median time as a share of the HBM
bound (8 TB/s, the spec peak; a float4 copy reaches 6.3), the workspace bytes as a share of those, and
the largest |O_split - O_plain| with the fp16 forward tolerance of tests/gate.py it must stay within.

K and V rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left
by the call before.  The last shape (b = 1024) is the control: the GPU is full without splitting.

    python tools/splitkv_time.py [--out profiles/splitk_time.json] [--repeats 7] [--window-ms 30]

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
from tests.gate import TOL  # noqa: E402
from tf_flash_attention_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s (MI355X spec)
LLC_BYTES = 256 << 20

POL = {"full": _lib.FULL, "causal": _lib.CAUSAL}
SYNC = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}

SHAPES = (
    [dict(policy="full", b=16, qs=(nq,), ks=(16384,), d=d, sync="none_front") for nq in (1, 32, 128) for d in (64, 128)]
    + [dict(policy="causal", b=16, qs=(64,), ks=(16384,), d=d, sync="scale_end") for d in (64, 128)]
    + [dict(policy="full", b=16, qs=(8, 8), ks=(128, 128), d=d, sync="scale_front") for d in (64, 128)]
    + [dict(policy="full", b=1024, qs=(128,), ks=(16384,), d=d, sync="none_front", control=True) for d in (64, 128)]
)


def time_shape(s, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b, d = s["b"], s["d"]
    nq, nk = math.prod(s["qs"]), math.prod(s["ks"])
    prob = _lib.make_problem(_lib.F16, POL[s["policy"]], len(s["qs"]), SYNC[s["sync"]], b, s["qs"], s["ks"], d, d)
    plan = (ctypes.c_int32 * 4)()
    assert L.fa_forward_split_plan(prob, plan) == 0 and plan[0] >= 2, "shape does not split"
    ws_bytes = int(L.fa_forward_workspace_bytes(prob))

    g = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=g, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * b * d * nk * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    Q = rnd(b, d, nq)
    KV = [(rnd(b, d, nk), rnd(b, d, nk))]
    KV += [(KV[0][0].clone(), KV[0][1].clone()) for _ in range(copies - 1)]
    O = [torch.empty((b, d, nq), dtype=torch.float16, device=dev) for _ in range(2)]
    l = torch.empty((b, nq), dtype=torch.float32, device=dev)
    m = torch.empty((b, nq), dtype=torch.float16, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(split, i):
        K, V = KV[i % copies]
        if split:
            st = L.fa_forward_ws(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O[1].data_ptr(), l.data_ptr(),
                                 m.data_ptr(), ws.data_ptr(), ws_bytes)
        else:
            st = L.fa_forward(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O[0].data_ptr(), l.data_ptr(),
                              m.data_ptr())
        if st != 0:
            raise RuntimeError(_lib.last_error())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(split, iters):
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            call(split, i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    iters = {}
    for split in (False, True):  # warm-up of both paths, and the calls per window from a first estimate
        window(split, 3)
        iters[split] = max(5, min(400, int(window_ms / max(window(split, 3), 1e-3)) + 1))
    times = {False: [], True: []}
    for _ in range(repeats):
        for split in (False, True):
            times[split].append(window(split, iters[split]))

    call(False, 0)
    call(True, 0)
    torch.cuda.synchronize()
    ref, got = O[0].double().cpu().numpy(), O[1].double().cpu().numpy()
    rtol, atol = TOL[np.float16]["fwd"]
    scale = max(float(np.abs(ref).max()), 1.0)
    err = np.abs(got - ref)
    within = bool((err <= atol * scale + rtol * np.abs(ref)).all())

    algo_bytes = kv_bytes + 2 * b * d * nq * 2
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(
        policy=s["policy"], b=b, q_seq=list(s["qs"]), k_seq=list(s["ks"]), d=d, sync=s["sync"],
        control=bool(s.get("control", False)), chunks=int(plan[0]), chunk_keys=int(plan[1]), kv_copies=copies,
        calls_per_window={"plain": iters[False], "split": iters[True]},
        plain_ms=dict(median=med[False], min=min(times[False]), max=max(times[False])),
        split_ms=dict(median=med[True], min=min(times[True]), max=max(times[True])),
        speedup=med[False] / med[True],
        split_over_plain=med[True] / med[False],
        plain_spread=(max(times[False]) - min(times[False])) / med[False],
        algo_bytes=algo_bytes,
        plain_hbm_share=algo_bytes / (med[False] * 1e-3) / HBM_PEAK,
        split_hbm_share=algo_bytes / (med[True] * 1e-3) / HBM_PEAK,
        workspace_bytes=ws_bytes,
        # the partials are written once and read once
        workspace_traffic_share=2 * ws_bytes / algo_bytes,
        max_abs_diff_O=float(err.max()), fp16_fwd_bound_min=atol * scale, within_fp16_fwd_tol=within,
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
        sys.exit("splitkv_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        r = time_shape(s, a.repeats, a.window_ms)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, shapes=res), f, indent=1)
            f.write("\n")
    return 0 if all(r["within_fp16_fwd_tol"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
