"""Split-key backward against the two-pass backward on few-query shapes, one process.

The backward counterpart of tools/splitkv_time.py, same protocol and shapes.  For each shape the same seeded
device inputs (and the forward's O, l, m) go alternately through fa_backward (its dQ pass runs one workgroup
per slice for these shapes: the path every caller took before the split dQ pass) and fa_backward_split,
`--repeats` times each after a warm-up of both.  Every repeat is a HIP-event window over enough back-to-back
calls to last about `--window-ms`.  Reported per shape: the median / min / max time of both paths, their
ratio, the spread (max - min over the median) of the fa_backward path, whether the split path is faster by
more than twice that spread, the workspace traffic share nq*d*4 / (chunk*(d + v_d)*2) (a chunk's partial
beside the K / V bytes it reads), and the largest |dQ_split - dQ_plain| with twice the plain fp16 backward
bound of tests/gate.py it must stay within (dK and dV must be bitwise equal).

K and V rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left
by the call before.  The last shapes (b = 1024) are the control: the GPU is full without splitting.

    python tools/splitk_bwd_time.py [--out profiles/splitk_bwd_time.json] [--repeats 7] [--window-ms 30]
                                    [--only b16|control] [--index N ...]

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splitkv_time import LLC_BYTES, POL, SHAPES, SYNC  # noqa: E402  (the forward tool's shapes)
from tests.gate import TOL, plain_bound  # noqa: E402
from tf_flash_attention_amd import _lib  # noqa: E402


def time_shape(s, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b, d = s["b"], s["d"]
    nq, nk = math.prod(s["qs"]), math.prod(s["ks"])
    prob = _lib.make_problem(_lib.F16, POL[s["policy"]], len(s["qs"]), SYNC[s["sync"]], b, s["qs"], s["ks"], d, d)
    plan = (ctypes.c_int32 * 4)()
    assert L.fa_backward_split_plan(prob, plan) == 0 and plan[0] >= 2, "shape does not split"
    ws_bytes = {False: int(L.fa_backward_workspace_bytes(prob)), True: int(L.fa_backward_split_workspace_bytes(prob))}
    fws_bytes = int(L.fa_forward_workspace_bytes(prob))

    g = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=g, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * b * d * nk * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    Q, dO = rnd(b, d, nq), rnd(b, d, nq)
    KV = [(rnd(b, d, nk), rnd(b, d, nk))]
    KV += [(KV[0][0].clone(), KV[0][1].clone()) for _ in range(copies - 1)]
    O = torch.empty((b, d, nq), dtype=torch.float16, device=dev)
    l = torch.empty((b, nq), dtype=torch.float32, device=dev)
    m = torch.empty((b, nq), dtype=torch.float16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    fws = torch.empty(max(fws_bytes, 1), dtype=torch.uint8, device=dev)
    st = L.fa_forward_ws(stream, prob, Q.data_ptr(), KV[0][0].data_ptr(), KV[0][1].data_ptr(), O.data_ptr(),
                         l.data_ptr(), m.data_ptr(), fws.data_ptr(), fws_bytes)
    if st != 0:
        raise RuntimeError(_lib.last_error())
    del fws
    dQ = [torch.empty_like(Q) for _ in range(2)]
    dK = [torch.empty_like(KV[0][0]) for _ in range(2)]
    dV = [torch.empty_like(KV[0][1]) for _ in range(2)]
    ws = torch.empty(ws_bytes[True], dtype=torch.uint8, device=dev)

    def call(split, i):
        K, V = KV[i % copies]
        fn = L.fa_backward_split if split else L.fa_backward
        st = fn(stream, prob, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), l.data_ptr(), m.data_ptr(),
                dO.data_ptr(), dQ[split].data_ptr(), dK[split].data_ptr(), dV[split].data_ptr(), ws.data_ptr(),
                ws_bytes[split])
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
    ref, got = dQ[0].double().cpu().numpy(), dQ[1].double().cpu().numpy()
    bound = 2.0 * plain_bound(ref, *TOL[np.float16]["bwd"])
    err = np.abs(got - ref)
    dq_within = bool(np.isfinite(got).all() and (err <= bound).all())
    dkdv_bitwise = bool(torch.equal(dK[0].view(torch.int16), dK[1].view(torch.int16))
                        and torch.equal(dV[0].view(torch.int16), dV[1].view(torch.int16)))

    med = {k: statistics.median(v) for k, v in times.items()}
    spread = (max(times[False]) - min(times[False])) / med[False]
    gain = (med[False] - med[True]) / med[False]
    return dict(
        policy=s["policy"], b=b, q_seq=list(s["qs"]), k_seq=list(s["ks"]), d=d, sync=s["sync"],
        control=bool(s.get("control", False)), chunks=int(plan[0]), chunk_keys=int(plan[1]), kv_copies=copies,
        calls_per_window={"plain": iters[False], "split": iters[True]},
        plain_ms=dict(median=med[False], min=min(times[False]), max=max(times[False])),
        split_ms=dict(median=med[True], min=min(times[True]), max=max(times[True])),
        speedup=med[False] / med[True],
        split_over_plain=med[True] / med[False],
        plain_spread=spread,
        faster_by_more_than_twice_the_spread=bool(gain > 2 * spread),
        partials_bytes=ws_bytes[True] - ws_bytes[False],
        # a chunk's fp32 partial (written once, read once by the reduce) beside the K and V bytes it reads
        workspace_traffic_share=nq * d * 4 / (plan[1] * (d + d) * 2),
        max_abs_diff_dQ=float(err.max()), max_diff_over_two_bounds=float((err / bound).max()),
        dQ_within_two_fp16_bwd_bounds=dq_within, dK_dV_bitwise_equal=dkdv_bitwise,
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--only", choices=("b16", "control"), help="the b = 16 table or the b = 1024 control alone")
    ap.add_argument("--index", type=int, action="append", help="only this entry of the shape list (repeatable): "
                    "one shape under a kernel trace keeps the per-kernel averages of that shape")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("splitk_bwd_time.py: no GPU; timings are only taken on the device")
    res = []
    for i, s in enumerate(SHAPES):
        if a.only and (a.only == "control") != bool(s.get("control", False)):
            continue
        if a.index and i not in a.index:
            continue
        r = time_shape(s, a.repeats, a.window_ms)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shapes=res), f, indent=1)
            f.write("\n")
    return 0 if all(r["dQ_within_two_fp16_bwd_bounds"] and r["dK_dV_bitwise_equal"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
