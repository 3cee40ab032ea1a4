"""Split-query backward against the two-pass backward on few-key shapes, one process.

The mirror of tools/splitk_bwd_time.py, same protocol.  For each shape the same seeded device inputs (and the
forward's O, l, m) go alternately through fa_backward (its dK/dV pass runs one workgroup per slice for these
shapes: the path every caller took before the split dK/dV pass) and fa_backward_split, `--repeats` times each
after a warm-up of both.  Every repeat is a HIP-event window over enough back-to-back calls to last about
`--window-ms`.  Reported per shape: the median / min / max time of both paths, their ratio, the spread
(max - min over the median) of the fa_backward path, whether the split path is faster by more than twice
that spread, the workspace traffic share nk*(d + v_d)*4 / (chunk*(d + v_d)*2) (a chunk's partial beside the
Q / dO bytes it reads), and the largest |dK_split - dK_plain| and |dV_split - dV_plain| with twice the plain
fp16 backward bound of tests/gate.py they must stay within (dQ must be bitwise equal).

Here the big tensors are Q and dO: they rotate over several copies, so a call does not find its queries in
the 256 MB last-level cache left by the call before.  The last shapes (b = 1024) are the control: the GPU is
full without splitting.

    python tools/splitq_bwd_time.py [--out profiles/splitq_bwd_time.json] [--repeats 7] [--window-ms 30]
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
from splitkv_time import LLC_BYTES, POL, SYNC  # noqa: E402
from tests.gate import TOL, plain_bound  # noqa: E402
from tf_flash_attention_amd import _lib  # noqa: E402

SHAPES = (
    [dict(policy="full", b=16, qs=(16384,), ks=(nk,), d=d, sync="none_front") for nk in (32, 77, 128) for d in (64, 128)]
    + [dict(policy="causal", b=16, qs=(16384,), ks=(128,), d=d, sync="scale_end") for d in (64, 128)]
    + [dict(policy="full", b=1024, qs=(4096,), ks=(128,), d=d, sync="none_front", control=True) for d in (64, 128)]
)


def time_shape(s, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b, d = s["b"], s["d"]
    nq, nk = math.prod(s["qs"]), math.prod(s["ks"])
    prob = _lib.make_problem(_lib.F16, POL[s["policy"]], len(s["qs"]), SYNC[s["sync"]], b, s["qs"], s["ks"], d, d)
    plan = (ctypes.c_int32 * 4)()
    assert L.fa_backward_split_q_plan(prob, plan) == 0 and plan[0] >= 2, "shape does not split"
    ws_bytes = {False: int(L.fa_backward_workspace_bytes(prob)), True: int(L.fa_backward_split_workspace_bytes(prob))}

    g = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=g, device=dev) * 4 - 2).half()  # noqa: E731
    qo_bytes = 2 * b * d * nq * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // qo_bytes)))
    K, V = rnd(b, d, nk), rnd(b, d, nk)
    QO = [(rnd(b, d, nq), rnd(b, d, nq))]
    QO += [(QO[0][0].clone(), QO[0][1].clone()) for _ in range(copies - 1)]
    O = torch.empty((b, d, nq), dtype=torch.float16, device=dev)
    l = torch.empty((b, nq), dtype=torch.float32, device=dev)
    m = torch.empty((b, nq), dtype=torch.float16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    st = L.fa_forward(stream, prob, QO[0][0].data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), l.data_ptr(),
                      m.data_ptr())
    if st != 0:
        raise RuntimeError(_lib.last_error())
    dQ = [torch.empty_like(QO[0][0]) for _ in range(2)]
    dK = [torch.empty_like(K) for _ in range(2)]
    dV = [torch.empty_like(V) for _ in range(2)]
    ws = torch.empty(ws_bytes[True], dtype=torch.uint8, device=dev)

    def call(split, i):
        Q, dO = QO[i % copies]
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
    diffs, within = {}, True
    for name, t in (("dK", dK), ("dV", dV)):
        ref, got = t[0].double().cpu().numpy(), t[1].double().cpu().numpy()
        bound = 2.0 * plain_bound(ref, *TOL[np.float16]["bwd"])
        err = np.abs(got - ref)
        within = within and bool(np.isfinite(got).all() and (err <= bound).all())
        diffs[name] = dict(max_abs_diff=float(err.max()), max_diff_over_two_bounds=float((err / bound).max()))
    dq_bitwise = bool(torch.equal(dQ[0].view(torch.int16), dQ[1].view(torch.int16)))

    med = {k: statistics.median(v) for k, v in times.items()}
    spread = (max(times[False]) - min(times[False])) / med[False]
    gain = (med[False] - med[True]) / med[False]
    return dict(
        policy=s["policy"], b=b, q_seq=list(s["qs"]), k_seq=list(s["ks"]), d=d, sync=s["sync"],
        control=bool(s.get("control", False)), chunks=int(plan[0]), chunk_queries=int(plan[1]), q_dO_copies=copies,
        calls_per_window={"plain": iters[False], "split": iters[True]},
        plain_ms=dict(median=med[False], min=min(times[False]), max=max(times[False])),
        split_ms=dict(median=med[True], min=min(times[True]), max=max(times[True])),
        speedup=med[False] / med[True],
        split_over_plain=med[True] / med[False],
        plain_spread=spread,
        faster_by_more_than_twice_the_spread=bool(gain > 2 * spread),
        partials_bytes=ws_bytes[True] - ws_bytes[False],
        # a chunk's fp32 partial (written once, read once by the reduce) beside the Q and dO bytes it reads
        workspace_traffic_share=nk * (d + d) * 4 / (plan[1] * (d + d) * 2),
        dK=diffs["dK"], dV=diffs["dV"],
        dK_dV_within_two_fp16_bwd_bounds=within, dQ_bitwise_equal=dq_bitwise,
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
        sys.exit("splitq_bwd_time.py: no GPU; timings are only taken on the device")
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
    return 0 if all(r["dK_dV_within_two_fp16_bwd_bounds"] and r["dQ_bitwise_equal"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
