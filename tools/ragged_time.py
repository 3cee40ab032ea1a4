"""Ragged few-query forward against what a caller has without it, one process.

For each shape (16 sequences of Hk = 2 K/V heads, capacity 16384) the same seeded device inputs go alternately
through these runs, `--repeats` times each after a warm-up of all:
  base          fa_forward_grouped (fa_forward_ws for kv_group = 1) on the whole cache: no lengths at all;
  ragged_full   fa_forward_ragged with every length equal to the capacity: the same work as base, so the
                difference is the price of the length machinery;
  ragged        fa_forward_ragged with lengths drawn uniformly from [1, capacity] (fixed seed);
  loop          the per-sequence loop a caller runs today, on K / V already sliced to each length and made
                contiguous outside the window: one fa_forward_grouped (fa_forward_ws) per sequence;
  loop_copy     the same loop with the slice + .contiguous() copies inside the window.  (Neither loop pays the
                host synchronisation a caller needs to learn the lengths: they are known to this script.)
Every repeat is a HIP-event window over enough back-to-back calls to last about `--window-ms`.  Reported per
shape: median / min / max and spread ((max - min) / median) of each run; the price ragged_full / base - 1 and
whether it stays within twice the larger of the two spreads; ragged against both loops and against ragged_full;
the K + V bytes below the lengths over ragged's median time (and as a share of the 6.29 TB/s a device copy
reaches, profiles/combine_time.json); the largest |O_ragged - O_loop| with the fp16 forward tolerance of
tests/gate.py, and whether ragged_full's bits are base's (kv_group >= 2).

K and V rotate over several copies, so a call does not find its keys in the 256 MB last-level cache left by the
call before.  The last shapes (b_kv = 1024) are the control: the GPU is full either way; they skip the loops.

    python tools/ragged_time.py [--out profiles/ragged_time.json] [--repeats 7] [--window-ms 30]

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
CAP = 16384

SHAPES = (
    [dict(seqs=16, hk=2, g=g, nq=nq, d=d) for d in (64, 128) for g in (1, 4, 8) for nq in (1, 4)]
    + [dict(seqs=512, hk=2, g=4, nq=4, d=d, control=True) for d in (64, 128)]
)


def time_shape(s, repeats, window_ms):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    seqs, hk, g, nq, d, control = s["seqs"], s["hk"], s["g"], s["nq"], s["d"], bool(s.get("control", False))
    bkv, b = seqs * hk, seqs * hk * g
    problem = lambda batch, nk: _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, batch, (nq,), (nk,), d, d)  # noqa: E731
    prob = problem(b, CAP)
    plan = (ctypes.c_int32 * 6)()
    assert L.fa_forward_ragged_plan(prob, g, plan) == 0 and plan[0] >= 1, "shape is outside the fused envelope"
    ws_bytes = max(int(L.fa_forward_ragged_workspace_bytes(prob, g)), int(L.fa_forward_grouped_workspace_bytes(prob, g)), 1)

    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 4 - 2).half()  # noqa: E731
    kv_bytes = 2 * bkv * d * CAP * 2
    copies = max(1, min(8, -(-2 * LLC_BYTES // kv_bytes)))
    Q = rnd(b, d, nq)
    KV = [(rnd(bkv, d, CAP), rnd(bkv, d, CAP))]
    KV += [(KV[0][0].clone(), KV[0][1].clone()) for _ in range(copies - 1)]
    lens_np = np.random.default_rng(4321).integers(1, CAP + 1, seqs).astype(np.int32)
    lens = {"ragged_full": torch.full((seqs,), CAP, dtype=torch.int32, device=dev),
            "ragged": torch.from_numpy(lens_np).to(dev)}
    runs = ["base", "ragged_full", "ragged"] + ([] if control else ["loop", "loop_copy"])
    O = {r: torch.empty((b, d, nq), dtype=torch.float16, device=dev) for r in runs}
    l = torch.empty((b, nq), dtype=torch.float32, device=dev)
    m = torch.empty((b, nq), dtype=torch.float16, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def grouped(p, Qt, K, V, out, lo, mo):  # what the caller has today: no kv_group = 1 in fa_forward_grouped's plan
        return L.fa_forward_grouped(stream, p, g, Qt.data_ptr(), K.data_ptr(), V.data_ptr(), out.data_ptr(),
                                    lo.data_ptr(), mo.data_ptr(), ws.data_ptr(), ws_bytes)

    seq_prob = [problem(hk * g, int(n)) for n in lens_np]
    q0 = lambda i: slice(i * hk * g, (i + 1) * hk * g)  # noqa: E731
    k0 = lambda i: slice(i * hk, (i + 1) * hk)  # noqa: E731
    sliced = None if control else [[(K[k0(i), :, :n].contiguous(), V[k0(i), :, :n].contiguous())
                                    for i, n in enumerate(lens_np)] for K, V in KV]

    def call(run, it):
        K, V = KV[it % copies]
        if run == "base":
            st = grouped(prob, Q, K, V, O[run], l, m)
        elif run in lens:
            st = L.fa_forward_ragged(stream, prob, g, Q.data_ptr(), K.data_ptr(), V.data_ptr(), lens[run].data_ptr(), hk,
                                     0, O[run].data_ptr(), l.data_ptr(), m.data_ptr(), ws.data_ptr(), ws_bytes)
        else:
            st = 0
            for i, n in enumerate(lens_np):
                Ks, Vs = (sliced[it % copies][i] if run == "loop"
                          else (K[k0(i), :, :n].contiguous(), V[k0(i), :, :n].contiguous()))
                st = st or grouped(seq_prob[i], Q[q0(i)], Ks, Vs, O[run][q0(i)], l[q0(i)], m[q0(i)])
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
    for run in runs:  # warm-up of every run, and the calls per window from a first estimate
        window(run, 3)
        iters[run] = max(5, min(400, int(window_ms / max(window(run, 3), 1e-3)) + 1))
    times = {run: [] for run in runs}
    for _ in range(repeats):
        for run in runs:
            times[run].append(window(run, iters[run]))

    for run in runs:
        call(run, 0)
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(O["base"].view(torch.int16), O["ragged_full"].view(torch.int16)))
    med = {r: statistics.median(v) for r, v in times.items()}
    spread = {r: (max(v) - min(v)) / med[r] for r, v in times.items()}
    stats = lambda r: dict(median=med[r], min=min(times[r]), max=max(times[r]), spread=spread[r])  # noqa: E731
    price = med["ragged_full"] / med["base"] - 1.0
    live_bytes = 2 * hk * d * 2 * int(lens_np.astype(np.int64).sum())
    out = dict(
        sequences=seqs, kv_heads=hk, b_kv=bkv, kv_group=g, nq=nq, capacity=CAP, d=d, control=control,
        chunks=int(plan[0]), chunk_keys=int(plan[1]), pitch=int(plan[4]), folded_rows=int(plan[5]), kv_copies=copies,
        calls_per_window=iters, lengths=[int(n) for n in lens_np] if not control else None,
        mean_length_share=float(lens_np.mean() / CAP), **{r + "_ms": stats(r) for r in runs},
        # (a) the price of the length machinery: ragged_full against base, same work
        length_machinery_price=price,
        price_within_twice_the_larger_spread=bool(price <= 2 * max(spread["ragged_full"], spread["base"])),
        ragged_full_bits_are_base=same_bits if g >= 2 else None,
        # (b) random lengths
        ragged_over_ragged_full=med["ragged"] / med["ragged_full"],
        kv_bytes_capacity=kv_bytes, kv_bytes_below_lengths=live_bytes,
        ragged_live_bytes_per_s=live_bytes / (med["ragged"] * 1e-3),
        ragged_share_of_copy_rate=live_bytes / (med["ragged"] * 1e-3) / COPY_RATE,
        ragged_full_bytes_per_s=kv_bytes / (med["ragged_full"] * 1e-3),
        workspace_bytes=ws_bytes,
    )
    if not control:
        ref, got = O["loop"].double().cpu().numpy(), O["ragged"].double().cpu().numpy()
        rtol, atol = TOL[np.float16]["fwd"]
        scale = max(float(np.abs(ref).max()), 1.0)
        err = np.abs(got - ref)
        out.update(speedup_over_loop=med["loop"] / med["ragged"], speedup_over_loop_copy=med["loop_copy"] / med["ragged"],
                   max_abs_diff_O=float(err.max()), fp16_fwd_bound_min=atol * scale,
                   within_twice_fp16_fwd_tol=bool((err <= 2 * (atol * scale + rtol * np.abs(ref))).all()),
                   loops_equal=bool(torch.equal(O["loop"].view(torch.int16), O["loop_copy"].view(torch.int16))))
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
        sys.exit("ragged_time.py: no GPU; timings are only taken on the device")
    res = []
    for s in SHAPES:
        r = time_shape(s, a.repeats, a.window_ms)
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), copy_rate_bytes_per_s=COPY_RATE, shapes=res), f, indent=1)
            f.write("\n")
    return 0 if all(r.get("within_twice_fp16_fwd_tol", True) for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
