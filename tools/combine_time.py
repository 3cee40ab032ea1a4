"""The merge of attention partials, alone and inside combined attention, one process.

1. The merge kernel alone: fp16, b = 1024, nq = 4096, v_d = 64, N = 2 and N = 4 parts.  fa_merge_partials
   and a torch implementation of the same formulas (the only alternative without the kernel) run
   alternately on the same tensors, `--repeats` HIP-event windows each after a warm-up of both.  Reported:
   median / min / max and spread of both, the kernel's algorithmic bytes (N reads and one write of
   (v_d + 2) rows, l in fp32) per second as a share of the measured float4-copy rate (6.29 TB/s).
2. The merge's overhead: bench.py's config 4 (local_1d, window 256, 1024 slices of 16384 queries, d = 64)
   plus 16 global keys.  combined_1d, its two parts as separate calls (local_1d and full_1d over the 16
   keys) and local_1d alone run alternately, forward only and forward + backward.  combined minus the sum
   of the parts is the merge (forward) and the merge + accumulate (forward + backward) overhead; combined
   over local_1d alone is the price of the global tokens.  The bytes the merge and the accumulate move,
   at the copy rate, are reported beside the overhead.

    python tools/combine_time.py [--out profiles/combine_time.json] [--repeats 7] [--slices 1024]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flash_attention_amd import _lib  # noqa: E402
from tf_flash_attention_amd import flash_attention as fa  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s: measured float4 copy on MI355X


def alternate(fns, repeats, iters):
    """{name: [ms per call of each window]}: the windows of all fns interleaved, after a warm-up of each."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, n):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for fn in fns.values():
        window(fn, 2)
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def stats(ts):
    med = statistics.median(ts)
    return dict(median_ms=med, min_ms=min(ts), max_ms=max(ts), spread=(max(ts) - min(ts)) / med)


def torch_merge(Os, ls, ms):
    """The formulas of include/fa_api.h in torch (fp32 arithmetic, as the kernel)."""
    l = torch.stack(ls)
    m = torch.stack(ms).float()
    live = l != 0
    mx = torch.where(live, m, torch.full_like(m, float("-inf"))).amax(dim=0)
    e = l * torch.exp(torch.where(live, m - mx, torch.zeros_like(m)))
    L = e.sum(dim=0)
    w = e / L
    O = (w[:, :, None, :] * torch.stack(Os).float()).sum(dim=0).half()
    return O, L, mx.half()


def merge_alone(n, repeats, b=1024, nq=4096, v_d=64):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    Os = [(torch.rand((b, v_d, nq), generator=g, device=dev) * 4 - 2).half() for _ in range(n)]
    ls = [torch.rand((b, nq), generator=g, device=dev) * 49 + 1 for _ in range(n)]
    ms = [(torch.rand((b, nq), generator=g, device=dev) * 40 - 20).half() for _ in range(n)]
    times = alternate({"kernel": lambda: fa.merge_partials(Os, ls, ms), "torch": lambda: torch_merge(Os, ls, ms)},
                      repeats, iters=10)
    got, ref = fa.merge_partials(Os, ls, ms), torch_merge(Os, ls, ms)
    nbytes = (n + 1) * b * nq * (v_d * 2 + 4 + 2)
    k, t = stats(times["kernel"]), stats(times["torch"])
    return dict(what="merge_alone", n_parts=n, b=b, nq=nq, v_d=v_d, algo_bytes=nbytes, kernel=k, torch=t,
                kernel_bytes_per_s=nbytes / (k["median_ms"] * 1e-3),
                kernel_share_of_copy_rate=nbytes / (k["median_ms"] * 1e-3) / COPY_RATE,
                torch_over_kernel=t["median_ms"] / k["median_ms"],
                max_abs_diff_O=float((got[0].float() - ref[0].float()).abs().max()))


def overhead(slices, repeats, nq=16384, d=64, window=256, n_global=16):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *shape: (torch.rand(shape, generator=g, device=dev) * 4 - 2).half()  # noqa: E731
    Q, K, V, dO = (rnd(slices, d, nq) for _ in range(4))
    Kg, Vg = rnd(slices, d, n_global), rnd(slices, d, n_global)
    parts = lambda: [fa.Part("local", K, V, window_size=window), fa.Part("full", Kg, Vg)]  # noqa: E731
    res = []
    for bwd in (False, True):
        for t in (Q, K, V, Kg, Vg):
            t.requires_grad_(bwd)

        def run(f):
            def go():
                for t in (Q, K, V, Kg, Vg):
                    t.grad = None
                o = f()
                if bwd:
                    o.backward(dO)
            return go

        with torch.set_grad_enabled(bwd):
            times = alternate({
                "combined": run(lambda: fa.combined_1d(Q, parts())),
                "local": run(lambda: fa.local_1d(Q, K, V, window, 0, False, "none_front")),
                "global": run(lambda: fa.full_1d(Q, Kg, Vg)),
            }, repeats, iters=3)
        st = {k: stats(v) for k, v in times.items()}
        over = st["combined"]["median_ms"] - st["local"]["median_ms"] - st["global"]["median_ms"]
        lm = 4 + 2
        merge_bytes = 3 * slices * nq * (d * 2 + lm)
        acc_bytes = 3 * slices * nq * d * 2 if bwd else 0
        res.append(dict(what="overhead", backward=bwd, slices=slices, nq=nq, d=d, window=window, n_global=n_global,
                        **st, overhead_ms=over, combined_over_local=st["combined"]["median_ms"] / st["local"]["median_ms"],
                        merge_bytes=merge_bytes, accumulate_bytes=acc_bytes,
                        bytes_at_copy_rate_ms=(merge_bytes + acc_bytes) / COPY_RATE * 1e3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slices", type=int, default=1024)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians of alternated repeats)")
    if not torch.cuda.is_available():
        sys.exit("combine_time.py: no GPU; timings are only taken on the device")
    _lib.lib()
    res = [merge_alone(n, a.repeats) for n in (2, 4)]
    for r in res:
        print(json.dumps(r), flush=True)
    for r in overhead(a.slices, a.repeats):
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), copy_rate_bytes_per_s=COPY_RATE, results=res), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
