"""Run fp16 forward + backward over shapes outside the interval-rule / aligned envelope (strided and
2d local windows, lengths not divisible by 8, misaligned pointers, d <= 32), so a rocprofv3 kernel
trace shows which kernels serve them:

  rocprofv3 --kernel-trace --stats -d gpurun_out/disp -o run -- python3 tools/dispatch_trace.py

The two-pass backward (bwd_dkdv_kernel / bwd_dq_kernel) should be the only backward kernels in the
trace: no *_generic_*.

With the argument f64 it runs fp64 forward + backward at 128 < D <= 256 over every rule class instead
(the trace should show fwd_f64_kernel / bwd_dkdv_f64_kernel / bwd_dq_f64_kernel and no *_generic_*).
With f16w: fp16 at 128 < D <= 256 in the shapes past the 16-B chunk staging and the interval rules
(odd lengths, a misaligned pointer, strided 1d and 2d local windows): fwd_f16_wide_kernel and the
four-role bwd_dkdv_w4_kernel / bwd_dq_w4_kernel only, no *_generic_*.
With simt: one tiny forward + backward per dtype through the diagnostic library with FA_FWD_VARIANT =
FA_BWD_VARIANT = 9000, the pin that skips the MFMA dispatch: fwd_generic_ch_kernel, bwd_prep_kernel,
bwd_generic_ch_kernel and bwd_generic_ch_dq_kernel only (the torch kernels that fill the inputs aside).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if sys.argv[1:2] == ["simt"]:  # (before the package is imported: it reads FA_HIP_LIB once)
    os.environ["FA_HIP_LIB"] = os.path.join(ROOT, "tf_flash_attention_amd", "libfa_hip_diag.so")
    os.environ["FA_FWD_VARIANT"] = os.environ["FA_BWD_VARIANT"] = "9000"
from tf_flash_attention_amd import flash_attention as fa  # noqa: E402

SHAPES = [
    # policy, seq_dims, d, qs, ks, ws, ls, causal, misalign
    ("local", 1, 64, (520,), (520,), 20, 2, False, False),
    ("local", 2, 128, (24, 20), (24, 20), 5, 0, False, False),
    ("local", 2, 64, (16, 24), (20, 12), 3, 1, True, False),
    ("full", 1, 64, (263,), (517,), 1, 0, False, False),
    ("causal", 1, 128, (333,), (199,), 1, 0, False, False),
    ("full", 1, 64, (256,), (192,), 1, 0, False, True),
    ("causal", 1, 16, (200,), (200,), 1, 0, False, False),
]


SHAPES_F64 = [
    ("full", 1, 256, (131,), (197,), 1, 0, False, False),
    ("causal", 1, 256, (150,), (150,), 1, 0, False, False),
    ("local", 1, 200, (120,), (241,), 40, 0, True, False),
    ("local", 2, 256, (9, 14), (9, 14), 4, 2, True, False),
]


SHAPES_F16W = [
    ("full", 1, 256, (131,), (197,), 1, 0, False, False),
    ("causal", 1, 160, (150,), (75,), 1, 0, False, False),
    ("causal", 1, 256, (264,), (264,), 1, 0, False, True),
    ("local", 1, 256, (150,), (150,), 20, 3, False, False),
    ("local", 2, 200, (9, 14), (9, 14), 4, 2, True, False),
    ("local", 2, 256, (16, 24), (16, 24), 5, 0, False, False),
]


SHAPES_SIMT = [("causal", 1, 40, (33,), (70,), 1, 0, False, False)]


def choice_rows(dev):
    """One fa_forward per row of the CPU choice table (tests/test_fwd_choice.py, imported, in table order) whose
    operands take at most 1 GiB; prints each row with the kernel the table expects and, where the library has
    fa_forward_kernel, the one it names for the real pointers (asserted equal)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_fwd_choice as T
    from tf_flash_attention_amd import _lib
    L = _lib.lib()
    for name, kw, want in T.TABLE:
        p, off = T.problem(**kw), kw.get("off", (0, 0, 0))
        nq, nk = p.q_seq[0] * p.q_seq[1], p.k_seq[0] * p.k_seq[1]
        elt = {_lib.F16: 2, _lib.F32: 4, _lib.F64: 8}[p.dtype]
        sizes = [p.b * n * elt for n in (p.d * nq, p.d * nk, p.v_d * nk, p.v_d * nq)] + [p.b * nq * 8] * 2
        if want == "none" or sum(sizes) > 1 << 30:
            continue
        bufs = [torch.zeros(n + 16, dtype=torch.uint8, device=dev) for n in sizes]
        ptrs = [t.data_ptr() + o for t, o in zip(bufs, off + (0, 0, 0))]
        assert all(t.data_ptr() % 16 == 0 for t in bufs)
        named = "-"
        if hasattr(L, "fa_forward_kernel"):
            named = L.fa_forward_kernel(p, *ptrs[:3]).decode()
            assert named == want, (name, named, want)
        st = L.fa_forward(torch.cuda.current_stream().cuda_stream, p, *ptrs)
        torch.cuda.synchronize()
        assert st == 0, (name, _lib.last_error())
        print(f"row {name} {want} | {named}", flush=True)
    print("choice rows done")


def choice_check(rows_file, *ordered_files):
    """The ordered kernel lists (tools/trace_summary.py RUN_DIR --ordered) of runs of `choice` are equal, and row by
    row the kernel each row of `rows_file` (a run's output) names."""
    rows = [ln.split(" | ")[0].split(" ", 2)[2] for ln in open(rows_file) if ln.startswith("row ")]
    lists = [[ln.strip() for ln in open(f) if ln.strip()] for f in ordered_files]
    assert all(x == lists[0] for x in lists), "the runs launched different kernels"
    assert len(rows) == len(lists[0]), (len(rows), len(lists[0]))
    for want, got in zip(rows, lists[0]):
        family = want in ("fwd_f32", "fwd_f64", "fwd_generic")  # (named by family: any kernel of it)
        assert f"::{want}_" in got if family else f"::{want}(" in got, (want, got)
    print(f"{len(ordered_files)} traces of {len(rows)} launches: equal, and each the kernel its row names")


def main():
    if sys.argv[1:2] == ["choice-check"]:
        return choice_check(*sys.argv[2:])
    dev = torch.device("cuda:0")
    if sys.argv[1:2] == ["choice"]:
        return choice_rows(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    shapes = {"f64": SHAPES_F64, "f16w": SHAPES_F16W, "simt": SHAPES_SIMT}.get(mode, SHAPES)
    dtypes = {"f64": [torch.float64], "simt": [torch.float16, torch.float32, torch.float64]}.get(mode, [torch.float16])
    for dt, (policy, sd, d, qs, ks, ws, ls, causal, mis) in ((dt, s) for dt in dtypes for s in shapes):
        def mk(shape):
            n = 1
            for x in shape:
                n *= x
            buf = (torch.rand(n + 1, generator=g, device=dev, dtype=torch.float64) * 4 - 2).to(dt)
            t = (buf[1:] if mis else buf[:n]).view(shape)
            return t.requires_grad_(True)
        q, k, v = mk((2, d) + qs), mk((2, d) + ks), mk((2, d) + ks)
        o, l, m = fa.attention_forward(policy, sd, q, k, v, "none_front", ws, ls, causal)
        fa.attention_backward(policy, sd, q, k, v, o, l, m, torch.ones_like(o), "none_front", ws, ls, causal)
    torch.cuda.synchronize()
    print("dispatch trace shapes done")


if __name__ == "__main__":
    main()
