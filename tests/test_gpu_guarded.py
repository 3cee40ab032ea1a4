"""The dense kernels behind guard bands and under mixed alignments (tests/guarded.py), through the C ABI of the
product library: fa_forward / fa_forward_ws and fa_backward_split, the calls the torch wrappers make.

Every other test reaches these kernels through the wrappers, whose outputs are fresh 256-byte aligned torch.empty
tensors and whose inputs move together if they move at all.  Here every tensor sits between 4096-byte guard bands, and
for each case and each alignment variant (no tensor, every tensor, each tensor alone one element off a 16-byte
boundary) the call runs twice: run A with NaN (0xFF) around the inputs and 0xA5 in and around the outputs and the
workspace, run B with zeros and 0x5A.  Asserted: both statuses, every guard intact, every input unchanged, run A's
outputs bitwise run B's, and run A within run_case's unchanged tolerances of the float64 oracle (computed once a case).

A variant that moves K or V re-routes a call (the 16-byte staging kernels decline): that is intended, the subject is
the contract of include/fa_api.h, which asks for element alignment only.  The workspace stays 256-byte aligned.

b = 3 (a first, a middle and a last slice), inputs U(-2, 2) from a per-case seed.  The shapes are the smallest that
keep a ragged tail on every axis where the family can have one.  The route beside each case is read from
fa_forward / fa_backward (fa_api.hip), fwd_f16_choice (fa_fwd_f16_choice.h; fa_forward_kernel names its result),
fwd_f16_band_positions (fa_fwd_f16_band.hip), with_pol_fast / fast_staging (fa_fwd_f16_core.h), launch_bwd_f16_fast / launch_prep / launch_dkdv_pass (fa_bwd_f16_fast.hip), launch_bwd_f16_dq
(fa_bwd_f16_dq.hip), bwd_aligned / with_pol_aln (fa_bwd_f16_parts.h), launch_bwd_f16_wide, launch_fwd_f32 /
launch_bwd_f32, launch_fwd_f64 / launch_bwd_f64 and fa_generic.hip, for the variant "none"; the three split plans are
asserted, in both directions."""
import ctypes
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from tests import guarded
from tests.test_gpu_parity import check_outputs, diag_lib, oracle_outputs  # noqa: F401  (diag_lib is a fixture)

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64


@dataclass
class Case:
    id: str
    dtype: type
    policy: str
    d: int
    vd: int
    qs: tuple
    ks: tuple
    mode: str = "none_front"
    ws: int = 1
    ls: int = 0
    causal: bool = False
    b: int = 3
    split: str = ""            # "k": fa_forward_split_plan and fa_backward_split_plan, "q": fa_backward_split_q_plan


def _c(id, dtype, policy, d, vd, qs, ks, **kw):
    qs, ks = ((qs,), (ks,)) if isinstance(qs, int) else (tuple(qs), tuple(ks))
    return Case(id, dtype, policy, d, vd, qs, ks, **kw)


# Backward routes, fp16 (launch_bwd_f16_fast): launch_prep -> bwd_prep8_kernel where nq % 8 == 0 and O, dO are 16-byte
# aligned, else bwd_prep_kernel; max(d, v_d) <= 64: bwd_dkdv_kernel<64, 4, 2, POL, ALN> + bwd_dq_kernel<64, 4, 2, POL,
# ALN>; <= 128: bwd_dkdv_pc_kernel<128, POL, ALN> + (ALN ? bwd_dq_pc_kernel<128> : bwd_dq_kernel<128, 4, 1>); <= 256:
# bwd_dkdv_w4_kernel<POL, ALN> + bwd_dq_w4_kernel<POL, ALN>.  ALN = bwd_aligned: Q, K, V, dO 16-byte aligned and
# nq % 8 == nk % 8 == 0; POL 0 full, 1 interval rules, 2 other windows.  "bwd ALN / elem" below names which.
CASES = [
    # fwd_f16_kernel<32, 4, POL 0, elem> (launch_t<32, 4, 8>: max(d, v_d) <= 32 is below the tuned kernels;
    # d != 32, so fast_staging declines); bwd elem, prep
    _c("f16-core-d32-full", F16, "full", 24, 20, 37, 75),
    # fwd_f16_kernel<64, 8, POL 0, elem> (nk % 8 != 0: not fwd_f16_tuned_operands, not fast_staging); bwd elem, prep
    _c("f16-core-d64-full-elem", F16, "full", 64, 64, 37, 77),
    # fwd_f16_kernel<128, 4, POL 1, elem>; bwd elem: bwd_dkdv_pc_kernel<128, 1, false> + bwd_dq_kernel<128, 4, 1, 1, false>
    _c("f16-core-d128-causal-elem", F16, "causal", 128, 128, 77, 77),
    # fwd_f16_kernel<64, 4, POL 2, FAST> (a 2d window is no interval rule; nk = 72, d = v_d = 64: 16-byte staging);
    # bwd ALN POL 2, prep8 (nq = 72)
    _c("f16-core-d64-local2d", F16, "local", 64, 64, (9, 8), (9, 8), ws=3),
    # fwd_f16_pingpong_kernel with qvec (nq % 8 == 0, Q aligned); bwd ALN, prep8
    _c("f16-pingpong-qvec", F16, "full", 48, 64, 72, 136),
    # fwd_f16_pingpong_kernel, element-wise Q (nq = 37); bwd elem, prep
    _c("f16-pingpong-ragged-q", F16, "full", 64, 40, 37, 136),
    # fwd_f16_fast_kernel<64, 8, POL 1> (causal: an interval rule, not a 1d window); bwd ALN POL 1, prep8
    _c("f16-8wave-d64-causal", F16, "causal", 64, 40, 136, 136),
    # fwd_f16_band_kernel: 1d window, ls = 0, 32 < d <= 64 = v_d, nq % 8 == nk % 8 == 0, Q / K / V aligned; two
    # 256-query blocks a slice, the second with 8 queries; bwd ALN POL 1, prep8
    _c("f16-band-local", F16, "local", 40, 64, 264, 264, ws=40),
    # the same kernel, causal window, nq != nk under scale_front
    _c("f16-band-local-causal", F16, "local", 64, 64, 264, 528, ws=40, causal=True, mode="scale_front"),
    # fwd_f16_fast_kernel<64, 4, POL 1> (v_d = 48 != 64: fwd_f16_band_positions declines)
    _c("f16-4wave-d64-local", F16, "local", 64, 48, 264, 264, ws=40),
    # fwd_f16_gap128_kernel<0>; bwd ALN: bwd_dkdv_pc_kernel<128, 0, true> + bwd_dq_pc_kernel<128, 0, true>, prep8
    _c("f16-gap128-full", F16, "full", 96, 128, 72, 136),
    # fwd_f16_gap128_kernel<1>, two 256-query blocks (a heavy / light pair)
    _c("f16-gap128-causal", F16, "causal", 128, 72, 264, 264),
    # fwd_f16_fast_kernel<128, 4, POL 1> (policy 2 skips the gap-stream and ping-pong kernels)
    _c("f16-4wave-d128-local", F16, "local", 128, 128, 264, 264, ws=40),
    # fwd_f16_wide_kernel<0, true>; bwd_dkdv_w4_kernel<0, true> + bwd_dq_w4_kernel<0, true>, prep8
    _c("f16-wide-full", F16, "full", 160, 200, 72, 136),
    # fwd_f16_wide_kernel<1, true>; d = 256: the dQ epilogue's 2-byte buffer stores
    _c("f16-wide-causal", F16, "causal", 256, 256, 136, 136),
    # fwd_f16_wide_kernel<0, false> (nk = 77); bwd w4 <0, false>, prep
    _c("f16-wide-full-elem", F16, "full", 130, 256, 37, 77),
    # fwd_f16_wide_kernel<2, false> (a strided window is no interval rule; nk = 75); bwd w4 <2, false>, prep
    _c("f16-wide-strided", F16, "local", 200, 160, 75, 75, ws=9, ls=2),
    # splitk_partial_kernel + splitk_merge_kernel (fa_forward_ws: one query block, 2056 keys in 5 chunks of 512);
    # fa_backward_split: prep + bwd_dkdv_kernel<64, 4, 2> + bwd_dq_kernel<64, ..., split> + dq_split_reduce_kernel
    _c("f16-splitk-d64", F16, "full", 64, 40, 33, 2056, b=2, split="k"),
    # the same at D = 128, one query; bwd_dkdv_pc_kernel<128> + bwd_dq_kernel<128, 4, 1, ..., split> + the reduce
    _c("f16-splitk-d128-q1", F16, "causal", 128, 128, 1, 2056, mode="scale_end", b=2, split="k"),
    # fwd_f16_kernel<64, 8, 0, elem> (nk = 77); backward_split_q: prep8 + bwd_dkdv_kernel<64, 4, 2, 0, false, 1, split>
    # over 3 chunks of 1024 queries + dkdv_split_reduce_kernel + bwd_dq_kernel<64, 4, 2>
    _c("f16-splitq-d64", F16, "full", 64, 64, 2056, 77, b=2, split="q"),
    # fwd_f32_kernel<32> / bwd_f32 launch_t<32>
    _c("f32-d32-full", F32, "full", 24, 20, 37, 75),
    # fwd_f32_kernel<64> / bwd_f32 launch_t<64> with its qvec (nq % 4 == 0, Q and dO aligned)
    _c("f32-d64-causal-qvec", F32, "causal", 64, 64, 76, 76),
    # fwd_f32_kernel<128> / bwd_f32 launch_t<128>
    _c("f32-d128-local-causal", F32, "local", 100, 128, 37, 75, ws=20, causal=True),
    # fa_fwd_f32_wide.hip (32-key tiles) / fa_bwd_f32_wide.hip (16x16x4 MFMAs)
    _c("f32-wide-full", F32, "full", 160, 130, 37, 75),
    # fa_f64.hip launch_fwd_t<32> / launch_bwd_t<32>
    _c("f64-d32-full", F64, "full", 24, 20, 37, 75),
    # launch_fwd_t<128> / launch_bwd_t<128>
    _c("f64-d128-causal", F64, "causal", 100, 128, 37, 75),
    # launch_fwd_t<256> / launch_bwd_t<256>: dK / dV in channel quarters, dQ in halves per launch
    _c("f64-d256-local-causal", F64, "local", 200, 160, 37, 75, ws=20, causal=True),
    # fa_generic.hip's channel-chunked SIMT kernels, both directions (no MFMA predicate takes 257 channels)
    _c("f16-simt-d257", F16, "full", 257, 260, 33, 70),
    _c("f32-simt-d257", F32, "full", 257, 260, 33, 70),
    _c("f64-simt-d257", F64, "full", 257, 260, 33, 70),
]
# The ping-pong kernel at 64 < d <= 128 (csrc/diag/fa_fwd_f16_pingpong128.hip) is a study: the gap-stream kernel takes
# every shape it takes, so only the diagnostic library holds it, behind FA_FWD_VARIANT=2301.  Forward only.
PINGPONG128 = _c("diag-2301-pingpong128", F16, "full", 128, 128, 72, 136)


def _problem(case):
    from tf_flash_attention_amd import _lib
    dt = {F16: _lib.F16, F32: _lib.F32, F64: _lib.F64}[case.dtype]
    pol = {"full": _lib.FULL, "causal": _lib.CAUSAL, "local": _lib.LOCAL}[case.policy]
    sync = {"none_front": _lib.NONE_FRONT, "scale_front": _lib.SCALE_FRONT, "scale_end": _lib.SCALE_END}[case.mode]
    return _lib.make_problem(dt, pol, len(case.qs), sync, case.b, case.qs, case.ks, case.d, case.vd, case.ws, case.ls,
                             case.causal)


def _assert_plans(case, L, prob):
    """Each split plan is active exactly where the case says so, with at least two chunks."""
    for key, fn in (("k", L.fa_forward_split_plan), ("k", L.fa_backward_split_plan), ("q", L.fa_backward_split_q_plan)):
        out = (ctypes.c_int32 * 4)()
        assert fn(prob, out) == 0
        if case.split == key:
            assert out[0] >= 2, (case.id, fn.__name__, tuple(out))
        else:
            assert out[0] == 0, (case.id, fn.__name__, tuple(out))
    assert (L.fa_forward_workspace_bytes(prob) > 0) == (case.split == "k")


def _run(case, variants=None, bwd=True):
    from tf_flash_attention_amd import _lib
    L = _lib.lib()
    prob = _problem(case)
    _assert_plans(case, L, prob)
    dt, b, d, vd = case.dtype, case.b, case.d, case.vd
    nq, nk = int(np.prod(case.qs)), int(np.prod(case.ks))
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    arrays = {n: rng.uniform(-2, 2, s).astype(dt)
              for n, s in (("Q", (b, d, nq)), ("K", (b, d, nk)), ("V", (b, vd, nk)), ("dO", (b, vd, nq)))}
    ldt = np.float32 if dt == F16 else dt
    specs = {"O": ((b, vd, nq), dt), "l": ((b, nq), ldt), "m": ((b, nq), dt),
             "dQ": ((b, d, nq), dt), "dK": ((b, d, nk), dt), "dV": ((b, vd, nk), dt)}
    seq = {"Q": case.qs, "dO": case.qs, "O": case.qs, "l": case.qs, "m": case.qs, "dQ": case.qs,
           "K": case.ks, "V": case.ks, "dK": case.ks, "dV": case.ks}
    shaped = lambda n, x: x.reshape(x.shape[:x.ndim - 1] + seq[n])  # noqa: E731  ([b, ch, n] -> [b, ch, *seq])
    rule = (case.policy, len(case.qs), case.mode)
    win = (case.ws, case.ls, case.causal)
    ins = tuple(shaped(n, arrays[n]) for n in ("Q", "K", "V", "dO"))
    oracle = oracle_outputs(dt, *rule, *win, *ins, list(range(b)), bwd)     # once: every variant has the same values
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    fwd_ws = int(L.fa_forward_workspace_bytes(prob))
    bwd_ws = int(L.fa_backward_split_workspace_bytes(prob))
    assert bwd_ws > 0

    def forward(bufs, ws):             # attention_forward's own branch
        p = [bufs[n].data_ptr() for n in ("Q", "K", "V", "O", "l", "m")]
        if fwd_ws:
            return L.fa_forward_ws(stream, prob, *p, ws.data_ptr(), fwd_ws)
        return L.fa_forward(stream, prob, *p)

    def backward(bufs, ws):            # attention_backward's call
        p = [bufs[n].data_ptr() for n in ("Q", "K", "V", "O", "l", "m", "dO", "dQ", "dK", "dV")]
        return L.fa_backward_split(stream, prob, *p, ws.data_ptr(), bwd_ws)

    def check(variant, res):
        r = {n: shaped(n, x) for n, x in res.items()}
        try:
            check_outputs(dt, *rule, d, vd, case.qs, case.ks, *win, *ins, r["O"], r["l"], r["m"],
                          (r["dQ"], r["dK"], r["dV"]) if bwd else None, oracle=oracle)
        except AssertionError as e:
            raise AssertionError(f"{case.id} [{variant}] run A against the float64 oracle: {e}") from e

    with torch.cuda.device(dev):
        guarded.guarded_case(case.id, arrays, specs, dev, forward, backward if bwd else None, fwd_ws, bwd_ws, check,
                             variants)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_guard_bands_and_alignments(case):
    _run(case)


def test_guard_bands_pingpong128(monkeypatch, diag_lib):  # noqa: F811
    monkeypatch.setenv("FA_FWD_VARIANT", "2301")
    variants = ["none", "Q", "O"]
    before = diag_lib.fa_diag_call_count(0)
    _run(PINGPONG128, variants, bwd=False)
    assert diag_lib.fa_diag_call_count(0) == before + 2 * len(variants)   # the diagnostic library made the calls
