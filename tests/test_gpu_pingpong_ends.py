"""GPU tests of the ends of fwd_f16_pingpong_kernel's key loop (fa_fwd_f16_pingpong.hip): the drain that
replaces the steps past the last tile, and the independence of a query block from the launch it is in.

The loop runs whole groups of three key tiles; the ntiles mod 3 tiles left run as iterations without
staging, and the PV of the last tile runs on its own after the wave's last barrier.  The drain cases
take tile counts 1-7 (every residue mod 3, with and without a masked tail tile, and fewer tiles than one
group), a ragged second query block whose last waves are inactive, and the generic epilogue
(d, v_d) = (40, 48).  The staircase cases put a lazy rebase on the last tile, once in a drain iteration
and once in the loop's last step, so the PV that follows the loop carries a rescaled O.

The many-items cases launch at least four query blocks per CU with a ragged last block per slice; the
independence cases run the same inputs whole and in batch slabs of fewer than two blocks per CU and ask
for the same bits on every slice (a block's result may not depend on what the launch holds beside it).

Every shape is first shown to reach this kernel: full policy, 32 < max(d, v_d) <= 64, nk % 8 == 0, and
no split-key plan.  Checks are run_case's (float64 oracle, its tolerances, forward only)."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import fa_oracle as O
from tests import score_ramp as R
from tests.test_gpu_parity import run_case

pytestmark = pytest.mark.gpu

KBN = 64     # keys per tile
KBM = 256    # queries per block


def _assert_pingpong(policy, d, vd, nq, nk, b):
    """The dispatcher's conditions for fwd_f16_pingpong_kernel (fwd_f16_choice, csrc/fa_fwd_f16_choice.h)."""
    from tf_flash_attention_amd import _lib
    assert policy == "full"
    assert 32 < max(d, vd) <= 64
    assert nk % 8 == 0 and nk > 0
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (nk,), d, vd)
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fa_forward_split_plan(prob, out) == 0
    assert out[0] == 0, tuple(out)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------ the drain
@pytest.mark.parametrize("d,vd", [(64, 64), (40, 48)])
@pytest.mark.parametrize("nq", [40, 300])
@pytest.mark.parametrize("nk", [8, 64, 72, 128, 136, 192, 200, 256, 392, 448])
def test_drain(nk, nq, d, vd):
    _assert_pingpong("full", d, vd, nq, nk, 3)
    run_case(np.float16, "full", 1, "none_front", (3,), d, vd, (nq,), (nk,), seed=nk + nq, bwd=False)


# nk = 456: 8 tiles, the tail tile is the second drain iteration; nk = 520: 9 tiles, the tail tile is the
# loop's last step and the PV after the loop follows it directly.  Plateaus of one tile: a climb row
# rebases on every tile up to the third from last, not on the second from last, and again on the last
# (score_ramp: the steps towards the top are ..., 4σ0, 2σ0, σ0 with 8/3 < σ0 <= 4).
@pytest.mark.parametrize("nk", [456, 520])
def test_staircase_across_the_drain(nk):
    case = R._c(f"f16-pingpong-ends-nk{nk}", np.float16, "full", "none_front", 64, 64, 300, nk, KBN, KBN, bwd=False)
    _assert_pingpong(case.policy, case.d, case.vd, 300, nk, int(np.prod(case.batch)))
    inputs, info = case.inputs()
    Q, K = (R._flat3(x, 1) for x in inputs[:2])
    rebased, active = R.rebase_tiles(R.kernel_scores(Q, K, case.d, True), info["mask"], KBN, case.thr)
    climb = info["kind"] == R.CLIMB
    nt = (nk + KBN - 1) // KBN
    assert rebased[climb, nt - 1].any() and rebased[climb, nt - 3].any() and not rebased[~climb].any()
    run_case(case.dtype, case.policy, 1, case.mode, case.batch, case.d, case.vd, case.qs, case.ks, bwd=False,
             inputs=inputs, m_bound=R.m_rounding_bound(Q, K, info, case.dtype, case.d))


# ------------------------------------------------------------------------------------------ many items
@pytest.mark.parametrize("nk", [200, 392])
def test_many_items(nk):
    cus = _cus()
    batch = (4, -(-(cus + 1) // 4))
    b, nq = int(np.prod(batch)), 1000
    assert b * (-(-nq // KBM)) >= 4 * cus
    _assert_pingpong("full", 64, 64, nq, nk, b)
    run_case(np.float16, "full", 1, "none_front", batch, 64, 64, (nq,), (nk,), seed=nk, bwd=False,
             slices=sorted({0, 1, b // 3, b // 2 + 1, b - 2, b - 1}))


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "alternate-q-times-8"])
def test_block_is_independent_of_the_launch(hot):
    """The same inputs in one launch of >= 4 blocks per CU and in slabs of fewer than 2 blocks per CU: O, l and m
    bitwise equal on every slice.  `hot`: every other slice's Q scaled by 8, so that a running max, a rebase
    threshold or a packed-P maximum left over from a block with large scores would show in the cold
    block a workgroup (or a CU) takes next."""
    from tf_flash_attention_amd import flash_attention as fa
    cus = _cus()
    nq, nk, d = 1000, 392, 64
    nqb = -(-nq // KBM)
    b = 4 * -(-(cus + 1) // 4)
    slab = (2 * cus - 1) // nqb
    assert b * nqb >= 4 * cus and slab * nqb < 2 * cus and slab >= 1
    _assert_pingpong("full", d, d, nq, nk, b)
    _assert_pingpong("full", d, d, nq, nk, slab)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    q, k, v = ((torch.rand((b, d, n), generator=g, device=dev) * 4 - 2).half() for n in (nq, nk, nk))
    if hot:
        q[::2] *= 8
    whole = fa.full_1d(q, k, v, returning_l_m=True)
    for s in range(0, b, slab):
        part = fa.full_1d(q[s:s + slab], k[s:s + slab], v[s:s + slab], returning_l_m=True)
        for name, w, p in zip("Olm", whole, part):
            assert torch.equal(w[s:s + slab], p), f"{name}: slices {s}..{s + slab - 1} differ between the launches"
    # and the whole launch is right where the oracle is taken: odd slices, the ones never scaled (the
    # tolerance is run_case's for U(-2, 2) inputs)
    sl = [1, b // 2 + 1, b - 1]   # (b is a multiple of 4)
    O64, _, _, _ = O.forward_f64(q[sl].cpu().numpy(), k[sl].cpu().numpy(), v[sl].cpu().numpy(),
                                 O.Problem("full", 1, "none_front"))
    err = np.abs(whole[0][sl].float().cpu().numpy().astype(np.float64) - O64)
    assert (err <= 1e-3 * max(np.abs(O64).max(), 1.0) + 1e-3 * np.abs(O64)).all(), err.max()
