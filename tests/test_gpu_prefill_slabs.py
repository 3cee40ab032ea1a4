"""GPU test of the batch-slab launch loop (fewq_slabs, csrc/fa_api.hip) behind the query-blocked
entry points, in the manner of tests/test_gpu_window_slabs.py and with tests/test_gpu_slabs.py's
inputs: the diagnostic library lowers the slab limit to FA_SLAB_MAX K/V slices and counts the slab launches, each of
which is one partial and one merge launch.  The capped call is bitwise the uncapped one, the uncapped one passes
test_gpu_ragged._check_ref, and the counter rose by ceil(slices / cap) > 1.  70 queries at g = 2 are two blocks of 64,
so a slab's workspace offset counts the block axis; every cap but 1 makes a slab straddle two sequences, so len0 and
rem0 pick the length that a block's key end is formed from, the table row and the head's scales."""

import ctypes

import pytest
import torch

from tests import test_gpu_ragged as rg
from tests import test_gpu_slabs as sl
from tests.test_gpu_parity import diag_lib  # noqa: F401  (a fixture)
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

NQ = 70


@pytest.mark.parametrize("d,vd,tail", [(64, 64, True), (64, 64, False), (96, 40, True)])
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_prefill_wrappers(monkeypatch, diag_lib, form, fp8, d, vd, tail):  # noqa: F811
    bkv = sl.SEQS * sl.HK
    sl._check_caps(sl.DECODE_CAPS, bkv)
    plan = (ctypes.c_int32 * 8)()
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, bkv * sl.G, (NQ,), (sl.PAGE * sl.MAX_PAGES,), d, vd)
    assert diag_lib.fa_forward_ragged_prefill_plan(prob, sl.G, plan) == _lib.FA_OK
    assert tuple(plan[:6]) == (1, 1024, 64, 128, 2, 0)
    args, scales, (Q, Kref, Vref, kv_lens) = sl._decode_case(form, fp8, d, vd, NQ, seed=1000 * d + tail)
    wrapper = fa.ragged_prefill_1d if form == "ragged" else fa.paged_prefill_1d

    def call():
        with torch.no_grad():
            out = wrapper(*args, tail_causal=tail, returning_l_m=True, **scales)
        return tuple(t.reshape((-1,) + t.shape[2:]) for t in out)

    ref = sl._run(monkeypatch, diag_lib, None, bkv, call)
    res = rg._check_ref(ref, Q, Kref, Vref, kv_lens, sl.G, tail)
    print(f"{form} fp8={fp8} d={d} vd={vd} tail={tail}: worst error / allowance {res}")
    for cap in sl.DECODE_CAPS:
        assert -(-bkv // cap) > 1
        assert sl._same(sl._run(monkeypatch, diag_lib, cap, bkv, call), ref), cap
