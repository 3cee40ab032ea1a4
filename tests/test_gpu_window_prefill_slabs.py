"""GPU test of the batch-slab launch loop (fewq_slabs, csrc/fa_api.hip) behind the sliding-window
prefill entry points, in the manner of tests/test_gpu_prefill_slabs.py and with tests/test_gpu_slabs.py's
inputs: the diagnostic library lowers the slab limit to FA_SLAB_MAX K/V slices and counts the slab launches.  The
capped call is bitwise the uncapped one, the uncapped one passes the window's gate
(tests/test_gpu_window._check_window), and the counter rose by ceil(slices / cap) > 1.  70 queries at g = 2 are two
blocks of 64 under a window of 40 keys over a capacity of 256, so the plan is the form's own, a slab's workspace offset
counts the block axis, and every cap but 1 makes a slab straddle two sequences: len0 and rem0 pick the length that a
block's L_b and lo_b are formed from, the table row and the head's scales."""

import ctypes

import numpy as np
import pytest
import torch

from tests import test_gpu_slabs as sl
from tests import test_gpu_window as gw
from tests.test_gpu_parity import diag_lib  # noqa: F401  (a fixture)
from tf_flash_attention_amd import _lib
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

NQ, WINDOW = 70, 40


@pytest.mark.parametrize("d,vd", [(64, 64), (96, 40)])
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_window_prefill_wrappers(monkeypatch, diag_lib, form, fp8, d, vd):  # noqa: F811
    bkv = sl.SEQS * sl.HK
    sl._check_caps(sl.DECODE_CAPS, bkv)
    plan = (ctypes.c_int32 * 8)()
    prob = _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, bkv * sl.G, (NQ,), (sl.PAGE * sl.MAX_PAGES,), d, vd)
    assert diag_lib.fa_forward_ragged_window_prefill_plan(prob, sl.G, WINDOW, plan) == _lib.FA_OK
    assert tuple(plan) == (1, 1024, WINDOW + 63, 1, 64, 128, 2, 0)
    args, scales, (Q, Kref, Vref, kv_lens) = sl._decode_case(form, fp8, d, vd, NQ, seed=1000 * d + 7)
    wrapper = fa.ragged_window_prefill_1d if form == "ragged" else fa.paged_window_prefill_1d

    def call():
        with torch.no_grad():
            out = wrapper(*args, WINDOW, returning_l_m=True, **scales)
        return tuple(t.reshape((-1,) + t.shape[2:]) for t in out)

    ref = sl._run(monkeypatch, diag_lib, None, bkv, call)
    res = gw._check_window(ref, Q, Kref, Vref, kv_lens, sl.G, WINDOW)
    print(f"{form} fp8={fp8} d={d} vd={vd}: worst error / allowance {res}")
    assert np.asarray(kv_lens).max() > WINDOW + NQ
    for cap in sl.DECODE_CAPS:
        assert -(-bkv // cap) > 1
        assert sl._same(sl._run(monkeypatch, diag_lib, cap, bkv, call), ref), cap
