"""GPU test of the batch-slab launch loop (fewq_slabs, csrc/fa_api.hip) behind the sliding-window
decode entry points, in the manner of tests/test_gpu_slabs.py and with its inputs: the diagnostic library lowers the
slab limit to FA_SLAB_MAX K/V slices and counts the slab launches.  The capped call is bitwise the uncapped one, the
uncapped one passes the window's gate (tests/test_gpu_window._check_window), and the counter rose by
ceil(slices / cap).  The window (40 keys over a capacity of 256) makes the plan the window's, not the delegated
twin's; every cap but 1 makes a slab straddle two sequences, so len0 and rem0 pick the length that lo is formed
from, the table row and the head's scales."""

import numpy as np
import pytest
import torch

from tests import test_gpu_slabs as sl
from tests import test_gpu_window as gw
from tests.test_gpu_parity import diag_lib  # noqa: F401  (a fixture)
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

WINDOW = 40


@pytest.mark.parametrize("d,vd,nq", [(64, 64, 1), (64, 64, 4), (96, 40, 4)])
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("form", ["ragged", "paged"])
def test_windowed_decode_wrappers(monkeypatch, diag_lib, form, fp8, d, vd, nq):  # noqa: F811
    bkv = sl.SEQS * sl.HK
    sl._check_caps(sl.DECODE_CAPS, bkv)
    args, scales, (Q, Kref, Vref, kv_lens) = sl._decode_case(form, fp8, d, vd, nq, seed=1000 * d + 10 * nq)
    wrapper = fa.ragged_1d if form == "ragged" else fa.paged_1d

    def call():
        with torch.no_grad():
            out = wrapper(*args, tail_causal=True, returning_l_m=True, window_size=WINDOW, **scales)
        return tuple(t.reshape((-1,) + t.shape[2:]) for t in out)

    ref = sl._run(monkeypatch, diag_lib, None, bkv, call)
    res = gw._check_window(ref, Q, Kref, Vref, kv_lens, sl.G, WINDOW)
    print(f"{form} fp8={fp8} d={d} vd={vd} nq={nq}: worst error / allowance {res}")
    # and the window cut something: the un-windowed tail call differs
    with torch.no_grad():
        tail = wrapper(*args, tail_causal=True, returning_l_m=True, **scales)
    assert not sl._same(tuple(t.reshape((-1,) + t.shape[2:]) for t in tail), ref)
    for cap in sl.DECODE_CAPS:
        assert sl._same(sl._run(monkeypatch, diag_lib, cap, bkv, call), ref), cap
    assert np.asarray(kv_lens).max() > WINDOW + nq
