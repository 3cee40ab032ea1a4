"""GPU tests of the fused append into the MLA latent pool (mla_paged_append_1d): the WHOLE pool
afterwards, viewed as [num_pages, 1, C, page], is tests/append_ref.paged_one's, byte for byte."""

import numpy as np
import pytest
import torch

from tests import append_ref, fp8_ref
from tests import test_gpu_mla as mla
from tests import test_gpu_mla_fp8 as mla8
from tests import test_gpu_ragged as rg
from tf_flash_attention_amd import flash_attention as fa

pytestmark = pytest.mark.gpu

C, SCALE = 576, np.float32(0.005)  # (the scale saturates some of the new values at +-448)


def _append(fp8, n_new, page, with_new_lens, seed):
    """Five sequences whose lengths after the append are 0, Nnew - 1, a page edge, just past it and the capacity;
    returns (Q, table, lens, the appended device pool, the reference pool)."""
    Q, K8, table, pool8 = mla8._case8(5, 16, C, 1, page, seed)
    pool = pool8 if fp8 else pool8.astype(np.float16)
    lens = [0, n_new - 1, page, page + 3, K8.shape[2]]
    new_lens = [3, 5, 0, n_new, 1] if with_new_lens else None
    new = np.random.default_rng(seed + 5).uniform(-3, 3, (5, C, n_new)).astype(np.float16)
    tp = mla._t(pool)
    fa.mla_paged_append_1d(tp, mla._t(new), mla._t(table, torch.int32), mla._t(lens, torch.int32),
                           None if new_lens is None else mla._t(new_lens, torch.int32),
                           mla._t([SCALE], torch.float32) if fp8 else None)
    torch.cuda.synchronize()
    ref = append_ref.paged_one(pool[:, None], new[:, None], table, lens, new_lens, [SCALE] if fp8 else None)[:, 0]
    return Q, table, lens, tp, ref


@pytest.mark.parametrize("with_new_lens", [False, True], ids=["all_new", "new_lens"])
@pytest.mark.parametrize("page", [64, 192])
@pytest.mark.parametrize("n_new", [1, 9, 130])
@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
def test_the_whole_pool_is_the_reference(fp8, n_new, page, with_new_lens):
    _, _, _, tp, ref = _append(fp8, n_new, page, with_new_lens, seed=100 * n_new + page + fp8)
    assert np.array_equal(tp.cpu().numpy().view(np.uint8), ref.view(np.uint8))


def test_the_forward_reads_the_appended_fp8_pool():
    v, page = 512, 64
    Q, table, lens, tp, ref = _append(True, 9, page, False, seed=31)
    got = fa.mla_paged_1d(mla._t(Q).reshape(5, 16, C, 1), tp, mla._t(table, torch.int32), mla._t(lens, torch.int32), v,
                          returning_l_m=True, kv_scale=mla._t([SCALE], torch.float32))
    torch.cuda.synchronize()
    Kd = fp8_ref.decode(ref[table]).transpose(0, 2, 1, 3).reshape(5, C, -1) * float(SCALE)  # the gathered cache
    rg._check_ref(tuple(t.reshape((-1,) + t.shape[2:]) for t in got), Q, Kd, Kd[:, :v, :], lens, 16, False)
