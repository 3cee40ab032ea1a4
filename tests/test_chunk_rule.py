"""CPU test of the one chunk rule behind every split plan: through each of the eight plans' exports,

    chunk = max(min_chunk, ceil(span / (kmax * granule)) * granule)

with the plan's own span, kmax (64, or max(1, 64 / blocks)), minimum (512 or 1024) and granule (64 keys; 128 queries
for the backward's query split).  The spans sit one below, at and one above kmax * granule * j: j = 1, 2 (the cap's
first steps) and the j at which the cap passes each minimum.  Host-only arithmetic, no device."""

import ctypes

import pytest

from tf_flash_attention_amd import _lib

BIG = 1 << 22  # a capacity no window here reaches


def _chunk(fn, p, *own):
    out = (ctypes.c_int32 * 8)()
    assert getattr(_lib.lib(), fn)(p, *own, out) == _lib.FA_OK, _lib.last_error()
    assert out[0] >= 1, "outside the plan's envelope"
    return out[1]


def _prob(nq, nk, b=1, d=64, vd=64):
    return _lib.make_problem(_lib.F16, _lib.FULL, 1, _lib.NONE_FRONT, b, (nq,), (nk,), d, vd)


# (id, kmax, min_chunk, granule, span -> the export's chunk).  The blocked forms' kmax of 3 and 1 are 17 and 33 blocks.
CASES = [
    ("split-512", 64, 512, 64, lambda s: _chunk("fa_forward_split_plan", _prob(64, s))),
    ("split-1024", 64, 1024, 64, lambda s: _chunk("fa_forward_split_plan", _prob(65, s))),
    ("grouped-512", 64, 512, 64, lambda s: _chunk("fa_forward_grouped_plan", _prob(1, s, 64), 64)),
    ("grouped-1024", 64, 1024, 64, lambda s: _chunk("fa_forward_grouped_plan", _prob(1, s, 65), 65)),
    ("window-512", 64, 512, 64, lambda s: _chunk("fa_forward_ragged_window_plan", _prob(1, BIG), 1, s)),
    ("window-1024", 64, 1024, 64, lambda s: _chunk("fa_forward_ragged_window_plan", _prob(1, BIG, 128), 128, s)),
    ("prefill-one-block-512", 64, 512, 64, lambda s: _chunk("fa_forward_ragged_prefill_plan", _prob(64, s), 1)),
    ("prefill-one-block-1024", 64, 1024, 64, lambda s: _chunk("fa_forward_ragged_prefill_plan", _prob(128, s), 1)),
    ("prefill-17-blocks", 3, 1024, 64, lambda s: _chunk("fa_forward_ragged_prefill_plan", _prob(17 * 128, s), 1)),
    ("prefill-33-blocks", 1, 1024, 64, lambda s: _chunk("fa_forward_ragged_prefill_plan", _prob(33 * 128, s), 1)),
    ("window-prefill-one-block-512", 64, 512, 64, lambda s: _chunk("fa_forward_ragged_window_prefill_plan", _prob(1, BIG), 1, s)),
    ("window-prefill-one-block-1024", 64, 1024, 64,
     lambda s: _chunk("fa_forward_ragged_window_prefill_plan", _prob(1, BIG, 128), 128, s)),
    ("window-prefill-17-blocks", 3, 1024, 64, lambda s: _chunk("fa_forward_ragged_window_prefill_plan", _prob(17, BIG, 128), 128, s)),
    ("window-prefill-33-blocks", 1, 1024, 64, lambda s: _chunk("fa_forward_ragged_window_prefill_plan", _prob(33, BIG, 128), 128, s)),
    ("backward-query-split-512", 64, 512, 128, lambda s: _chunk("fa_backward_split_q_plan", _prob(s, 64))),
    ("backward-query-split-1024", 64, 1024, 128, lambda s: _chunk("fa_backward_split_q_plan", _prob(s, 65))),
    ("mla-512", 64, 512, 64, lambda s: _chunk("fa_forward_mla_paged_plan", _prob(1, s, 1, 576, 512), 1, 64)),
    ("mla-1024", 64, 1024, 64, lambda s: _chunk("fa_forward_mla_paged_plan", _prob(1, s, 128, 576, 512), 128, 64)),
    ("mla-blocked-one-block", 64, 512, 64, lambda s: _chunk("fa_forward_mla_paged_prefill_plan", _prob(4, s, 16, 576, 512), 16, 64)),
    ("mla-blocked-17-blocks", 3, 1024, 64, lambda s: _chunk("fa_forward_mla_paged_prefill_plan", _prob(68, s, 16, 576, 512), 16, 64)),
    ("mla-blocked-33-blocks", 1, 1024, 64, lambda s: _chunk("fa_forward_mla_paged_prefill_plan", _prob(132, s, 16, 576, 512), 16, 64)),
]


@pytest.mark.parametrize("name,kmax,min_chunk,granule,chunk_of", CASES, ids=[c[0] for c in CASES])
def test_every_plan_cuts_by_the_one_closed_form(name, kmax, min_chunk, granule, chunk_of):
    # an MLA capacity is whole pages of 64 keys, so its spans step by a page; the split plans need a range of 2048
    step = 64 if name.startswith("mla") else 1
    least = 2048 if name.startswith(("split", "backward")) else 1
    cover = kmax * granule
    at_min = min_chunk // granule  # the cap is the minimum at cover * at_min and one granule more just above it
    seen = set()
    for j in (1, 2, at_min, at_min + 1):
        for span in (cover * j - step, cover * j, cover * j + step):
            if span < least:
                continue
            want = max(min_chunk, -(-span // cover) * granule)
            assert chunk_of(span) == want, (span, want)
            seen.add(want > min_chunk)
    assert seen == {False, True}  # both the minimum and the cap decided
