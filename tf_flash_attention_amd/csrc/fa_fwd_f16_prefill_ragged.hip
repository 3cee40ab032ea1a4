// fa_fwd_f16_prefill_ragged.hip — the ragged few-query fp16 forward (fa_fwd_f16_ragged.hip) over any number of
// queries, in blocks, and the merge of all four query-blocked forwards (gfx950 MFMA; fa_fwd_f16_prefill.h says
// what they share).
#include "fa_fwd_f16_prefill.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void prefill_ragged_partial_kernel(PrefillOf<RaggedArgs> pf) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = pf.a;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int qb, q0, ch, lb, kt0, ntiles;
  if (!prefill_block(ra, pf.nqb, POL == 1, &bkv, &qb, &q0, &ch, &lb, &kt0, &ntiles)) return;  // the merge does not read its record
  const BlockRows map = {{folded_rows(ra.g), lb, block_queries(ra.g, q0)}, q0};
  WaveRegs<D, kFewqNW> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws, (int64_t)bkv * pf.nqb + qb);
}

__global__ __launch_bounds__(256) void prefill_merge_kernel(PrefillOf<RaggedArgs> pf) { prefill_merge(pf.a, pf.nqb); }

}  // namespace

hipError_t launch_fwd_f16_prefill_merge(const PrefillOf<RaggedArgs>& pf, hipStream_t s) {
  return launch_fewq_merge(prefill_merge_kernel, pf, pf.a.g.s.f, pf.a.g.g, s);
}

hipError_t launch_fwd_f16_prefill_ragged(const PrefillOf<RaggedArgs>& pf, hipStream_t s) {
  const SplitArgs& sa = pf.a.g.s;
  const hipError_t e = with_fewq_tail(pf.a, sa.f.rule.k.n, [&](auto d, auto pol, auto fast) {
    return launch_prefill_partial(d, prefill_ragged_partial_kernel<d.value, pol.value, fast.value != 0>, pf, sa, pf.nqb, s);
  });
  if (e != hipSuccess) return e;
  return launch_fwd_f16_prefill_merge(pf, s);
}

}  // namespace fa
