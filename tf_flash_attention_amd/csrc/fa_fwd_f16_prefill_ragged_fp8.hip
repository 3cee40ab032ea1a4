// fa_fwd_f16_prefill_ragged_fp8.hip — the ragged few-query forward over an FP8 K/V cache (fa_fwd_f16_ragged_fp8.hip)
// over any number of queries, in blocks (gfx950 MFMA; fa_fwd_f16_prefill.h says what the query-blocked forwards share).
#include "fa_fwd_f16_prefill.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void prefill_ragged_fp8_partial_kernel(PrefillOf<RaggedFp8Args> pf) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = pf.a.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int qb, q0, ch, lb, kt0, ntiles;
  if (!prefill_block(ra, pf.nqb, POL == 1, &bkv, &qb, &q0, &ch, &lb, &kt0, &ntiles)) return;  // the merge does not read its record
  const Kv8Mul sc = kv8_mul(pf.a.k_scale, pf.a.v_scale, (int)(((uint32_t)ra.rem0 + bkv) % (uint32_t)ra.kv_per_len));
  const BlockRows8 map = {{{folded_rows(ra.g), lb, block_queries(ra.g, q0)}, sc.kmul, sc.qmul, sc.vmul}, q0};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws, (int64_t)bkv * pf.nqb + qb);
}

}  // namespace

hipError_t launch_fwd_f16_prefill_ragged_fp8(const PrefillOf<RaggedFp8Args>& pf, hipStream_t s) {
  const RaggedArgs& ra = pf.a.r;
  const hipError_t e = with_fewq_tail(ra, ra.g.s.f.rule.k.n, [&](auto d, auto pol, auto fast) {
    return launch_prefill_partial(d, prefill_ragged_fp8_partial_kernel<d.value, pol.value, fast.value != 0>, pf, ra.g.s, pf.nqb, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_prefill_merge({ra, pf.nqb}, s);  // v_scale is already in the records
}

}  // namespace fa
