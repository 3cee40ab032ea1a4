// fa_fwd_f16_prefill_paged_fp8.hip — the paged few-query forward over FP8 page pools (fa_fwd_f16_paged_fp8.hip)
// over any number of queries, in blocks (gfx950 MFMA; fa_fwd_f16_prefill.h says what the query-blocked forwards share).
#include "fa_fwd_f16_prefill.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void prefill_paged_fp8_partial_kernel(PrefillOf<PagedFp8Args> pf) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PagedArgs& pa = pf.a.p;
  const RaggedArgs& ra = pa.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int qb, q0, ch, lb, kt0, ntiles;
  if (!prefill_block(ra, pf.nqb, POL == 1, &bkv, &qb, &q0, &ch, &lb, &kt0, &ntiles)) return;  // the merge does not read its record
  PagedRows rows = paged_rows<D, FAST>(pa, bkv, lb, kt0);
  rows.nq = block_queries(ra.g, q0);
  const Kv8Mul sc = kv8_mul(pf.a.k_scale, pf.a.v_scale, rows.hk);
  const BlockPagedRows8 map = {{rows, sc.kmul, sc.qmul, sc.vmul}, q0};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws, (int64_t)bkv * pf.nqb + qb);
}

}  // namespace

hipError_t launch_fwd_f16_prefill_paged_fp8(const PrefillOf<PagedFp8Args>& pf, hipStream_t s) {
  const RaggedArgs& ra = pf.a.p.r;
  const hipError_t e = with_fewq_tail(ra, pf.a.p.page, [&](auto d, auto pol, auto fast) {
    return launch_prefill_partial(d, prefill_paged_fp8_partial_kernel<d.value, pol.value, fast.value != 0>, pf, ra.g.s, pf.nqb, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_prefill_merge({ra, pf.nqb}, s);
}

}  // namespace fa
