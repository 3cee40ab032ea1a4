// fa_fwd_f16_prefill.hip — the query-blocked form of the decode forwards over the four K/V caches of
// fa_fwd_f16_decode.h, for any number of queries, and its merge (gfx950 MFMA; fa_fwd_f16_prefill.h says what the
// form is).  A cache builds its map for the block's lb keys and nq_b queries: a paged cache's first table entry
// loaded is the first staged tile's, and its look-ahead stops at page (lb - 1) / page.
#include "fa_fwd_f16_decode.h"
#include "fa_fwd_f16_prefill.h"

namespace fa {
namespace {

using namespace f16core;

template <class Cache, int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void prefill_partial_kernel(PrefillOf<typename Cache::Args> pf) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = Cache::ragged(pf.a);
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int qb, q0, ch, lb, kt0, ntiles;
  if (!prefill_block(ra, pf.nqb, POL == 1, &bkv, &qb, &q0, &ch, &lb, &kt0, &ntiles)) return;  // the merge does not read its record
  const BlockRowsOf<typename Cache::Rows> map = {Cache::template rows<D, FAST>(pf.a, bkv, lb, block_queries(ra.g, q0), kt0), q0};
  CacheRegs<Cache, D> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws, (int64_t)bkv * pf.nqb + qb);
}

__global__ __launch_bounds__(256) void prefill_merge_kernel(PrefillOf<RaggedArgs> pf) { prefill_merge(pf.a, pf.nqb); }

}  // namespace

template <class Args>
hipError_t launch_fwd_f16_prefill(const PrefillOf<Args>& pf, hipStream_t s) {
  using Cache = CacheOf<Args>;
  const RaggedArgs& ra = Cache::ragged(pf.a);
  const hipError_t e = with_fewq_tail(ra, Cache::row_keys(pf.a), [&](auto d, auto pol, auto fast) {
    return launch_prefill_partial(d, prefill_partial_kernel<Cache, d.value, pol.value, fast.value != 0>, pf, ra.g.s, pf.nqb, s);
  }, Cache::kChunkBytes);
  if (e != hipSuccess) return e;
  // (the merge reads neither K / V nor a table nor the scales: v_scale is already in the records)
  return launch_fewq_merge(prefill_merge_kernel, PrefillOf<RaggedArgs>{ra, pf.nqb}, ra.g.s.f, ra.g.g, s);
}
template hipError_t launch_fwd_f16_prefill(const PrefillOf<RaggedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_prefill(const PrefillOf<PagedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_prefill(const PrefillOf<RaggedFp8Args>&, hipStream_t);
template hipError_t launch_fwd_f16_prefill(const PrefillOf<PagedFp8Args>&, hipStream_t);

}  // namespace fa
