// fa_fwd_f16_window_prefill.hip — the sliding-window form over query blocks of the decode forwards over the four
// K/V caches of fa_fwd_f16_decode.h, and its merge (gfx950 MFMA; fa_fwd_f16_window_prefill.h says what the form
// is).  A cache builds its map for the block's lb keys and nq_b queries at the first staged tile: a paged cache's
// first table entry loaded is that tile's and its look-ahead stops at page (lb - 1) / page, so the entries of pages
// wholly below the block's window, like those past its newest key, are never loaded.
#include "fa_fwd_f16_decode.h"
#include "fa_fwd_f16_window_prefill.h"

namespace fa {
namespace {

using namespace f16core;

template <class Cache, int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_prefill_partial_kernel(
    WindowPrefillOf<typename Cache::Args> wp) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = Cache::ragged(wp.a);
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int qb, q0, c, lb, kt0, ntiles;
  if (!window_prefill_block(ra, wp.nqb, wp.window, &bkv, &qb, &q0, &c, &lb, &kt0, &ntiles)) return;  // the merge does not read its record
  const WindowBlockRowsOf<typename Cache::Rows> map = {
      {Cache::template rows<D, FAST>(wp.a, bkv, lb, block_queries(ra.g, q0), kt0), wp.window}, q0};
  CacheRegs<Cache, D> rg;
  WaveState<D> ws;
  fewq_partial<D, 1, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, c, kt0, ntiles, rg, ws, (int64_t)bkv * wp.nqb + qb);
}

__global__ __launch_bounds__(256) void window_prefill_merge_kernel(WindowPrefillOf<RaggedArgs> wp) {
  window_prefill_merge(wp.a, wp.nqb, wp.window);
}

}  // namespace

template <class Args>
hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<Args>& wp, hipStream_t s) {
  using Cache = CacheOf<Args>;
  const RaggedArgs& ra = Cache::ragged(wp.a);
  const SplitArgs& sa = ra.g.s;
  const hipError_t e = with_fewq_window(sa.f, Cache::row_keys(wp.a), [&](auto d, auto fast) {
    return launch_prefill_partial(d, window_prefill_partial_kernel<Cache, d.value, fast.value != 0>, wp, sa, wp.nqb, s);
  }, Cache::kChunkBytes);
  if (e != hipSuccess) return e;
  // (the merge reads neither K / V nor a table nor the scales: v_scale is already in the records)
  return launch_fewq_merge(window_prefill_merge_kernel, WindowPrefillOf<RaggedArgs>{ra, wp.window, wp.nqb}, sa.f, ra.g.g, s);
}
template hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<RaggedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<PagedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<RaggedFp8Args>&, hipStream_t);
template hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<PagedFp8Args>&, hipStream_t);

}  // namespace fa
