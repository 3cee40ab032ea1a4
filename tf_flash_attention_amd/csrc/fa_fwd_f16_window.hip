// fa_fwd_f16_window.hip — the sliding-window form of the decode forwards over the four K/V caches of
// fa_fwd_f16_decode.h, and its merge (gfx950 MFMA; fa_fwd_f16_window.h says what the form is).  A paged cache's
// first table entry loaded is the first staged tile's and the look-ahead runs up from there to the last live page,
// so the entries of pages wholly below the window, like those past the length, are never loaded.  The scales of an
// FP8 cache go where they go without a window.
#include "fa_fwd_f16_decode.h"
#include "fa_fwd_f16_window.h"

namespace fa {
namespace {

using namespace f16core;

template <class Cache, int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_partial_kernel(WindowOf<typename Cache::Args> wa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = Cache::ragged(wa.a);
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int c, len, kt0, ntiles;
  if (!window_block(ra, wa.window, &bkv, &c, &len, &kt0, &ntiles)) return;  // the merge does not read its record
  const WindowRowsOf<typename Cache::Rows> map = {Cache::template rows<D, FAST>(wa.a, bkv, len, sa.f.rule.q.n, kt0), wa.window};
  CacheRegs<Cache, D> rg;
  WaveState<D> ws;
  fewq_partial<D, 1, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, c, kt0, ntiles, rg, ws);
}

// over the live launched chunks of the thread's K/V slice: relative chunk c is absolute chunk lo / chunk + c, and
// the last live one holds key len - 1; each of them wrote the records of all live rows
__global__ __launch_bounds__(256) void window_merge_kernel(WindowOf<RaggedArgs> wa) {
  const RaggedArgs& ra = wa.a;
  const SplitArgs& sa = ra.g.s;
  merge_folded(ra.g, [&](int64_t bkv) {
    const int len = slice_len(ra, (uint32_t)bkv);
    if (len < 1) return 0;
    const int lo = window_lo(len, sa.f.rule.q.n, wa.window);
    return min(sa.nchunks, (len - 1) / sa.chunk - lo / sa.chunk + 1);
  });
}

}  // namespace

template <class Args>
hipError_t launch_fwd_f16_window(const WindowOf<Args>& wa, hipStream_t s) {
  using Cache = CacheOf<Args>;
  const RaggedArgs& ra = Cache::ragged(wa.a);
  const SplitArgs& sa = ra.g.s;
  const hipError_t e = with_fewq_window(sa.f, Cache::row_keys(wa.a), [&](auto d, auto fast) {
    return launch_fewq_partial(d, window_partial_kernel<Cache, d.value, fast.value != 0>, wa, sa, s);
  }, Cache::kChunkBytes);
  if (e != hipSuccess) return e;
  // (the merge reads neither K / V nor a table nor the scales: v_scale is already in the records)
  return launch_fewq_merge(window_merge_kernel, WindowOf<RaggedArgs>{ra, wa.window}, sa.f, ra.g.g, s);
}
template hipError_t launch_fwd_f16_window(const WindowOf<RaggedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_window(const WindowOf<PagedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_window(const WindowOf<RaggedFp8Args>&, hipStream_t);
template hipError_t launch_fwd_f16_window(const WindowOf<PagedFp8Args>&, hipStream_t);

}  // namespace fa
