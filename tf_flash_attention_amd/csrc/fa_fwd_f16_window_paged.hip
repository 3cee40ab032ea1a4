// fa_fwd_f16_window_paged.hip — the paged few-query fp16 forward (fa_fwd_f16_paged.hip) under a sliding window
// (gfx950 MFMA; fa_fwd_f16_window.h says what the windowed forwards share).  The first table entry loaded is the
// first staged tile's and the look-ahead runs up from there to the last live page, so the entries of pages wholly
// below the window, like those past the length, are never loaded.
#include "fa_fwd_f16_window.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_paged_partial_kernel(WindowOf<PagedArgs> wa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PagedArgs& pa = wa.a;
  const SplitArgs& sa = pa.r.g.s;
  uint32_t bkv;
  int c, len, kt0, ntiles;
  if (!window_block(pa.r, wa.window, &bkv, &c, &len, &kt0, &ntiles)) return;  // the merge does not read its record
  const WindowPagedRows map = {paged_rows<D, FAST>(pa, bkv, len, kt0), wa.window};
  WaveRegs<D, kFewqNW> rg;
  WaveState<D> ws;
  fewq_partial<D, 1, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, c, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_window_paged(const WindowOf<PagedArgs>& wa, hipStream_t s) {
  const SplitArgs& sa = wa.a.r.g.s;
  const hipError_t e = with_fewq_window(sa.f, wa.a.page, [&](auto d, auto fast) {
    return launch_fewq_partial(d, window_paged_partial_kernel<d.value, fast.value != 0>, wa, sa, s);
  });
  if (e != hipSuccess) return e;
  return launch_fwd_f16_window_merge({wa.a.r, wa.window}, s);  // the merge reads neither K / V nor the table
}

}  // namespace fa
