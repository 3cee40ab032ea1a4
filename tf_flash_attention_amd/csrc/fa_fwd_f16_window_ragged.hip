// fa_fwd_f16_window_ragged.hip — the ragged few-query fp16 forward (fa_fwd_f16_ragged.hip) under a sliding
// window, and the merge of all four windowed forwards (gfx950 MFMA; fa_fwd_f16_window.h says what they share).
#include "fa_fwd_f16_window.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_ragged_partial_kernel(WindowOf<RaggedArgs> wa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = wa.a;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int c, len, kt0, ntiles;
  if (!window_block(ra, wa.window, &bkv, &c, &len, &kt0, &ntiles)) return;  // the merge does not read its record
  const WindowRows map = {{folded_rows(ra.g), len, sa.f.rule.q.n}, wa.window};
  WaveRegs<D, kFewqNW> rg;
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

hipError_t launch_fwd_f16_window_merge(const WindowOf<RaggedArgs>& wa, hipStream_t s) {
  return launch_fewq_merge(window_merge_kernel, wa, wa.a.g.s.f, wa.a.g.g, s);
}

hipError_t launch_fwd_f16_window_ragged(const WindowOf<RaggedArgs>& wa, hipStream_t s) {
  const SplitArgs& sa = wa.a.g.s;
  const hipError_t e = with_fewq_window(sa.f, sa.f.rule.k.n, [&](auto d, auto fast) {
    return launch_fewq_partial(d, window_ragged_partial_kernel<d.value, fast.value != 0>, wa, sa, s);
  });
  if (e != hipSuccess) return e;
  return launch_fwd_f16_window_merge(wa, s);
}

}  // namespace fa
