// fa_fwd_f16_window_paged_fp8.hip — the paged few-query forward over FP8 page pools (fa_fwd_f16_paged_fp8.hip)
// under a sliding window (gfx950 MFMA; fa_fwd_f16_window.h says what the windowed forwards share).
#include "fa_fwd_f16_window.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_paged_fp8_partial_kernel(WindowOf<PagedFp8Args> wa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PagedArgs& pa = wa.a.p;
  const SplitArgs& sa = pa.r.g.s;
  uint32_t bkv;
  int c, len, kt0, ntiles;
  if (!window_block(pa.r, wa.window, &bkv, &c, &len, &kt0, &ntiles)) return;  // the merge does not read its record
  const PagedRows rows = paged_rows<D, FAST>(pa, bkv, len, kt0);
  const Kv8Mul sc = kv8_mul(wa.a.k_scale, wa.a.v_scale, rows.hk);
  const WindowPagedRows8 map = {{rows, sc.kmul, sc.qmul, sc.vmul}, wa.window};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, 1, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, c, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_window_paged_fp8(const WindowOf<PagedFp8Args>& wa, hipStream_t s) {
  const SplitArgs& sa = wa.a.p.r.g.s;
  const hipError_t e = with_fewq_window(sa.f, wa.a.p.page, [&](auto d, auto fast) {
    return launch_fewq_partial(d, window_paged_fp8_partial_kernel<d.value, fast.value != 0>, wa, sa, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_window_merge({wa.a.p.r, wa.window}, s);  // the merge reads neither K / V nor the table nor the scales
}

}  // namespace fa
