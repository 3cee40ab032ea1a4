// fa_fwd_f16_window_ragged_fp8.hip — the ragged few-query forward over an FP8 K/V cache
// (fa_fwd_f16_ragged_fp8.hip) under a sliding window (gfx950 MFMA; fa_fwd_f16_window.h says what the windowed
// forwards share).  The scales go where they go without a window: kv8_mul (fa_fwd_f16_fewq.h).
#include "fa_fwd_f16_window.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void window_ragged_fp8_partial_kernel(WindowOf<RaggedFp8Args> wa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = wa.a.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int c, len, kt0, ntiles;
  if (!window_block(ra, wa.window, &bkv, &c, &len, &kt0, &ntiles)) return;  // the merge does not read its record
  const Kv8Mul sc = kv8_mul(wa.a.k_scale, wa.a.v_scale, (int)(((uint32_t)ra.rem0 + bkv) % (uint32_t)ra.kv_per_len));
  const WindowRows8 map = {{{folded_rows(ra.g), len, sa.f.rule.q.n}, sc.kmul, sc.qmul, sc.vmul}, wa.window};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, 1, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, c, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_window_ragged_fp8(const WindowOf<RaggedFp8Args>& wa, hipStream_t s) {
  const SplitArgs& sa = wa.a.r.g.s;
  const hipError_t e = with_fewq_window(sa.f, sa.f.rule.k.n, [&](auto d, auto fast) {
    return launch_fewq_partial(d, window_ragged_fp8_partial_kernel<d.value, fast.value != 0>, wa, sa, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_window_merge({wa.a.r, wa.window}, s);  // v_scale is already in the records
}

}  // namespace fa
