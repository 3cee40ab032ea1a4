// fa_fwd_f16_ragged_fp8.hip — the ragged few-query fp16 forward (fa_fwd_f16_ragged.hip) over an FP8 K/V cache
// (gfx950 MFMA).
//
// K [b/g][d][cap] and V [b/g][v_d][cap] are OCP e4m3fn bytes; Q, O, m stay fp16 and l fp32.  The true key is
// k_scale[h] * K8 and the true value v_scale[h] * V8, h = the slice's head among the kv_per_len heads of its
// sequence; the scales are device arrays that only the kernel reads (null: 1.0).  This is ragged_partial_kernel
// with RaggedRows8: the same dead-chunk return, length clamp, chunks and records, and ragged_merge_kernel itself as
// the merge.  The 8-bit cache is a staging concern of the core (fa_fwd_f16_core.h: KvOf): half the bytes loaded,
// converted exactly to the same fp16 LDS image; where the scales go: kv8_mul (fa_fwd_f16_fewq.h).  With both scales
// null or 1.0 the results are bitwise fa_forward_ragged's on the cache converted to fp16.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void ragged_fp8_partial_kernel(RaggedFp8Args fa8) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = fa8.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const Kv8Mul sc = kv8_mul(fa8.k_scale, fa8.v_scale, (int)(((uint32_t)ra.rem0 + bkv) % (uint32_t)ra.kv_per_len));
  const RaggedRows8 map = {{folded_rows(ra.g), len, sa.f.rule.q.n}, sc.kmul, sc.qmul, sc.vmul};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_ragged_fp8(const RaggedFp8Args& fa8, hipStream_t s) {
  // the capacity is the row stride in bytes: a multiple of 8 with 8-byte aligned K / V keeps every chunk aligned
  const hipError_t e = with_fewq_tail(fa8.r, fa8.r.g.s.f.rule.k.n, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, ragged_fp8_partial_kernel<d.value, pol.value, fast.value != 0>, fa8, fa8.r.g.s, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_ragged_merge(fa8.r, s);  // v_scale is already in the records
}

}  // namespace fa
