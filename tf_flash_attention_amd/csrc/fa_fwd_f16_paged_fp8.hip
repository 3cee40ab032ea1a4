// fa_fwd_f16_paged_fp8.hip — the paged few-query fp16 forward (fa_fwd_f16_paged.hip) over FP8 page pools
// (gfx950 MFMA).
//
// K_pool [num_pages][Hk][d][page] and V_pool [num_pages][Hk][v_d][page] are OCP e4m3fn bytes with the key axis
// contiguous; the block table, the lengths, Q, O, l and m are the fp16 forward's.  The true key is k_scale[hk] * K8
// and the true value v_scale[hk] * V8, device arrays of Hk floats that only the kernel reads (null: 1.0).  This is
// paged_partial_kernel with PagedRows8: the same dead-chunk return, length clamp, table look-ahead and clamp,
// chunks and records, and ragged_merge_kernel itself as the merge.  The 8-bit pools are a staging concern of the
// core (fa_fwd_f16_core.h: KvOf); where the scales go: kv8_mul (fa_fwd_f16_fewq.h).  With both scales null or 1.0
// the results are bitwise fa_forward_paged's on the pools converted to fp16.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void paged_fp8_partial_kernel(PagedFp8Args pa8) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PagedArgs& pa = pa8.p;
  const RaggedArgs& ra = pa.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const PagedRows rows = paged_rows<D, FAST>(pa, bkv, len, kt0);
  const Kv8Mul sc = kv8_mul(pa8.k_scale, pa8.v_scale, rows.hk);
  const PagedRows8 map = {rows, sc.kmul, sc.qmul, sc.vmul};
  WaveRegs<D, kFewqNW, u32x2> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_paged_fp8(const PagedFp8Args& pa8, hipStream_t s) {
  // a page is a multiple of 8 keys, so with 8-byte aligned pools every page row starts 8-byte aligned
  const hipError_t e = with_fewq_tail(pa8.p.r, pa8.p.page, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, paged_fp8_partial_kernel<d.value, pol.value, fast.value != 0>, pa8, pa8.p.r.g.s, s);
  }, 8);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_ragged_merge(pa8.p.r, s);  // the merge reads neither K / V nor the table nor the scales
}

}  // namespace fa
