// fa_fwd_f16_gqa.hip — grouped-query fp16 forward for few queries (gfx950 MFMA).
//
// In grouped-query attention g query slices (heads) share one K/V slice: Q slice bi attends K/V slice
// bi / g.  On expanded K/V the split-key forward (fa_fwd_f16_splitk.hip) would stream every shared key g
// times, each time with nq live columns in a wave's 32.  Here the g heads of a group are folded into the
// 128 query rows of ONE workgroup (FoldedRows, fa_fwd_f16_core.h): row rho = head rho / pitch, query
// rho % pitch, pitch the smallest power of two >= nq, g * pitch <= 128.  K and V stream once per group and
// the MFMA columns fill up.  The key range of the query block [0, nq-1] is cut into chunks
// (fa_api.hip: grouped_plan), also for a short range (one chunk, and an empty range is one chunk without
// tiles), so there is one path: the partial + merge pair of fa_fwd_f16_fewq.h, one workgroup per (K/V slice,
// chunk), a record row of g * pitch floats, and a merge that writes O, l, m of query slice bkv * g + j.
// A query slice's bits are not those of the ungrouped forward on expanded K/V: the core's lazy rebase is
// taken per wave, so a row's arithmetic depends on which rows share its wave.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void gqa_partial_kernel(GqaArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SplitArgs& sa = ga.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, sa.k_first, &bkv, &ch, &kt0);
  const int ntiles = chunk_tiles(sa, kt0, sa.k_end, true);  // (an empty range: one chunk without tiles)
  WaveRegs<D, kFewqNW> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, folded_rows(ga), bkv, ch, kt0, ntiles, rg, ws);
}

__global__ __launch_bounds__(256) void gqa_merge_kernel(GqaArgs ga) {
  merge_folded(ga, [&](int64_t) { return ga.s.nchunks; });
}

}  // namespace

hipError_t launch_fwd_f16_gqa(const GqaArgs& ga, hipStream_t s) {
  const hipError_t e = with_fewq_rule(ga.s.f, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, gqa_partial_kernel<d.value, pol.value, fast.value != 0>, ga, ga.s, s);
  });
  if (e != hipSuccess) return e;
  return launch_fewq_merge(gqa_merge_kernel, ga, ga.s.f, ga.g, s);
}

}  // namespace fa
