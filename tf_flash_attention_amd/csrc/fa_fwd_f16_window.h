// fa_fwd_f16_window.h — the sliding-window form of the ragged and paged few-query forwards: what its kernel
// template over the four caches (fa_fwd_f16_window.hip; the caches: fa_fwd_f16_decode.h) is made of.
//
// The nq queries are the last nq positions of a sequence of len live keys (the tail rule): query i sits at
// position len - nq + i and sees the W keys [max(0, pos - W + 1), pos].  The block as a whole sees [lo, len),
// lo = max(0, len - nq - W + 1): at most W + nq - 1 keys, wherever they lie in the capacity.  So the plan
// (fa_api.hip) launches, per K/V slice, only the n_launch chunks that such an interval can touch, and the chunk
// boundaries stay at absolute multiples of `chunk` from key 0:
//   * workgroup (slice, c) loads its slice's length, forms lo, and works ABSOLUTE chunk lo / chunk + c: the tiles
//     from max(chunk start, lo rounded down to the 64-key tile) to min(chunk end, len).  An empty range returns
//     before any other load.  Tiles wholly below the window are never staged, and a paged map never loads the
//     table entry of a page wholly below it: paged_rows' first entry is the first staged tile's, and
//     PagedRows::tile looks ahead from there.
//   * the map is the un-windowed one with lane_interval's lower end moved: klo = max(0, khi - W + 1).  Both ends
//     stay non-decreasing in the query, which the core's wave bounds rest on (lanes 0 / last of a wave hold its
//     first / last query at every pitch of the fold: fa_fwd_f16_core.h).  The core is untouched: POL 1's tile
//     class skips a wave's tiles below its klo, and the one-compare mask cuts the keys of the first staged tile
//     that lie below a query's klo.  Those keys are loaded and masked, never zeroed, so they must be finite.
//   * the merge is merge_folded over the slice's live launched chunks (len - 1) / chunk - lo / chunk + 1, in
//     order; record c of a slice is relative chunk c.
// Only POL 1 is instantiated: one query with a window needs the interval form too.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_H_

#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace f16core {

// the first key any query of a block of nq tail queries sees under window `win` (len clamped, 1 <= win < nk)
__device__ __forceinline__ int window_lo(int len, int nq, int win) { return max(len - nq - win + 1, 0); }

// a map with the window's lower end; Base: RaggedRows, PagedRows or their 8-bit forms
template <class Base>
struct WindowRowsOf : Base {
  int32_t win;
  __device__ __forceinline__ void lane_interval(const Rule&, int qi, int* klo, int* khi) const {
    *khi = this->len - this->nq + qi;
    *klo = max(*khi - win + 1, 0);
  }
};
using WindowRows = WindowRowsOf<RaggedRows>;
using WindowPagedRows = WindowRowsOf<PagedRows>;
using WindowRows8 = WindowRowsOf<RaggedRows8>;
using WindowPagedRows8 = WindowRowsOf<PagedRows8>;

// What workgroup blockIdx.x of a windowed partial kernel works: K/V slice *bkv, its length *len, record *c, and
// the tiles [*kt0, *kt0 + 64 * *ntiles) of absolute chunk lo / chunk + c.  False: nothing (no record is read).
__device__ __forceinline__ bool window_block(const RaggedArgs& ra, int win, uint32_t* bkv, int* c, int* len, int* kt0,
                                             int* ntiles) {
  const SplitArgs& sa = ra.g.s;
  int rel;
  fewq_block(sa, 0, bkv, c, &rel);
  *len = __builtin_amdgcn_readfirstlane(slice_len(ra, *bkv));
  const int lo = window_lo(*len, sa.f.rule.q.n, win);
  const int cs = (int)((uint32_t)lo / (uint32_t)sa.chunk) * sa.chunk + rel;  // the chunk's first key
  *kt0 = max(cs, lo & ~(kBN - 1));
  const int end = min(cs + sa.chunk, *len);
  *ntiles = (end - *kt0 + kBN - 1) / kBN;
  return *kt0 < end;
}

// host: the <D, FAST> instantiation of a windowed forward (with_fewq_tail's, POL 1 always)
template <class Launch>
hipError_t with_fewq_window(const FwdArgs& a, int row_keys, Launch&& launch, int chunk_bytes = 16) {
  return with_fewq_d(a, [&](auto d) {
    return fast_staging<decltype(d)::value>(a, row_keys, chunk_bytes) ? launch(d, IC<1>{}) : launch(d, IC<0>{});
  });
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_H_
