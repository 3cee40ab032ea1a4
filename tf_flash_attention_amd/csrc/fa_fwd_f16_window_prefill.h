// fa_fwd_f16_window_prefill.h — the sliding-window form over query blocks of the ragged and paged few-query
// forwards: what its kernel template over the four caches (fa_fwd_f16_window_prefill.hip; the caches:
// fa_fwd_f16_decode.h) is made of.
//
// It is the product of the windowed form (fa_fwd_f16_window.h) and the query-blocked form (fa_fwd_f16_prefill.h),
// and nothing else: no key loop, no mask and no fold of its own.
//   * the nq queries are cut into nqb blocks of P = GqaArgs::pitch queries as in the query-blocked form.  Block qb
//     holds the queries [q0, q0 + nq_b) and, under the tail rule (implied, as in every windowed form), sees the keys
//     below L_b = block_len(len, q0): it is the windowed twin's problem with (len, nq) = (L_b, nq_b).  So its
//     queries see [lo_b, L_b) as a whole, lo_b = window_lo(L_b, nq_b, W): at most W + nq_b - 1 keys.
//   * one workgroup per (K/V slice, query block, relative chunk), chunks fastest.  It loads and clamps its slice's
//     length, forms L_b and lo_b, and works ABSOLUTE chunk lo_b / chunk + c: the tiles from max(chunk start, lo_b
//     rounded down to the 64-key tile) to min(chunk end, L_b).  An empty range (a block of queries before position 0
//     among them) returns before any other load.  The plan (fa_api.hip) launches as many relative chunks per block
//     as an interval of W + P - 1 keys can touch.
//   * the map is BlockRowsOf<WindowRowsOf<Cache::Rows>> with those two numbers, q0 and W.  Under kQBlock the core
//     counts its queries by map.nq = nq_b and hands lane_interval a block-relative query, so WindowRowsOf's
//     khi = L_b - nq_b + qi and klo = max(khi - W + 1, 0) are the query's interval, and both ends stay
//     non-decreasing in the query.
//   * the record is filed under slice * nqb + qb at relative chunk c.  The merge, one thread per (slice, channel,
//     head, query), finds its block as prefill_merge does and folds the block's live launched chunks
//     (L_b - 1) / chunk - lo_b / chunk + 1 in order; none: the empty row.
// A paged cache's first table entry loaded is the first staged tile's and its look-ahead stops at page
// (L_b - 1) / page, so entries of pages wholly below lo_b or past L_b are never loaded.  Keys of the first staged
// tile below a query's klo are loaded and masked, never zeroed: they must be finite.  Only POL 1 is instantiated.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_PREFILL_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_PREFILL_H_

#include "fa_fwd_f16_prefill.h"
#include "fa_fwd_f16_window.h"

namespace fa {
namespace f16core {

// a windowed map over one query block; Base: RaggedRows, PagedRows or their 8-bit forms, with len = L_b, nq = nq_b
template <class Base>
using WindowBlockRowsOf = BlockRowsOf<WindowRowsOf<Base>>;

// the live launched chunks of a block that sees the keys [lo_b, lb): relative chunk c is absolute chunk
// lo_b / chunk + c, and the last live one holds key lb - 1
__device__ __forceinline__ int window_block_chunks(const SplitArgs& sa, int lb, int nq_b, int win) {
  if (lb < 1) return 0;
  const int lo = window_lo(lb, nq_b, win);
  return min(sa.nchunks, (int)((uint32_t)(lb - 1) / (uint32_t)sa.chunk) - (int)((uint32_t)lo / (uint32_t)sa.chunk) + 1);
}

// What workgroup blockIdx.x of a windowed query-blocked partial kernel works: K/V slice *bkv, query block *qb at
// *q0, record (relative chunk) *c, the block's key end *lb, and the tiles [*kt0, *kt0 + 64 * *ntiles) of absolute
// chunk lo_b / chunk + c.  False: nothing (no record is read).
__device__ __forceinline__ bool window_prefill_block(const RaggedArgs& ra, int nqb, int win, uint32_t* bkv, int* qb, int* q0,
                                                     int* c, int* lb, int* kt0, int* ntiles) {
  const SplitArgs& sa = ra.g.s;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x), t = bid / (uint32_t)sa.nchunks;
  *c = (int)(bid - t * (uint32_t)sa.nchunks);
  *bkv = t / (uint32_t)nqb;
  *qb = (int)(t - *bkv * (uint32_t)nqb);
  *q0 = *qb << ra.g.log2_pitch;
  *lb = block_len(ra.g, true, __builtin_amdgcn_readfirstlane(slice_len(ra, *bkv)), *q0);
  const int lo = window_lo(*lb, block_queries(ra.g, *q0), win);
  const int cs = ((int)((uint32_t)lo / (uint32_t)sa.chunk) + *c) * sa.chunk;  // the chunk's first key
  *kt0 = max(cs, lo & ~(kBN - 1));
  const int end = min(cs + sa.chunk, *lb);
  *ntiles = (end - *kt0 + kBN - 1) / kBN;
  return *kt0 < end;
}

// the merge thread: query q of head j is row j * P + q % P of block q / P, over that block's live launched chunks
__device__ __forceinline__ void window_prefill_merge(const RaggedArgs& ra, int nqb, int win) {
  const GqaArgs& ga = ra.g;
  const SplitArgs& sa = ga.s;
  int64_t bkv;
  int v, j, q;
  if (!merge_thread(sa.f, ga.g, &bkv, &v, &j, &q)) return;
  const int qb = q >> ga.log2_pitch, q0 = qb << ga.log2_pitch;
  const int lb = block_len(ga, true, slice_len(ra, (uint32_t)bkv), q0);
  merge_row(sa, ga.g * ga.pitch, bkv * nqb + qb, j * ga.pitch + (q - q0), v,
            window_block_chunks(sa, lb, block_queries(ga, q0), win), bkv * ga.g + j, q);
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_WINDOW_PREFILL_H_
