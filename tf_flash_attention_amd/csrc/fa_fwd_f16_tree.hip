// fa_fwd_f16_tree.hip — the tree-masked draft form of the decode forwards over the four K/V caches of
// fa_fwd_f16_decode.h (gfx950 MFMA; fa_fwd_f16_tree.h says what the form is).  The kernel is the plain form's
// (fa_fwd_f16_decode.hip) with the mask's row pointer and base = len - nq added to the cache's map; a paged cache
// loads the table entries the plain form loads, and the scales of an FP8 cache go where they go there.
#include "fa_fwd_f16_decode.h"
#include "fa_fwd_f16_tree.h"

namespace fa {
namespace {

using namespace f16core;

template <class Cache, int D, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void tree_partial_kernel(TreeOf<typename Cache::Args> ta) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = Cache::ragged(ta.a);
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const int nq = sa.f.rule.q.n, words = (nq + 31) >> 5;
  // ta.mask is this launch's first sequence's: the sequence is counted as slice_len counts it
  const uint32_t seq = ((uint32_t)ra.rem0 + bkv) / (uint32_t)ra.kv_per_len;
  const TreeRowsOf<typename Cache::Rows> map = {Cache::template rows<D, FAST>(ta.a, bkv, len, nq, kt0),
                                                ta.mask + (int64_t)seq * nq * words, len - nq, words, 0, 0};
  CacheRegs<Cache, D> rg;
  WaveState<D> ws;
  fewq_partial<D, 0, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws);
}

// the plain form's merge: over the live chunks [0, ceil(len / chunk)) of the thread's K/V slice
__global__ __launch_bounds__(256) void tree_merge_kernel(RaggedArgs ra) {
  const SplitArgs& sa = ra.g.s;
  merge_folded(ra.g, [&](int64_t bkv) {
    return min(sa.nchunks, (slice_len(ra, (uint32_t)bkv) + sa.chunk - 1) / sa.chunk);
  });
}

}  // namespace

template <class Args>
hipError_t launch_fwd_f16_tree(const TreeOf<Args>& ta, hipStream_t s) {
  using Cache = CacheOf<Args>;
  const RaggedArgs& ra = Cache::ragged(ta.a);
  const SplitArgs& sa = ra.g.s;
  const hipError_t e = with_fewq_tree(sa.f, Cache::row_keys(ta.a), [&](auto d, auto fast) {
    return launch_fewq_partial(d, tree_partial_kernel<Cache, d.value, fast.value != 0>, ta, sa, s);
  }, Cache::kChunkBytes);
  if (e != hipSuccess) return e;
  return launch_fewq_merge(tree_merge_kernel, ra, sa.f, ra.g.g, s);
}
template hipError_t launch_fwd_f16_tree(const TreeOf<RaggedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_tree(const TreeOf<PagedArgs>&, hipStream_t);
template hipError_t launch_fwd_f16_tree(const TreeOf<RaggedFp8Args>&, hipStream_t);
template hipError_t launch_fwd_f16_tree(const TreeOf<PagedFp8Args>&, hipStream_t);

}  // namespace fa
