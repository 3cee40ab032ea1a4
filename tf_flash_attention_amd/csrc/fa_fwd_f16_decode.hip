// fa_fwd_f16_decode.hip — the plain form of the decode forwards: few queries against one of the four K/V caches of
// fa_fwd_f16_decode.h, every query seeing the slice's live keys (gfx950 MFMA).
//
// The structure is fa_fwd_f16_gqa.hip's — FoldedRows blocks of g heads x pitch rows, one workgroup per (K/V slice,
// key chunk) of grouped_plan's chunks over the capacity, the partial + merge pair of fa_fwd_f16_fewq.h — with the
// slice's length threaded through:
//   * decode_partial_kernel loads and clamps its slice's length as a wave-uniform value.  A chunk that starts at or
//     past it returns before the core and writes nothing; the others run fwd_f16_core over
//     [chunk start, min(chunk end, len)) with the cache's map.
//   * ragged_merge_kernel, the merge of all four caches (it reads neither K / V nor a table nor the scales: v_scale
//     is already in the records), folds only the chunks below len, so no unwritten workspace word reaches an output;
//     len = 0 writes the empty rows (O = 0, l = 0, m = bytes 0xFA).
// Two rules.  Full (POL 0): every query sees keys [0, len).  Tail-causal (POL 1): the nq queries are the last nq
// positions of the sequence, query i sees keys [0, len - nq + i]; queries i < nq - len see nothing.
// With every length equal to the capacity and g >= 2 the full rule over the ragged fp16 cache runs
// gqa_partial_kernel's loop over the same chunks, and the result is bitwise fa_forward_grouped's.
#include "fa_fwd_f16_decode.h"

namespace fa {
namespace {

using namespace f16core;

template <class Cache, int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void decode_partial_kernel(typename Cache::Args args) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = Cache::ragged(args);
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const typename Cache::Rows map = Cache::template rows<D, FAST>(args, bkv, len, sa.f.rule.q.n, kt0);
  CacheRegs<Cache, D> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws);
}

// over the live chunks [0, ceil(len / chunk)) of the thread's K/V slice: every live chunk wrote the records of
// all live rows, and the dead ones are not read
__global__ __launch_bounds__(256) void ragged_merge_kernel(RaggedArgs ra) {
  const SplitArgs& sa = ra.g.s;
  merge_folded(ra.g, [&](int64_t bkv) {
    return min(sa.nchunks, (slice_len(ra, (uint32_t)bkv) + sa.chunk - 1) / sa.chunk);
  });
}

}  // namespace

template <class Args>
hipError_t launch_fwd_f16_decode(const Args& args, hipStream_t s) {
  using Cache = CacheOf<Args>;
  const RaggedArgs& ra = Cache::ragged(args);
  // K / V rows of every slice (or page) start aligned to the cache's chunk where with_pol_fast's do
  const hipError_t e = with_fewq_tail(ra, Cache::row_keys(args), [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, decode_partial_kernel<Cache, d.value, pol.value, fast.value != 0>, args, ra.g.s, s);
  }, Cache::kChunkBytes);
  if (e != hipSuccess) return e;
  return launch_fewq_merge(ragged_merge_kernel, ra, ra.g.s.f, ra.g.g, s);
}
template hipError_t launch_fwd_f16_decode(const RaggedArgs&, hipStream_t);
template hipError_t launch_fwd_f16_decode(const PagedArgs&, hipStream_t);
template hipError_t launch_fwd_f16_decode(const RaggedFp8Args&, hipStream_t);
template hipError_t launch_fwd_f16_decode(const PagedFp8Args&, hipStream_t);

}  // namespace fa
