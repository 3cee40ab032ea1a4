// fa_fwd_f16_ragged.hip — few-query fp16 forward over a padded K/V cache with per-sequence key lengths
// (gfx950 MFMA).
//
// A decode batch is ragged: K and V are laid out for a common capacity nk, and K/V slice bkv holds only
// len = k_lens[bkv / kv_per_len] live keys, a DEVICE value that changes from step to step (the call is
// replayed from a captured graph, so the host never sees it).  The structure is fa_fwd_f16_gqa.hip's —
// FoldedRows blocks of g heads x pitch rows, one workgroup per (K/V slice, key chunk) of grouped_plan's
// chunks over the capacity, the partial + merge pair of fa_fwd_f16_fewq.h — with the length threaded through:
//   * ragged_partial_kernel loads and clamps its slice's length as a wave-uniform value.  A chunk that
//     starts at or past it returns before the core and writes nothing; the others run fwd_f16_core over
//     [chunk start, min(chunk end, len)) with RaggedRows, whose key_limit is len while the capacity stays
//     the row stride.  Tiles wholly below len keep the unguarded 16-byte staging; in the tile that holds
//     len the core zeroes staged K and V past it element by element.
//   * ragged_merge_kernel folds only the chunks below len, so no unwritten workspace word reaches an output;
//     len = 0 writes the empty rows (O = 0, l = 0, m = bytes 0xFA).
// Two forms.  Full (POL 0): every query sees keys [0, len).  Tail-causal (POL 1): the nq queries are the last
// nq positions of the sequence, query i sees keys [0, len - nq + i]; queries i < nq - len see nothing.
// With every length equal to the capacity and g >= 2 the full form runs gqa_partial_kernel's loop over the
// same chunks, and the result is bitwise fa_forward_grouped's.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void ragged_partial_kernel(RaggedArgs ra) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const GqaArgs& ga = ra.g;
  const SplitArgs& sa = ga.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const RaggedRows map = {folded_rows(ga), len, sa.f.rule.q.n};
  WaveRegs<D, kFewqNW> rg;
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

// (also the merge of the paged forward, fa_fwd_f16_paged.hip: the same records, lengths and outputs)
hipError_t launch_fwd_f16_ragged_merge(const RaggedArgs& ra, hipStream_t s) {
  return launch_fewq_merge(ragged_merge_kernel, ra, ra.g.s.f, ra.g.g, s);
}

hipError_t launch_fwd_f16_ragged(const RaggedArgs& ra, hipStream_t s) {
  // the capacity is the row stride: K / V rows of every slice start 16-byte aligned where with_pol_fast's do
  const hipError_t e = with_fewq_tail(ra, ra.g.s.f.rule.k.n, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, ragged_partial_kernel<d.value, pol.value, fast.value != 0>, ra, ra.g.s, s);
  });
  if (e != hipSuccess) return e;
  return launch_fwd_f16_ragged_merge(ra, s);
}

}  // namespace fa
