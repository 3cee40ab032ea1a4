// fa_fwd_f16_tree.h — the tree-masked draft form of the ragged and paged few-query forwards: what its kernel
// template over the four caches (fa_fwd_f16_tree.hip; the caches: fa_fwd_f16_decode.h) is made of.
//
// The nq queries are the draft tokens of one speculative step, held in the last nq positions of a sequence of len
// live keys: draft slot j is key base + j, base = len - nq.  Every query sees the committed context [0, base) and,
// of the draft slots, those its row of a device bit mask names: word j >> 5, bit j & 31 of row i of
// mask[sequence][nq][W], W = ceil(nq / 32) <= 4.  A tree is not an index interval, so the form cannot be a
// lane_interval like the window's; it is the one hook of the core that a map with kTree switches on
// (fa_fwd_f16_core.h: HasTree), at POL 0:
//   * the tile class: tiles wholly below base are class 2, every other live tile (one that holds a draft slot or
//     the key len) is class 1.  At most three tiles of a chunk are class 1: nq <= 128 keys straddle three.
//   * the mask of a class-1 tile at k0: each lane keeps its query's mask as 128 bits (lo, hi; the bits at or past nq
//     cleared when they are loaded, once, before the key loop) and forms one 64-bit word for the keys
//     [k0, k0 + 64): ones below base, the mask's bits from slot k0 - base on, zeros from len on.  Shifted down by the
//     lane's 4h, each of the 32 score elements is a test of a compile-time bit.
// Masked keys are loaded and masked, never zeroed, so a sequence's keys below len must be finite, as under a window.
// Everything else is the plain form's: the chunk walk over the capacity, the length load, the record, the merge.
// A masked score is a select to -inf in front of the same max, exp and sum chains, and a tile that the tail-causal
// twin skips for a wave adds exact zeros when it is masked instead, so with the lower-triangular mask the results
// are the twin's bits.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_TREE_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_TREE_H_

#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace f16core {

// a map with a draft mask; Base: RaggedRows, PagedRows or their 8-bit forms
template <class Base>
struct TreeRowsOf : Base {
  static constexpr bool kTree = true;
  const uint32_t* mask;  // this sequence's [nq][words] rows
  int32_t base, words;   // len - nq (negative: slots below -base name no key); W
  uint64_t lo, hi;       // this lane's query's slots 0..63 and 64..127, zero from nq on (load_mask)

  // the core's hook, once per lane: query qi's row.  The loop bounds are wave-uniform.
  __device__ __forceinline__ void load_mask(int qi) {
    const uint32_t* row = mask + qi * words;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = this->nq - 32 * j;  // slots of this word
      w[j] = n > 0 ? row[j] & (n >= 32 ? 0xffffffffu : (1u << n) - 1u) : 0u;
    }
    lo = w[0] | ((uint64_t)w[1] << 32);
    hi = w[2] | ((uint64_t)w[3] << 32);
  }
  // the core's hook, per class-1 tile: bit p says whether this lane's query sees key k0 + p.  s = k0 - base is the
  // slot of key k0: -63 <= s (the tile reaches base) and s < nq <= 128 (k0 < len); wave-uniform
  __device__ __forceinline__ uint64_t allowed(int k0) const {
    const int s = k0 - base;
    if (s < 0) return (lo << -s) | ((1ull << -s) - 1ull);
    const uint64_t a = s < 64 ? lo : hi, b = s < 64 ? hi : 0ull;
    const int sh = s & 63;
    return (a >> sh) | ((b << 1) << (63 - sh));
  }
};

// host: the <D, FAST> instantiation of a tree forward (POL 0 always: the hook is the rule)
template <class Launch>
hipError_t with_fewq_tree(const FwdArgs& a, int row_keys, Launch&& launch, int chunk_bytes = 16) {
  return with_fewq_d(a, [&](auto d) {
    return fast_staging<decltype(d)::value>(a, row_keys, chunk_bytes) ? launch(d, IC<1>{}) : launch(d, IC<0>{});
  });
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_TREE_H_
