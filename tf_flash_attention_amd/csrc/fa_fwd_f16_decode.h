// fa_fwd_f16_decode.h — the four K/V caches of the decode forwards as traits (gfx950 MFMA).
//
// A decode forward is a cache times a form.  The cache says where the keys lie and how they are staged: ragged
// (a padded K/V with per-sequence lengths) or paged (page pools behind a device block table), fp16 or FP8.  The
// form says which keys a workgroup works: plain (fa_fwd_f16_decode.hip), under a sliding window
// (fa_fwd_f16_window.h, .hip), over query blocks (fa_fwd_f16_prefill.h, .hip) or with the last nq keys behind a
// device bit mask (fa_fwd_f16_tree.h, .hip).  Each form is ONE kernel template over `class Cache`; a cache supplies
//   Args         its argument struct (fa_kernels.h), which a form wraps in WindowOf<> / PrefillOf<> / TreeOf<>
//   Rows         its row map (fa_fwd_f16_fewq.h), which a form wraps in WindowRowsOf<> / BlockRowsOf<> / TreeRowsOf<>
//   ragged(a)    the RaggedArgs inside a: the plan, the lengths, what the merge reads
//   row_keys(a)  host: the keys between two channel rows of K / V (the capacity, or the page)
//   kChunkBytes  the bytes of 8 keys: with_fewq_tail's alignment unit
//   rows<D, FAST>(a, bkv, len, nq, kt0)
//                the map of K/V slice bkv with `len` >= 1 live keys seen by nq queries, for the chunk at kt0 < len
// so a new cache is one struct here and a new form one kernel template.
//
// The ragged caches: K [b/g][d][cap] and V [b/g][v_d][cap], slice bkv holding only
// len = k_lens[bkv / kv_per_len] live keys, a DEVICE value that changes from step to step (the call is replayed
// from a captured graph, so the host never sees it).  RaggedRows' key_limit is len while the capacity stays the row
// stride: tiles wholly below len keep the unguarded staging, and in the tile that holds len the core zeroes staged
// K and V past it element by element.
// The paged caches: K_pool [num_pages][Hk][d][page] and V_pool [num_pages][Hk][v_d][page]
// with the key axis contiguous, and a table [sequences][max_pages] of int32 on the device: entry [s][p] is the pool
// page that holds keys [p*page, (p+1)*page) of all Hk heads of sequence s.  page % 64 == 0, so a 64-key tile lies
// inside one page, and a page of one head is a [channels][page] block, the shape the core stages anyway.  Only the
// entries of pages that hold a live key are loaded, one tile ahead of their use, and each is clamped to
// [0, num_pages - 1] like a corrupt length: the answer is wrong, the access is inside the pool (PagedRows).
// The FP8 caches: the same layouts in OCP e4m3fn bytes, the true key k_scale[h] * K8 and the true value
// v_scale[h] * V8 with h the slice's head among the kv_per_len heads of its sequence; device arrays that only the
// kernel reads (null: 1.0).  The 8-bit cache is a staging concern of the core (fa_fwd_f16_core.h: KvOf): half the
// bytes loaded, converted exactly to the same fp16 LDS image; where the scales go: kv8_mul (fa_fwd_f16_fewq.h).
// Bitwise twins: the paged forward on pages laid out in order is the ragged forward on the gathered cache, and an
// FP8 forward with both scales null or 1.0 is the fp16 forward on the cache converted to fp16.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_DECODE_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_DECODE_H_

#include <utility>

#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace f16core {

struct RaggedCache {
  using Args = RaggedArgs;
  using Rows = RaggedRows;
  static constexpr int kChunkBytes = 16;
  static __host__ __device__ __forceinline__ const RaggedArgs& ragged(const Args& a) { return a; }
  static int row_keys(const Args& a) { return a.g.s.f.rule.k.n; }
  template <int D, bool FAST>
  static __device__ __forceinline__ Rows rows(const Args& a, uint32_t, int len, int nq, int) {
    return {folded_rows(a.g), len, nq};
  }
};

struct PagedCache {
  using Args = PagedArgs;
  using Rows = PagedRows;
  static constexpr int kChunkBytes = 16;
  static __host__ __device__ __forceinline__ const RaggedArgs& ragged(const Args& a) { return a.r; }
  static int row_keys(const Args& a) { return a.page; }
  // (the first entry loaded is the first staged tile's, and the look-ahead stops at page (len - 1) / page)
  template <int D, bool FAST>
  static __device__ __forceinline__ Rows rows(const Args& a, uint32_t bkv, int len, int nq, int kt0) {
    Rows r = paged_rows<D, FAST>(a, bkv, len, kt0);
    r.nq = nq;
    return r;
  }
};

struct RaggedCache8 {
  using Args = RaggedFp8Args;
  using Rows = RaggedRows8;
  static constexpr int kChunkBytes = 8;
  static __host__ __device__ __forceinline__ const RaggedArgs& ragged(const Args& a) { return a.r; }
  static int row_keys(const Args& a) { return a.r.g.s.f.rule.k.n; }
  template <int D, bool FAST>
  static __device__ __forceinline__ Rows rows(const Args& a, uint32_t bkv, int len, int nq, int) {
    const RaggedArgs& ra = a.r;
    const Kv8Mul sc = kv8_mul(a.k_scale, a.v_scale, (int)(((uint32_t)ra.rem0 + bkv) % (uint32_t)ra.kv_per_len));
    return {{folded_rows(ra.g), len, nq}, sc.kmul, sc.qmul, sc.vmul};
  }
};

struct PagedCache8 {
  using Args = PagedFp8Args;
  using Rows = PagedRows8;
  static constexpr int kChunkBytes = 8;
  static __host__ __device__ __forceinline__ const RaggedArgs& ragged(const Args& a) { return a.p.r; }
  static int row_keys(const Args& a) { return a.p.page; }
  template <int D, bool FAST>
  static __device__ __forceinline__ Rows rows(const Args& a, uint32_t bkv, int len, int nq, int kt0) {
    const PagedRows r = PagedCache::rows<D, FAST>(a.p, bkv, len, nq, kt0);
    const Kv8Mul sc = kv8_mul(a.k_scale, a.v_scale, r.hk);
    return {r, sc.kmul, sc.qmul, sc.vmul};
  }
};

// the cache of an argument struct (declarations only: CacheOf reads the return type)
RaggedCache cache_of(const RaggedArgs&);
PagedCache cache_of(const PagedArgs&);
RaggedCache8 cache_of(const RaggedFp8Args&);
PagedCache8 cache_of(const PagedFp8Args&);
template <class Args>
using CacheOf = decltype(cache_of(std::declval<const Args&>()));

// the registers a cache's staging keeps (fa_fwd_f16_core.h: KvOf)
template <class Cache, int D>
using CacheRegs = WaveRegs<D, kFewqNW, typename KvOf<typename Cache::Rows>::Reg>;

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_DECODE_H_
