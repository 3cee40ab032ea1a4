// fa_fwd_f16_paged.hip — few-query fp16 forward over a PAGED K/V cache with a device block table
// (gfx950 MFMA).
//
// A serving stack keeps K and V in pools of fixed-size pages, K_pool [num_pages][Hk][d][page] and V_pool
// [num_pages][Hk][v_d][page] halfs with the key axis contiguous, and a table [sequences][max_pages] of int32 on
// the device: entry [s][p] is the pool page that holds keys [p*page, (p+1)*page) of all Hk heads of sequence s.
// This is fa_fwd_f16_ragged.hip with that indirection: the same chunks over the capacity max_pages * page, the
// same length handling (dead chunks return, staged K / V past the length are zeroed, key_limit = len), the same
// partial records (fa_fwd_f16_fewq.h), and ragged_merge_kernel itself as the merge.  What differs is where a key tile is read from:
//   * page % 64 == 0, so a 64-key tile lies inside one page.  For tile k0 of (sequence s, head hk) PagedRows
//     loads block_table[s * max_pages + k0 / page] as a wave-uniform value, clamps it to [0, num_pages - 1], and
//     answers the core's tile() question with pool + ((entry * Hk + hk) * channels * page) + k0 % page and the
//     row stride `page`.  A page of one head is a [channels][page] block, the shape the core stages anyway.
//   * Only tiles below the length are ever staged, so only the entries of pages that hold a live key are
//     loaded; every page index is capped at (len - 1) / page < max_pages as well, so none leaves the table's row.
//     The entry of the next tile's page is loaded one tile ahead of its use (PagedRows below).
//   * A corrupt table entry is clamped like a corrupt length: the answer is wrong, the access is inside the
//     pool.  The kernels only read the pools and the table; their stores are the partial records and (O, l, m).
// With the pages of every sequence laid out in order this is the ragged forward tile for tile, and the results
// are bitwise fa_forward_ragged's on the gathered cache.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void paged_partial_kernel(PagedArgs pa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RaggedArgs& ra = pa.r;
  const SplitArgs& sa = ra.g.s;
  uint32_t bkv;
  int ch, kt0;
  fewq_block(sa, 0, &bkv, &ch, &kt0);
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv));
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = chunk_tiles(sa, kt0, len);
  const PagedRows map = paged_rows<D, FAST>(pa, bkv, len, kt0);
  WaveRegs<D, kFewqNW> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, map, bkv, ch, kt0, ntiles, rg, ws);
}

}  // namespace

hipError_t launch_fwd_f16_paged(const PagedArgs& pa, hipStream_t s) {
  // a page is a multiple of 8 keys, so with 16-byte aligned pools every page row starts 16-byte aligned
  const hipError_t e = with_fewq_tail(pa.r, pa.page, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, paged_partial_kernel<d.value, pol.value, fast.value != 0>, pa, pa.r.g.s, s);
  });
  if (e != hipSuccess) return e;
  return launch_fwd_f16_ragged_merge(pa.r, s);  // the merge reads neither K / V nor the table
}

}  // namespace fa
