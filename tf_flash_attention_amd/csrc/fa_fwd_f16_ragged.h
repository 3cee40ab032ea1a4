// fa_fwd_f16_ragged.h — what the ragged (fa_fwd_f16_ragged.hip) and the paged (fa_fwd_f16_paged.hip) few-query
// forwards share on the device: the row map with a per-slice key length and the clamped load of that length.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_RAGGED_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_RAGGED_H_

#include "fa_fwd_f16_core.h"

namespace fa {
namespace f16core {

// FoldedRows with a per-slice key length (fa_fwd_f16_core.h: the row maps)
struct RaggedRows {
  static constexpr bool kFolded = true;
  static constexpr bool kRagged = true;
  static constexpr bool kPaged = false;
  int32_t g, pitch, log2_pitch;
  int32_t len, nq;
  __device__ __forceinline__ int64_t q_slice(int64_t, int64_t bkv) const { return bkv * g; }
  __device__ __forceinline__ int64_t kv_slice(int64_t, int64_t bkv) const { return bkv; }
  __device__ __forceinline__ int wave_q0(int, int w) const { return (32 * w) & (pitch - 1); }
  __device__ __forceinline__ bool wave_active(int wq0, int w, int nq_) const { return 32 * w < g * pitch && wq0 < nq_; }
  __device__ __forceinline__ int lane_q(int, int w, int r) const { return (32 * w + r) & (pitch - 1); }
  __device__ __forceinline__ int lane_row(int, int w, int r) const { return 32 * w + r; }
  __device__ __forceinline__ int key_limit(int) const { return len; }
  // the tail-causal interval (POL 1): empty (khi < 0) for a query before the sequence's first position
  __device__ __forceinline__ void lane_interval(const Rule&, int qi, int* klo, int* khi) const {
    *klo = 0;
    *khi = len - nq + qi;
  }
};

// the length of K/V slice bkv of this launch, clamped to [0, nk]; the same value in every lane
__device__ __forceinline__ int slice_len(const RaggedArgs& ra, uint32_t bkv) {
  const int len = ra.k_lens[ra.len0 + ((uint32_t)ra.rem0 + bkv) / (uint32_t)ra.kv_per_len];
  return min(max(len, 0), ra.g.s.f.rule.k.n);
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_RAGGED_H_
