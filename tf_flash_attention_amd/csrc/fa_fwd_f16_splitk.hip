// fa_fwd_f16_splitk.hip — split-key fp16 forward for few queries and many keys (gfx950 MFMA).
//
// Every other forward gives one workgroup a (slice, query block) and walks the keys inside it,
// which leaves the GPU empty when a slice has one query block and a long key range (b = 16,
// nq <= 128, nk = 16384: 16 workgroups on 256 CUs).  Here the rule-bounded key range of the
// single query block is cut into chunks (fa_api.hip: split_plan) and goes through the partial +
// merge pair of fa_fwd_f16_fewq.h with the ungrouped rows (IdentityRows): row q of the block is
// query q of the slice, and a record row is nq floats.
#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace {

using namespace f16core;

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kFewqNW * 64, waves_per_eu(D, kFewqF)) void splitk_partial_kernel(SplitArgs sa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint32_t bi;
  int ch, kt0;
  fewq_block(sa, sa.k_first, &bi, &ch, &kt0);
  const int ntiles = chunk_tiles(sa, kt0, sa.k_end);
  WaveRegs<D, kFewqNW> rg;
  WaveState<D> ws;
  fewq_partial<D, POL, FAST>(sa, (lds_char_t*)smem_raw, IdentityRows{}, bi, ch, kt0, ntiles, rg, ws);
}

__global__ __launch_bounds__(256) void splitk_merge_kernel(SplitArgs sa) {
  int64_t bi;
  int v, j, q;
  if (!merge_thread(sa.f, 1, &bi, &v, &j, &q)) return;
  merge_row(sa, IdentityRows{}.rec_stride(sa.f.rule.q.n), bi, q, v, sa.nchunks, bi, q);
}

}  // namespace

// Slices per launch pair of a few-query forward: both grids stay below 2^31 blocks.
int64_t fwd_f16_fewq_max_batch(int32_t nchunks, int32_t v_d, int64_t rows_out) {
  const int64_t merge_blocks = ((int64_t)v_d * rows_out + 255) / 256;
  const int64_t per = nchunks > merge_blocks ? nchunks : merge_blocks;
  return ((1ll << 31) - 1) / per;
}

hipError_t launch_fwd_f16_splitk(const SplitArgs& sa, hipStream_t s) {
  const hipError_t e = with_fewq_rule(sa.f, [&](auto d, auto pol, auto fast) {
    return launch_fewq_partial(d, splitk_partial_kernel<d.value, pol.value, fast.value != 0>, sa, sa, s);
  });
  if (e != hipSuccess) return e;
  return launch_fewq_merge(splitk_merge_kernel, sa, sa.f, 1, s);
}

}  // namespace fa
