// fa_fwd_f16_splitk.hip — split-key fp16 forward for few queries and many keys (gfx950 MFMA).
//
// Every other forward gives one workgroup a (slice, query block) and walks the keys inside it,
// which leaves the GPU empty when a slice has one query block and a long key range (b = 16,
// nq <= 128, nk = 16384: 16 workgroups on 256 CUs).  Here the rule-bounded key range of the
// single query block is cut into chunks (fa_api.hip: split_plan):
//   * splitk_partial_kernel: one workgroup per (slice, chunk) runs fwd_f16_core
//     (fa_fwd_f16_core.h, the key loop of the general kernel fwd_f16_kernel) over its chunk
//     only and writes the UNNORMALISED fp32 accumulator with its statistics to the workspace;
//   * splitk_merge_kernel: folds the chunks of a query in fixed order (no atomics, so the result
//     is deterministic and independent of the batch) into the usual O, l, m.
// Workspace record of one (slice, chunk): (v_d + 3) rows of nq floats — O[v_d][nq] relative to
// m_run, then m_run[nq] (log2 units; -inf where the row attends nothing in the chunk), l[nq]
// and the exact row max m_max[nq].
#include "fa_fwd_f16_core.h"

namespace fa {
namespace {

using namespace f16core;

constexpr int kNW = 4;       // waves per workgroup: one query block of 128 rows
constexpr int kF = kFDot2;   // the core's structure flags: fwd_f16_kernel's default form

// One workgroup = 4 waves = the (single) query block of one slice x one key chunk.
// POL / FAST: see fwd_f16_core.  At nq <= 32 one wave computes and the other three only keep
// loads in flight.
template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kNW * 64, waves_per_eu(D, kF)) void splitk_partial_kernel(SplitArgs sa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const FwdArgs& a = sa.f;
  constexpr float kNegInf = -__builtin_huge_valf();

  const int nq = a.rule.q.n, vd = FAST ? D : a.v_d;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t bi = bid / (uint32_t)sa.nchunks;
  const int ch = (int)(bid % (uint32_t)sa.nchunks);

  // ---- this chunk's share [kt0, ce) of the block's key range (kt0 is tile-aligned)
  const int kt0 = sa.k_first + ch * sa.chunk;
  const int ce = min(kt0 + sa.chunk, sa.k_end);
  const int ntiles = (ce - kt0 + kBN - 1) / kBN;

  WaveRegs<D, kNW> rg;
  WaveState<D> ws;
  fwd_f16_core<D, kNW, POL, FAST, kF>(a, (lds_char_t*)smem_raw, bi, 0, kt0, ntiles, rg, ws);

  // ---- epilogue: the unnormalised partial of (slice bi, chunk ch); stores coalesce along nq
  const int qi = ws.qi;
  if (!ws.wave_active || qi >= nq) return;
  const float l_tot = ws.l_run + xor32(ws.l_run);
  float* rec = sa.ws + (bi * sa.nchunks + ch) * (int64_t)(vd + 3) * nq;
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * ws.h;
      if (FAST || v < vd) rec[(int64_t)v * nq + qi] = ws.acc_o[u][i];
    }
  if (ws.h == 0) {
    float* st = rec + (int64_t)vd * nq;
    st[qi] = ws.m_set ? ws.m_run : kNegInf;  // sentinel: the row attends nothing in this chunk
    st[nq + qi] = ws.m_set ? l_tot : 0.f;
    st[2 * nq + qi] = ws.m_max;
  }
}

// One thread per (slice, output channel, query), queries fastest.  The chunk loops run in fixed
// order on plain loads, so every thread of a query derives the same ref and L, and the result
// does not depend on the batch or on timing.  The threads of channel 0 also write l and m.
__global__ __launch_bounds__(256) void splitk_merge_kernel(SplitArgs sa) {
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n, vd = a.v_d, nc = sa.nchunks;
  const int64_t per = (int64_t)vd * nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bi = gid / per;
  const int rem = (int)(gid - bi * per);
  const int v = rem / nq, q = rem - v * nq;
  constexpr float kNegInf = -__builtin_huge_valf();
  const int64_t rstride = (int64_t)(vd + 3) * nq;
  const float* rec = sa.ws + bi * nc * rstride;
  const float* stat = rec + (int64_t)vd * nq + q;

  float ref = kNegInf, mmax = kNegInf;
  for (int s = 0; s < nc; ++s) {
    ref = fmaxf(ref, stat[s * rstride]);
    mmax = fmaxf(mmax, stat[s * rstride + 2 * nq]);
  }
  __half* O = static_cast<__half*>(a.O) + bi * per;
  float* lo = static_cast<float*>(a.l) + bi * (int64_t)nq;
  __half* mo = static_cast<__half*>(a.m) + bi * (int64_t)nq;
  if (ref == kNegInf) {  // no allowed key anywhere
    O[(int64_t)v * nq + q] = __float2half(0.f);
    if (v == 0) store_lm(lo, mo, q, 0.f, ref, mmax);
    return;
  }
  float L = 0.f, o = 0.f;
  for (int s = 0; s < nc; ++s) {
    const float wgt = __builtin_amdgcn_exp2f(stat[s * rstride] - ref);  // 0 for an empty chunk
    L += stat[s * rstride + nq] * wgt;
    o += rec[s * rstride + (int64_t)v * nq + q] * wgt;
  }
  O[(int64_t)v * nq + q] = __float2half(o / L);
  if (v == 0) store_lm(lo, mo, q, L, ref, mmax);  // L > 0: the chunk that set ref has l >= 1
}

template <int D>
hipError_t launch_partial_t(const SplitArgs& sa, hipStream_t s) {
  return with_pol_fast<D>(sa.f, [&](auto pol, auto fast) {
    auto kern = splitk_partial_kernel<D, decltype(pol)::value, decltype(fast)::value != 0>;
    const int smem = Smem<D, kNW>::kTotal;
    hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(sa.f.b * sa.nchunks)), dim3(kNW * 64), smem, s, sa);
    return hipGetLastError();
  });
}

}  // namespace

// Slices per launch pair: both grids stay below 2^31 blocks.
int64_t fwd_f16_splitk_max_batch(const SplitArgs& sa) {
  const int64_t merge_blocks = ((int64_t)sa.f.v_d * sa.f.rule.q.n + 255) / 256;
  const int64_t per = sa.nchunks > merge_blocks ? sa.nchunks : merge_blocks;
  return ((1ll << 31) - 1) / per;
}

hipError_t launch_fwd_f16_splitk(const SplitArgs& sa, hipStream_t s) {
  const FwdArgs& a = sa.f;
  const int dm = max(a.d, a.v_d);
  hipError_t e = dm <= 32 ? launch_partial_t<32>(sa, s) : dm <= 64 ? launch_partial_t<64>(sa, s)
                                                                     : launch_partial_t<128>(sa, s);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * a.rule.q.n;
  hipLaunchKernelGGL(splitk_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, sa);
  return hipGetLastError();
}

}  // namespace fa
