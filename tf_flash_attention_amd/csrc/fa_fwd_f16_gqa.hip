// fa_fwd_f16_gqa.hip — grouped-query fp16 forward for few queries (gfx950 MFMA).
//
// In grouped-query attention g query slices (heads) share one K/V slice: Q slice bi attends K/V slice
// bi / g.  On expanded K/V the split-key forward (fa_fwd_f16_splitk.hip) would stream every shared key g
// times, each time with nq live columns in a wave's 32.  Here the g heads of a group are folded into the
// 128 query rows of ONE workgroup (FoldedRows, fa_fwd_f16_core.h): row rho = head rho / pitch, query
// rho % pitch, pitch the smallest power of two >= nq, g * pitch <= 128.  K and V stream once per group and
// the MFMA columns fill up.  The key range of the query block [0, nq-1] is cut into chunks
// (fa_api.hip: grouped_plan), also for a short range (one chunk), so there is one path:
//   * gqa_partial_kernel: one workgroup per (K/V slice, chunk) runs fwd_f16_core over its chunk and writes
//     the UNNORMALISED fp32 accumulator of its live rows with their statistics to the workspace;
//   * gqa_merge_kernel: folds the chunks of a row in chunk order (no atomics: deterministic, independent
//     of the batch) and writes O, l, m of query slice bkv * g + j.
// Workspace record of one (K/V slice, chunk): (v_d + 3) rows of g * pitch floats — O[v_d][g * pitch]
// relative to m_run, then m_run (log2 units; -inf where the row attends nothing in the chunk), l and the
// exact row max m_max, the statistics format of fa_fwd_f16_splitk.hip.  Only live rows are written or read.
// A query slice's bits are not those of the ungrouped forward on expanded K/V: the core's lazy rebase is
// taken per wave, so a row's arithmetic depends on which rows share its wave.
#include "fa_fwd_f16_core.h"

namespace fa {
namespace {

using namespace f16core;

constexpr int kNW = 4;       // waves per workgroup: 128 folded rows
constexpr int kF = kFDot2;   // the core's structure flags: fwd_f16_kernel's default form

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kNW * 64, waves_per_eu(D, kF)) void gqa_partial_kernel(GqaArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SplitArgs& sa = ga.s;
  const FwdArgs& a = sa.f;
  constexpr float kNegInf = -__builtin_huge_valf();

  const int nq = a.rule.q.n, vd = FAST ? D : a.v_d;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t bkv = bid / (uint32_t)sa.nchunks;
  const int ch = (int)(bid % (uint32_t)sa.nchunks);

  // ---- this chunk's share [kt0, ce) of the block's key range (kt0 is tile-aligned)
  const int kt0 = sa.k_first + ch * sa.chunk;
  const int ce = min(kt0 + sa.chunk, sa.k_end);
  const int ntiles = ce > kt0 ? (ce - kt0 + kBN - 1) / kBN : 0;

  const FoldedRows map = {ga.g, ga.pitch, ga.log2_pitch};
  WaveRegs<D, kNW> rg;
  WaveState<D> ws;
  fwd_f16_core<D, kNW, POL, FAST, kF, FoldedRows>(a, (lds_char_t*)smem_raw, 0, 0, kt0, ntiles, rg, ws, map, bkv);

  // ---- epilogue: the unnormalised partial of the live rows; stores coalesce along the rows
  const int rho = ws.qi, gp = ga.g * ga.pitch;
  if (!ws.wave_active || rho >= gp || (rho & (ga.pitch - 1)) >= nq) return;
  const float l_tot = ws.l_run + xor32(ws.l_run);
  float* rec = sa.ws + (bkv * sa.nchunks + ch) * (int64_t)(vd + 3) * gp;
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * ws.h;
      if (FAST || v < vd) rec[(int64_t)v * gp + rho] = ws.acc_o[u][i];
    }
  if (ws.h == 0) {
    float* st = rec + (int64_t)vd * gp;
    st[rho] = ws.m_set ? ws.m_run : kNegInf;  // sentinel: the row attends nothing in this chunk
    st[gp + rho] = ws.m_set ? l_tot : 0.f;
    st[2 * gp + rho] = ws.m_max;
  }
}

// One thread per (K/V slice, output channel, head of the group, query), queries fastest.  The chunk loops
// run in fixed order on plain loads, so every thread of a row derives the same ref and L, and the result
// does not depend on the batch or on timing.  The threads of channel 0 also write l and m.
__global__ __launch_bounds__(256) void gqa_merge_kernel(GqaArgs ga) {
  const SplitArgs& sa = ga.s;
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n, vd = a.v_d, nc = sa.nchunks, g = ga.g, gp = ga.g * ga.pitch;
  const int64_t per = (int64_t)vd * g * nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bkv = gid / per;
  const int rem = (int)(gid - bkv * per);
  const int v = rem / (g * nq), t = rem - v * (g * nq);
  const int j = t / nq, q = t - j * nq;
  const int rho = j * ga.pitch + q;
  constexpr float kNegInf = -__builtin_huge_valf();
  const int64_t rstride = (int64_t)(vd + 3) * gp;
  const float* rec = sa.ws + bkv * nc * rstride;
  const float* stat = rec + (int64_t)vd * gp + rho;

  float ref = kNegInf, mmax = kNegInf;
  for (int s = 0; s < nc; ++s) {
    ref = fmaxf(ref, stat[s * rstride]);
    mmax = fmaxf(mmax, stat[s * rstride + 2 * gp]);
  }
  const int64_t bi = bkv * g + j;  // the query slice
  __half* O = static_cast<__half*>(a.O) + bi * (int64_t)vd * nq;
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
    L += stat[s * rstride + gp] * wgt;
    o += rec[s * rstride + (int64_t)v * gp + rho] * wgt;
  }
  O[(int64_t)v * nq + q] = __float2half(o / L);
  if (v == 0) store_lm(lo, mo, q, L, ref, mmax);  // L > 0: the chunk that set ref has l >= 1
}

template <int D>
hipError_t launch_partial_t(const GqaArgs& ga, hipStream_t s) {
  return with_pol_fast<D>(ga.s.f, [&](auto pol, auto fast) {
    auto kern = gqa_partial_kernel<D, decltype(pol)::value, decltype(fast)::value != 0>;
    const int smem = Smem<D, kNW>::kTotal;
    hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(ga.s.f.b * ga.s.nchunks)), dim3(kNW * 64), smem, s, ga);
    return hipGetLastError();
  });
}

}  // namespace

// K/V slices per launch pair: both grids stay below 2^31 blocks.
int64_t fwd_f16_gqa_max_batch(const GqaArgs& ga) {
  const int64_t merge_blocks = ((int64_t)ga.s.f.v_d * ga.g * ga.s.f.rule.q.n + 255) / 256;
  const int64_t per = ga.s.nchunks > merge_blocks ? ga.s.nchunks : merge_blocks;
  return ((1ll << 31) - 1) / per;
}

hipError_t launch_fwd_f16_gqa(const GqaArgs& ga, hipStream_t s) {
  const FwdArgs& a = ga.s.f;
  const int dm = max(a.d, a.v_d);
  hipError_t e = dm <= 32 ? launch_partial_t<32>(ga, s) : dm <= 64 ? launch_partial_t<64>(ga, s)
                                                                     : launch_partial_t<128>(ga, s);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * ga.g * a.rule.q.n;
  hipLaunchKernelGGL(gqa_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ga);
  return hipGetLastError();
}

}  // namespace fa
