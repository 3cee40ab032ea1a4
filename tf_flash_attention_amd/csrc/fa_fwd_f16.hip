// fa_fwd_f16.hip — fp16 fused attention forward on gfx950 MFMA: the general kernel.
//
// Replaces the reference's ForwardImpl (flash_attention.cu:425-1077), which ran
// QKᵀ and PV as scalar SIMT FMAs with fp16 accumulation and serialised the
// O/l/m read-modify-write of every (query block, key block) pair through a
// global spin lock.  Here one workgroup = NW waves = 32*NW query rows of one
// (batch, head) slice; the key loop runs inside the workgroup (FA2 order) so
// O, l, m live in registers and are written exactly once — no locks, no memsets.
// The key range of the block is bounded arithmetically from the rule, so skipped
// tiles cost nothing (causal, local bands).
// The key loop itself (staging, transposed scores on MFMA, log2-domain online
// softmax, tile classes, the three POL forms) is fwd_f16_core in
// fa_fwd_f16_core.h, shared with the split-key forward; this file maps a block
// to its query rows and key range, normalises and writes O, l, m, and chooses
// the instantiation.
#include "fa_fwd_f16_core.h"

#include <stdlib.h>

namespace fa {
namespace {

using namespace f16core;

// One workgroup = NW waves = 32*NW query rows of one (batch, head) slice, over the
// rule-bounded key range of those rows.  POL / FAST / F: see fwd_f16_core.
template <int D, int NW, int POL, bool FAST, int F>
__global__ __launch_bounds__(NW * 64, waves_per_eu(D, F)) void fwd_f16_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int kBM = Smem<D, NW>::kBM;

  const int nq = a.rule.q.n, nk = a.rule.k.n, vd = FAST ? D : a.v_d;
  const uint32_t nqb = (nq + kBM - 1) / kBM;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t bi = bid / nqb;
  const int q0 = (int)(nqb - 1 - (bid % nqb)) * kBM;  // latest (heaviest under causal) blocks first

  // ---- key range of this query block (rule-bounded)
  const int qlast = min(q0 + kBM, nq) - 1;
  int kb = 0, ke = nk;
  if (POL != 0) k_range_for_q_block(a.rule, q0, qlast, &kb, &ke);
  const int kt0 = (kb / kBN) * kBN;
  const int ntiles = (ke > kb) ? (ke - kt0 + kBN - 1) / kBN : 0;

  WaveRegs<D, NW> rg;
  WaveState<D> ws;
  fwd_f16_core<D, NW, POL, FAST, F>(a, (lds_char_t*)smem_raw, bi, q0, kt0, ntiles, rg, ws);

  if (!ws.wave_active) return;
  const int qi = ws.qi;
  const float l_tot = (F & kFMfmaSum) ? ws.acc_l[0] : ws.l_run + xor32(ws.l_run);
  const float inv = (l_tot > 0.f) ? 1.f / l_tot : 0.f;
  if (qi < nq) {
    __half* O = static_cast<__half*>(a.O) + bi * (int64_t)vd * nq;
#pragma unroll
    for (int u = 0; u < D / 32; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * ws.h;
        if (FAST || v < vd) O[(int64_t)v * nq + qi] = __float2half(ws.acc_o[u][i] * inv);
      }
    if (ws.h == 0)
      store_lm(static_cast<float*>(a.l) + bi * (int64_t)nq, static_cast<__half*>(a.m) + bi * (int64_t)nq, qi,
               l_tot, ws.m_run, ws.m_max);
  }
}

template <int D, int NW, int F>
hipError_t launch_t(const FwdArgs& a, hipStream_t s) {
  return with_pol_fast<D>(a, [&](auto pol, auto fast) {
    auto kern = fwd_f16_kernel<D, NW, decltype(pol)::value, decltype(fast)::value != 0, F>;
    const int64_t nqb = (a.rule.q.n + Smem<D, NW>::kBM - 1) / Smem<D, NW>::kBM;
    const int smem = Smem<D, NW>::kTotal;
    hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.b * nqb)), dim3(NW * 64), smem, s, a);
    return hipGetLastError();
  });
}

}  // namespace

bool fwd_f16_supported(const FwdArgs& a) {
  if (fwd_f16_wide_supported(a)) return true;
  return a.d >= 1 && a.v_d >= 1 && a.d <= 128 && a.v_d <= 128 && a.b * ((a.rule.q.n + 127) / 128) < (1ll << 31);
}

hipError_t launch_fwd_f16(const FwdArgs& a, hipStream_t s) {
  const int dm = max(a.d, a.v_d);
  // 128 < max(d, v_d) <= 256, every rule and alignment: 256-channel MFMA tiles (fa_fwd_f16_wide.hip)
  if (dm > 128) return launch_fwd_f16_wide(a, s);
#ifdef FA_DIAG
  // FA_FWD_VARIANT = <NW><F> below 1000 pins this general kernel (A/B runs), e.g. 408
  const int v = diag_variant("FA_FWD_VARIANT");
  if (v >= 0 && v < 1000 && dm <= 32) {  // d <= 32: 308 dot2c row sums (the round-3 default), 372 MFMA row sums
    if (v == 308) return launch_t<32, 4, 8>(a, s);
    if (v == 372) return launch_t<32, 4, 8 | kFMfmaSum>(a, s);
    if (v == 808) return launch_t<32, 8, 8>(a, s);
    if (v == 872) return launch_t<32, 8, 8 | kFMfmaSum>(a, s);
  }
  if (v >= 0 && v < 1000 && dm > 32 && dm <= 64) {
    switch (v) {
      case 400: return launch_t<64, 4, 0>(a, s);
      case 408: return launch_t<64, 4, 8>(a, s);
      case 424: return launch_t<64, 4, 24>(a, s);
      case 456: return launch_t<64, 4, 56>(a, s);
      case 800: return launch_t<64, 8, 0>(a, s);
      case 808: return launch_t<64, 8, 8>(a, s);
      case 840: return launch_t<64, 8, 40>(a, s);
      default: break;
    }
  }
  const bool pinned = v >= 0 && v < 1000;
#else
  constexpr bool pinned = false;
#endif
  if (!pinned && fwd_f16_fast_supported(a)) return launch_fwd_f16_fast(a, s);
  if (dm <= 32) return launch_t<32, 4, 8>(a, s);
  if (dm <= 64) {
    // local bands: ~10 key tiles per block, so block prologue/epilogue matter;
    // 4-wave blocks let two blocks per CU cover each other's (c4: 5.2 vs 5.9 ms)
    if (a.rule.policy == 2) return launch_t<64, 4, 8>(a, s);
    return launch_t<64, 8, 8>(a, s);
  }
  return launch_t<128, 4, 8>(a, s);
}

}  // namespace fa
