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
// to its query rows and key range, normalises and writes O, l, m, and launches the kernel that the choice
// (fa_fwd_f16_choice.h) names: its own instances here, the tuned kernels through their files' launchers.
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
hipError_t launch_t(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s) {
  return with_pol_fast(c.pol, c.aligned, [&](auto pol, auto fast) {
    auto kern = fwd_f16_kernel<D, NW, decltype(pol)::value, decltype(fast)::value != 0, F>;
    const int64_t nqb = (a.rule.q.n + Smem<D, NW>::kBM - 1) / Smem<D, NW>::kBM;
    return launch_smem(kern, (unsigned)(a.b * nqb), NW * 64, Smem<D, NW>::kTotal, s, a);
  });
}

// the instance <D, NW, F> of a kGeneral choice
constexpr int inst(int d, int nw, int f) { return (d * 16 + nw) * 128 + f; }

hipError_t launch_general(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s) {
  switch (inst(c.d, c.nw, c.f)) {
    case inst(32, 4, 8): return launch_t<32, 4, 8>(a, c, s);
    case inst(64, 4, 8): return launch_t<64, 4, 8>(a, c, s);
    case inst(64, 8, 8): return launch_t<64, 8, 8>(a, c, s);
    case inst(128, 4, 8): return launch_t<128, 4, 8>(a, c, s);
#ifdef FA_DIAG
    // the pins below 1000: at d <= 32 dot2c row sums (the round-3 default) against MFMA row sums
    case inst(32, 4, 8 | kFMfmaSum): return launch_t<32, 4, 8 | kFMfmaSum>(a, c, s);
    case inst(32, 8, 8): return launch_t<32, 8, 8>(a, c, s);
    case inst(32, 8, 8 | kFMfmaSum): return launch_t<32, 8, 8 | kFMfmaSum>(a, c, s);
    case inst(64, 4, 0): return launch_t<64, 4, 0>(a, c, s);
    case inst(64, 4, 24): return launch_t<64, 4, 24>(a, c, s);
    case inst(64, 4, 56): return launch_t<64, 4, 56>(a, c, s);
    case inst(64, 8, 0): return launch_t<64, 8, 0>(a, c, s);
    case inst(64, 8, 40): return launch_t<64, 8, 40>(a, c, s);
#endif
    default: return hipErrorInvalidValue;  // no such instance is chosen
  }
}

}  // namespace

FwdF16Choice choose_fwd_f16(const FwdArgs& a) {
#ifdef FA_DIAG
  const int variant = diag_variant("FA_FWD_VARIANT");
#else
  constexpr int variant = -1;
#endif
  // only the band's conditions, for local windows, read the XCD count
  return fwd_f16_choice(a, a.rule.policy == 2 ? device_xcds() : 0, variant);
}

hipError_t launch_fwd_f16(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s) {
  switch (c.kernel) {
    case FwdF16::kWide: return launch_fwd_f16_wide(a, c, s);
    case FwdF16::kBand: return launch_fwd_f16_band(a, c, s);
    case FwdF16::kPingpong: return launch_fwd_f16_pingpong(a, c, s);
    case FwdF16::kGap128: return launch_fwd_f16_gap128(a, c, s);
    case FwdF16::kFast: return launch_fwd_f16_fast(a, c, s);
    case FwdF16::kGeneral: return launch_general(a, c, s);
#ifdef FA_DIAG
    case FwdF16::kPp: return launch_fwd_f16_pp(a, c, s);
    case FwdF16::kGap: return launch_fwd_f16_gap(a, c, s);
    case FwdF16::kPingpong128: return launch_fwd_f16_pingpong128(a, c, s);
#endif
    default: return hipErrorInvalidValue;  // kNone, or a study in the product library: never chosen
  }
}

}  // namespace fa
