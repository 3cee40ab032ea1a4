// fa_fwd_f16_choice.h — which kernel the fp16 forward launches: the whole decision in one host function.
//
// fwd_f16_choice(a, xcds, variant) is pure: it reads the arguments (of the pointers only their alignment), asks
// the device nothing and reads no environment.  launch_fwd_f16 (fa_fwd_f16.hip) switches over its value and
// fa_forward_kernel (fa_api.hip) prints it, so the two cannot drift.  The order of the questions, the two
// reachability arguments and what left the product library: DESIGN.md §3.17.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CHOICE_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CHOICE_H_

#include <stdint.h>
#include <stdio.h>

#include <string>

#include "fa_kernels.h"
#include "fa_rules.h"

namespace fa {

enum class FwdF16 {
  kNone,     // no fp16 MFMA forward takes these arguments: the caller goes on to the SIMT path
  kWide,     // fa_fwd_f16_wide.hip      fwd_f16_wide_kernel<pol, aligned>
  kBand,     // fa_fwd_f16_band.hip      fwd_f16_band_kernel<f>, f the item's positions T
  kPingpong, // fa_fwd_f16_pingpong.hip  fwd_f16_pingpong_kernel
  kGap128,   // fa_fwd_f16_gap128.hip    fwd_f16_gap128_kernel<pol, f>, f = 1 the ablation behind pin 2701
  kFast,     // fa_fwd_f16_fast.hip      fwd_f16_fast_kernel<d, nw, pol, f>
  kGeneral,  // fa_fwd_f16.hip           fwd_f16_kernel<d, nw, pol, aligned, f>
  // the studies of csrc/diag/, behind a pin of the diagnostic library only
  kPp,           // fwd_f16_pp_kernel<pol, an ablation by the pin>
  kGap,          // fwd_f16_gap_kernel<0, an ablation by the pin>
  kPingpong128,  // fwd_f16_pingpong128_kernel<pol>
};

// one launch: pol, aligned and f count where the kernel's line above names them
struct FwdF16Choice {
  FwdF16 kernel;
  int d, nw;     // channel tile and waves per workgroup
  int pol;       // 0 the full policy, 1 an interval rule (causal, 1d unit-stride local), 2 any other window
  bool aligned;  // K / V rows of whole 16-byte chunks (nk % 8 == 0, both bases on 16 bytes); the general kernel's
                 // FAST staging needs d == v_d == its tile as well
  int f;         // structure flags F of the general and the fast kernel; the band's T; gap128's ablation
  int variant;   // the pin as given, for the forms that some pins select inside a family (21xx, 26xx: the studies'
                 // ablations; 2402: the band's item order), which the launchers read and the name does not show
};

constexpr int kFastF1 = 2 | 4;      // the fast kernel's kFPrio | kFLateV: one key tile per barrier
constexpr int kFastF2 = 2 | 4 | 8;  // the same with kFTpb2: two key tiles per barrier

// b * blocks < 2^31, for b >= 0, without forming the product
inline bool fwd_f16_grid_fits(int64_t b, int64_t blocks) { return blocks <= 0 || b <= 0x7fffffff / blocks; }

// fa_fwd_f16_band.hip: the positions T of the band kernel's instance (9, 13, 17 or 21) where the persistent band
// kernel takes these arguments on a device of `xcds` XCDs, else 0.  Its conditions need the band's constants.
int fwd_f16_band_positions(const FwdArgs& a, int xcds);

inline int fwd_f16_pol(const Rule& r) { return r.policy == 0 ? 0 : (rule_is_interval(r) ? 1 : 2); }

inline bool fwd_f16_kv_aligned(const FwdArgs& a) {
  return a.rule.k.n % 8 == 0 && reinterpret_cast<uintptr_t>(a.K) % 16 == 0 && reinterpret_cast<uintptr_t>(a.V) % 16 == 0;
}

// What every tuned kernel asks of the operands at `block_q` queries a workgroup: aligned K / V rows (16-byte
// staging chunks), at least one key, slices below 2^31 bytes on either side (32-bit buffer offsets) and a grid
// below 2^31 workgroups.
inline bool fwd_f16_tuned_operands(const FwdArgs& a, int block_q) {
  const int64_t nq = a.rule.q.n, nk = a.rule.k.n, dm = a.d > a.v_d ? a.d : a.v_d;
  return fwd_f16_kv_aligned(a) && nk > 0 && dm * nk * 2 < (1ll << 31) && dm * nq * 2 < (1ll << 31) &&
         fwd_f16_grid_fits(a.b, (nq + block_q - 1) / block_q);
}

// variant: -1 in the product library, FA_FWD_VARIANT in the diagnostic one.  A pin whose kernel does not take
// the arguments falls through to the next question.
inline FwdF16Choice fwd_f16_choice(const FwdArgs& a, int xcds, int variant) {
  const int dm = a.d > a.v_d ? a.d : a.v_d;
  const int64_t nq = a.rule.q.n, nk = a.rule.k.n;
  const int pol = fwd_f16_pol(a.rule), v = variant;
  const bool aligned = fwd_f16_kv_aligned(a);
  const FwdF16Choice none = {FwdF16::kNone, 0, 0, 0, false, 0, v};
  if (a.d < 1 || a.v_d < 1 || dm > 256) return none;

  // 128 < max(d, v_d) <= 256, every rule, alignment and length: 256-channel MFMA tiles.  The element-wise
  // staging reads up to 8 keys past a row, inside the slice's 2^31 bytes
  if (dm > 128) {
    const bool fits = nk > 0 && (int64_t)dm * (nk + 8) * 2 < (1ll << 31) && (int64_t)dm * nq * 2 < (1ll << 31) &&
                      fwd_f16_grid_fits(a.b, (nq + 127) / 128);
    return fits ? FwdF16Choice{FwdF16::kWide, 256, 4, pol, aligned, 0, v} : none;
  }
  if (!fwd_f16_grid_fits(a.b, (nq + 127) / 128)) return none;  // the general kernel's grid, at NW = 4

  auto general = [&](int d, int nw, int f) {
    return FwdF16Choice{FwdF16::kGeneral, d, nw, pol, aligned && a.d == d && a.v_d == d, f, v};
  };
  // FA_FWD_VARIANT = <NW><F> below 1000 pins the general kernel (A/B runs), e.g. 408; at d <= 32, 308 / 372 are
  // the 4-wave kernel with dot2c / MFMA row sums
  const bool pinned = v >= 0 && v < 1000;
  if (pinned && dm <= 32 && (v == 308 || v == 372 || v == 808 || v == 872)) return general(32, v / 100 == 3 ? 4 : 8, v % 100);
  if (pinned && dm > 32 && dm <= 64 &&
      (v == 400 || v == 408 || v == 424 || v == 456 || v == 800 || v == 808 || v == 840))
    return general(64, v / 100, v % 100);

  // the tuned kernels: 32 < max(d, v_d) <= 128 under the full policy and the interval rules.  The 128 queries
  // are the fast kernel's smallest block; band, ping-pong, gap128 and the studies run 256 a workgroup, and
  // ceil(nq / 256) <= ceil(nq / 128), so none of them asks more of the operands than this line
  if (!pinned && dm > 32 && pol != 2 && fwd_f16_tuned_operands(a, 128)) {
    const bool d64 = dm <= 64;
    auto fast = [&](int d, int nw, int f) { return FwdF16Choice{FwdF16::kFast, d, nw, pol, true, f, v}; };
    // pins of one structure onto a shape the order below would send elsewhere (parity coverage of every rule
    // each accepts): the studies of csrc/diag/, the shipped ping-pong and gap128, the fast kernel's instances
    if (d64 && v >= 2000 && v < 2200) return {FwdF16::kPp, 64, 4, pol, true, 0, v};  // 21xx: its ablations
    if (d64 && pol == 0 && v == 2200) return {FwdF16::kPingpong, 64, 8, 0, true, 0, v};
    if (d64 && pol == 0 && v >= 2600 && v < 2700) return {FwdF16::kGap, 64, 4, 0, true, 0, v};  // 26xx: its ablations
    if (!d64 && v >= 2700 && v < 2800) return {FwdF16::kGap128, 128, 4, pol, true, v == 2701, v};
    if (!d64 && v == 2301) return {FwdF16::kPingpong128, 128, 8, pol, true, 0, v};
    if (d64 && v == 1814) return fast(64, 8, kFastF2);
    if (v == 146) return d64 ? fast(64, 4, kFastF1) : fast(128, 4, kFastF1);
    if (v < 0 || (v >= 2400 && v < 2500)) {
      // 1d local windows at d <= 64: the persistent band kernel (no per-block start / end cost)
      const int T = a.rule.policy == 2 ? fwd_f16_band_positions(a, xcds) : 0;
      if (T) return {FwdF16::kBand, 64, 8, 1, true, T, v};
    }
    if (v < 0) {
      // the full policy at d <= 64: the ping-pong kernel (two wave groups alternating MFMA / softmax phases;
      // c2: 948 against 904 TF/s for the 8-wave fast kernel)
      if (d64 && pol == 0) return {FwdF16::kPingpong, 64, 8, 0, true, 0, v};
      // d in (64, 128], full and causal policies: the one-wave gap-stream kernel (c3 forward 2.29 against 2.40 ms
      // for the ping-pong of csrc/diag/, full policy at c3's shape 3.95 against 4.34: DESIGN.md §3.0b)
      if (!d64 && a.rule.policy != 2) return {FwdF16::kGap128, 128, 4, pol, true, 0, v};
    }
    // what is left without a pin: causal and declined local windows at d <= 64, local windows above.
    // Tuned on MI355X: full-length key loops 8 waves x 32 queries, two key tiles per barrier; rule-bounded short
    // loops (local windows, c4) 4-wave blocks with one tile per barrier (48 KB of LDS) so two blocks per CU
    // cover each other's prologue / epilogue; at D = 128 4 waves (one per SIMD)
    if (!d64) return fast(128, 4, kFastF1);
    return a.rule.policy == 2 ? fast(64, 4, kFastF1) : fast(64, 8, kFastF2);
  }

  if (dm <= 32) return general(32, 4, 8);
  // local bands: ~10 key tiles per block, so block prologue / epilogue matter; 4-wave blocks let two blocks
  // per CU cover each other's (c4: 5.2 vs 5.9 ms)
  if (dm <= 64) return a.rule.policy == 2 ? general(64, 4, 8) : general(64, 8, 8);
  return general(128, 4, 8);
}

// the kernel instance as a kernel trace prints its template arguments
inline std::string fwd_f16_choice_name(const FwdF16Choice& c) {
  char s[96];
  const char* al = c.aligned ? "true" : "false";
  switch (c.kernel) {
    case FwdF16::kNone: return "none";
    case FwdF16::kWide: snprintf(s, sizeof s, "fwd_f16_wide_kernel<%d, %s>", c.pol, al); break;
    case FwdF16::kBand: snprintf(s, sizeof s, "fwd_f16_band_kernel<%d>", c.f); break;
    case FwdF16::kPingpong: return "fwd_f16_pingpong_kernel";
    case FwdF16::kGap128: snprintf(s, sizeof s, "fwd_f16_gap128_kernel<%d, %d>", c.pol, c.f); break;
    case FwdF16::kFast: snprintf(s, sizeof s, "fwd_f16_fast_kernel<%d, %d, %d, %d>", c.d, c.nw, c.pol, c.f); break;
    case FwdF16::kGeneral: snprintf(s, sizeof s, "fwd_f16_kernel<%d, %d, %d, %s, %d>", c.d, c.nw, c.pol, al, c.f); break;
    case FwdF16::kPp: return "fwd_f16_pp_kernel";
    case FwdF16::kGap: return "fwd_f16_gap_kernel";
    case FwdF16::kPingpong128: snprintf(s, sizeof s, "fwd_f16_pingpong128_kernel<%d>", c.pol); break;
  }
  return s;
}

// fa_fwd_f16.hip: the choice for the current device (and, in the diagnostic library, FA_FWD_VARIANT), and the
// launch of a choice other than kNone
FwdF16Choice choose_fwd_f16(const FwdArgs& a);
hipError_t launch_fwd_f16(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);

// One launcher per kernel file, each for the choice of its own kind `c` of these arguments.
// 128 < max(d, v_d) <= 256: 256-channel MFMA tiles; interval rules by key ranges, strided / 2d windows by
// per-element masks, element-wise staging where K / V rows are not aligned — fa_fwd_f16_wide.hip
hipError_t launch_fwd_f16_wide(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
// persistent band forward for 1d unit-stride local windows, 32 < d <= 64 = v_d — fa_fwd_f16_band.hip
hipError_t launch_fwd_f16_band(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
// ping-pong forward (8 waves, two groups alternating MFMA / softmax phases), the full policy at
// 32 < max(d, v_d) <= 64 — fa_fwd_f16_pingpong.hip
hipError_t launch_fwd_f16_pingpong(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
// one-wave gap-stream forward for 64 < max(d, v_d) <= 128, full and causal — fa_fwd_f16_gap128.hip
hipError_t launch_fwd_f16_gap128(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
// streamlined forward at channel tiles 64 and 128 under the interval rules — fa_fwd_f16_fast.hip
hipError_t launch_fwd_f16_fast(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
#ifdef FA_DIAG
// the studies of csrc/diag/: the paired-block forward (one wave per SIMD, 20xx / 21xx), the hand-placed gap
// stream at d <= 64 (26xx) and the ping-pong at 64 < max(d, v_d) <= 128 (2301)
hipError_t launch_fwd_f16_pp(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
hipError_t launch_fwd_f16_gap(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
hipError_t launch_fwd_f16_pingpong128(const FwdArgs& a, const FwdF16Choice& c, hipStream_t s);
#endif

}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CHOICE_H_
