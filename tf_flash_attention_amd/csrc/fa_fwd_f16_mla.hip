// fa_fwd_f16_mla.hip — MLA decode: few queries of many heads against ONE latent K/V head held in a paged pool,
// up to 576 score channels and 512 value channels (gfx950 MFMA).
//
// In absorbed form a multi-head latent attention decode step is multi-query attention whose keys are the cached
// latent vectors (C channels, 576 = 512 latent + 64 rotary) and whose values are the first v_d channels of the
// SAME vectors.  So there is one pool, [num_pages][C][page] halfs with the key axis contiguous, and a 64-key tile
// of it, [C][64], is both the K operand of S^T = K^T.Q (contraction over channels) and, in its first v_d rows,
// the V operand of O^T += V.P^T (contraction over keys).  It crosses HBM -> LDS once and is read two ways from one
// image: transposed (ds_read_b64_tr_b16) as K, row-wise (ds_read_b128) as V.
//
// The work: the Hq heads x P query slots (P the smallest power of two >= nq) are folded into R = Hq * P rows, row
// rho = head * P + query.  One workgroup of 4 waves, one per SIMD with the whole register file, takes (sequence,
// block of 64 rows, key chunk of the plan) and writes a FewqRecord (fa_fwd_f16_fewq.h) of stride 64: fp32
// unnormalised O^T and (m_run, l, m_max) per row; mla_merge_kernel folds the live chunks of a row in chunk order
// with the few-query forwards' merge_row, no atomics.
//
//   wave (rh, cw) = (w >> 1, w & 1) owns rows 32 rh .. 32 rh + 31 and the 64-channel groups G = cw, cw + 2, ... of
//   O^T.  Per 64-key tile it forms S^T for its own 32 keys, 32 cw .. 32 cw + 31, over all C channels (C / 16 MFMAs),
//   hands the fp32 scores to the other wave of its row pair through LDS (4 KB a wave) and takes that wave's; both
//   then run the same softmax over the 64 keys (bit-identical statistics, twice the exp2 but no second hand-over
//   for the row maxima) and each runs the PV MFMAs of its own channel groups (v_d / 32 in all, 2 per group and
//   k-step).  At (576, 512): 36 + 32 = 68 v_mfma_f32_32x32x16_f16 per wave and tile.
//
//   registers (512 a wave; built with MFMA results in VGPRs, Makefile): Q fragments of all 36 k-steps 144, O^T 128,
//   the next tile's 18 16-byte chunks 72, scores 32, two groups of K or V fragments 32, P 16; the compiler keeps
//   the Q fragments in AGPRs and copies each to VGPRs before its MFMA (profiles/mla_resources.txt: no scratch).
//   LDS: tile ring 2 x 72 KB (tile i in slot i & 1), hand-over 4 x 4 KB: 160 KB.
//   LDS image of a tile: row c = channel, 128 bytes = 64 keys, the 16-byte chunk x of row c at x ^ f(c),
//   f(c) = bit 1 of c as bit 2 | bits 2..3 of c as bits 0..1: the four rows of a transposed read fall into four
//   different 32-byte bank groups, and 16 consecutive rows of a b128 read into 8 chunk positions x 2 row parities
//   (the bank-conflict counter reads 0).
//   staging: the table entry of tile i + 2 and the global loads of the whole tile i + 1 are issued at the head of
//   tile i and stay in flight through it, the LDS stores follow its MFMAs; two barriers a tile (hand-over,
//   publish).  The fragments of an MFMA group are read from LDS one group ahead (one wave per SIMD: no other wave
//   hides the round trip).
//
// Numerics are the other fp16 forwards': Q pre-scaled by softmax_scale * log2(e) in fp32 and rounded to fp16 once,
// scores and statistics in fp32 with the exact row maximum as the reference (no lazy rebase: the accumulators are
// rescaled only in tiles where some row's maximum rises), P rounded to fp16, fp32 accumulation.  Keys at or past
// the length are zeroed when their tile is staged and masked in the scores, so nothing past a length reaches a
// result; pages without a live key are never looked up, and every entry that is loaded is clamped to
// [0, num_pages - 1] before it forms an address.  C and v_d below (576, 512) are uniform loop bounds over 64-channel
// groups of this one instance.
//
// The pool's encoding is a compile-time parameter: over MlaFp8Args the pool holds OCP e4m3fn bytes,
// [num_pages][C][page], and only the staging differs.  A thread stages 16 keys of a channel row as ONE 16-byte load
// (9 loads and 36 registers a tile instead of 18 and 72), clears the bytes at or past the length as integers (so the
// NaN codes 0x7F / 0xFF never reach the conversion), converts with v_cvt_scalef32_pk_f16_fp8 (exact, with the power
// of two 2^e of kv_scale riding in it) and stores the two 16-byte chunks of the SAME swizzled fp16 image; everything
// after the publish barrier is the text above.  K and V are one image, so 2^e multiplies both; the remainder
// r = kv_scale / 2^e goes twice: into the fp32 Q pre-scale (for K) and into the accumulator where the record is
// written (for V).  An invalid scale makes the second factor NaN.
#include "fa_device.h"
#include "fa_fwd_f16_fewq.h"
#include "fa_kernels.h"
#include "fa_mfma.h"

namespace fa {
namespace {

using namespace mf;
using f16core::FewqRecord;

// the pool encoding of a kernel argument type: fp16 halfs (MlaArgs) or e4m3fn bytes with one device scale (MlaFp8Args)
template <class Args>
struct PoolOf {
  static constexpr bool k8 = false;
  static __device__ __forceinline__ const MlaArgs& mla(const Args& a) { return a; }
};
template <>
struct PoolOf<MlaFp8Args> {
  static constexpr bool k8 = true;
  static __device__ __forceinline__ const MlaArgs& mla(const MlaFp8Args& a) { return a.m; }
};

constexpr int kC = 576;                     // most score channels
constexpr int kVd = 512;                    // most value channels
constexpr int kBN = 64;                     // keys per tile
constexpr int kNW = 4;                      // waves per workgroup, one per SIMD
constexpr int kRows = 64;                   // folded rows per workgroup: the record stride
constexpr int kTile = kC * kBN * 2;         // 72 KB
constexpr int kOffX = 2 * kTile;            // the hand-over behind the ring
constexpr int kXWave = 64 * 16 * 4;         // 16 fp32 scores a lane
constexpr int kSmem = kOffX + kNW * kXWave; // 160 KB
constexpr int kCPT = kC * 8 / (kNW * 64);   // 16-byte chunks of a full tile per thread: 18
constexpr int kRowStep = kNW * 64 / 8;      // channel rows between two chunks of a thread: 32
constexpr int kCPT8 = kC * 4 / (kNW * 64);  // FP8: 16-byte loads (16 keys) of a full tile per thread: 9
constexpr int kRowStep8 = kNW * 64 / 4;     // FP8: channel rows between two loads of a thread: 64
static_assert(kCPT % 2 == 0, "staged in two halves");
static_assert(kSmem == 160 * 1024, "the whole LDS of a gfx950 CU");
static_assert(kRows == 64 && kVd % 128 == 0 && kC % 64 == 0, "two 32-row halves; channel groups dealt to two waves");

// the chunk swizzle of channel row c (see above)
__device__ __forceinline__ int swz(int c) { return (((c >> 1) & 1) << 2) | ((c >> 2) & 3); }

template <class Args>
__global__ __launch_bounds__(kNW * 64, 1) void mla_partial_kernel(Args args) {
  constexpr bool k8 = PoolOf<Args>::k8;
  const MlaArgs& ma = PoolOf<Args>::mla(args);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  constexpr float kNegInf = -__builtin_huge_valf();
  const SplitArgs& sa = ma.s;
  const FwdArgs& a = sa.f;

  // ---- this workgroup: (sequence, key chunk, row block), the row blocks of a chunk next to each other (they
  // read the same tiles)
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t per_seq = (uint32_t)(ma.nrb * sa.nchunks);
  const uint32_t seq = bid / per_seq, rem = bid - seq * per_seq;
  const int ch = (int)(rem / (uint32_t)ma.nrb), rb = (int)(rem - (uint32_t)ch * (uint32_t)ma.nrb);
  const int cap = a.rule.k.n, nq = a.rule.q.n, C = a.d, vd = a.v_d, page = ma.page;
  const int len = __builtin_amdgcn_readfirstlane(min(max(ma.k_lens[seq], 0), cap));
  const int kt0 = ch * sa.chunk;
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ntiles = (min(kt0 + sa.chunk, len) - kt0 + kBN - 1) / kBN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rh = w >> 1, cw = w & 1;
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const int ncg = C >> 6;   // 64-channel groups of the scores
  const int nvg = vd >> 6;  // 64-channel groups of the values; this wave owns G = 2 gi + cw < nvg

  // ---- this lane's row: query `qi` of head `head`; the keys it sees are [0, hi]
  const int rho = kRows * rb + 32 * rh + r;
  const int qi = rho & (ma.pitch - 1), head = rho >> ma.log2_pitch;
  const bool live = head < ma.heads && qi < nq;
  const int hi = ma.tail_causal ? min(len - nq + qi, len - 1) : len - 1;

  // ---- Q * softmax_scale * log2(e) as the B operand of S^T = K^T.Q: lane (r, h) holds channels 16 s + 8 h + e
  // (FP8: kv_scale = kmul * rmul, kmul = 2^e in the conversion of the one image, rmul here and in the record)
  float kmul = 1.f, rmul = 1.f, omul = 1.f;
  if constexpr (k8) {
    const f16core::Kv8Mul sc = f16core::kv8_mul(args.kv_scale, nullptr, 0);  // (vmul: 1.0, or NaN for an invalid scale)
    kmul = sc.kmul;
    rmul = sc.qmul;
    omul = __float_as_uint(sc.vmul) == 0x3f800000u ? sc.qmul : sc.vmul;  // r, not kv_scale: 2^e came with the image
  }
  half8 qf[kC / 16];
  {
    const float c2 = k8 ? (float)a.scale * kLog2e * rmul : (float)a.scale * kLog2e;
    const __half* Qr = static_cast<const __half*>(a.Q) + (((int64_t)seq * ma.heads + head) * C) * nq + qi;
    const bool qvec = nq == 1 && (reinterpret_cast<uintptr_t>(a.Q) & 15) == 0;  // a row's channels are contiguous
#pragma unroll
    for (int cg = 0; cg < kC / 64; ++cg)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int s = 4 * cg + s4, c0 = 16 * s + 8 * h;
        u32x4 v = {0, 0, 0, 0};
        if (cg < ncg && live) {
          if (qvec) {
            v = *reinterpret_cast<const u32x4*>(Qr + c0);
          } else {
            uint32_t hh[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) hh[e] = __half_as_ushort(Qr[(int64_t)(c0 + e) * nq]);
            v = u32x4{hh[0] | (hh[1] << 16), hh[2] | (hh[3] << 16), hh[4] | (hh[5] << 16), hh[6] | (hh[7] << 16)};
          }
        }
        qf[s] = scale8(__builtin_bit_cast(half8, v), c2);
      }
  }

  // ---- staging: chunk j of this thread is the 8 keys 8 cm .. 8 cm + 7 of channel row (tid >> 3) + 32 j
  const int cm = tid & 7, crow = tid >> 3, nj = C >> 5;
  const __half* pool = static_cast<const __half*>(a.K);
  const int32_t* trow = ma.block_table + (int64_t)seq * ma.max_pages;
  const int last_live = (int)((uint32_t)(len - 1) / (uint32_t)page);  // the last page with a live key (< max_pages)
  const uint32_t wo0 = (uint32_t)(crow * 128 + 16 * (cm ^ swz(crow)));  // (32 j leaves the swizzle's bits alone)
  // a tile is staged in two halves of 9 chunks a thread
  constexpr int kHalf = kCPT / 2;
  u32x4 stg2[2][kHalf];
  // the global loads of half `hf` of the tile at k0, whose page has the raw table entry `e_raw`
  auto issue = [&](auto hf_, int k0, int e_raw) __attribute__((always_inline)) {
    constexpr int hf = decltype(hf_)::value;
    u32x4 (&stg)[kHalf] = stg2[hf];
    const int entry = __builtin_amdgcn_readfirstlane(min(max(e_raw, 0), ma.last_page));
    const int p = (int)((uint32_t)k0 / (uint32_t)page);
    // (64-bit: a pool of many pages passes 4 GB)
    const __half* src = pool + ((int64_t)entry * C + (crow + hf * kHalf * kRowStep)) * page + (k0 - p * page) + 8 * cm;
    const int64_t step = (int64_t)kRowStep * page;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) {
      if (hf * kHalf + j < nj) stg[j] = *reinterpret_cast<const u32x4*>(src);
      src += step;
    }
  };
  // the LDS stores of the same half into `slot`; in the tile that holds the length the keys at or past it are
  // zeroed, whatever the pool holds there
  auto store = [&](auto hf_, int slot, int k0) __attribute__((always_inline)) {
    constexpr int hf = decltype(hf_)::value;
    u32x4 (&stg)[kHalf] = stg2[hf];
    if (k0 + kBN > len) {
      const int nv = len - k0 - 8 * cm;  // this thread's live keys, of 8
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const uint32_t keep = nv >= 2 * x + 2 ? 0xffffffffu : nv == 2 * x + 1 ? 0x0000ffffu : 0u;
#pragma unroll
        for (int j = 0; j < kHalf; ++j)
          if (hf * kHalf + j < nj) stg[j][x] &= keep;
      }
    }
#pragma unroll
    for (int j = 0; j < kHalf; ++j)
      if (hf * kHalf + j < nj)
        *reinterpret_cast<lds_u32x4_t*>(smem + slot * kTile + wo0 + (hf * kHalf + j) * kRowStep * 128) = stg[j];
  };
  // the raw entry of the page of key k, looked ahead to no further than the last page with a live key
  auto entry_of = [&](int k) __attribute__((always_inline)) {
    return trow[min((int)((uint32_t)k / (uint32_t)page), last_live)];
  };

  // ---- FP8 staging: load j of this thread is the 16 keys 16 cm8 .. 16 cm8 + 15 of channel row crow8 + 64 j, the
  // 16 rows of a wave with bits 1 and 2 of the row number swapped: the four rows of 16 consecutive lanes are then
  // r, r + 1, r + 4, r + 5, whose chunk positions (2 cm8 + b) ^ f(c) for one b are 8 different ones x 2 row parities.
  // (Generic lambdas: the fp16 instance holds none of this, and its machine code is what it was.)
  u32x4 stg8[k8 ? kCPT8 : 1];
  auto lane8 = [&](auto) __attribute__((always_inline)) {
    struct { int cm, crow, nj; } t;
    const int q8 = tid >> 2;
    t.cm = tid & 3;
    t.crow = (q8 & ~6) | ((q8 & 2) << 1) | ((q8 & 4) >> 1);
    t.nj = C >> 6;
    return t;
  };
  auto issue8 = [&](auto tag, int k0, int e_raw) __attribute__((always_inline)) {
    const auto t = lane8(tag);
    const int entry = __builtin_amdgcn_readfirstlane(min(max(e_raw, 0), ma.last_page));
    const int p = (int)((uint32_t)k0 / (uint32_t)page);
    const uint8_t* src = static_cast<const uint8_t*>(a.K) + ((int64_t)entry * C + t.crow) * page + (k0 - p * page) + 16 * t.cm;
    const int64_t step = (int64_t)kRowStep8 * page;
#pragma unroll
    for (int j = 0; j < kCPT8; ++j) {
      if (j < t.nj) stg8[j] = *reinterpret_cast<const u32x4*>(src);
      src += step;
    }
  };
  // in the tile that holds the length the BYTES at or past it become 0x00 (+0.0) before anything converts them
  auto store8 = [&](auto tag, int slot, int k0) __attribute__((always_inline)) {
    const auto t = lane8(tag);
    if (k0 + kBN > len) {
      const int nv = len - k0 - 16 * t.cm;  // this thread's live keys, of 16
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int k = nv - 4 * x;  // live bytes of word x
        const uint32_t keep = k >= 4 ? 0xffffffffu : k <= 0 ? 0u : (1u << (8 * (k & 3))) - 1u;
#pragma unroll
        for (int j = 0; j < kCPT8; ++j)
          if (j < t.nj) stg8[j][x] &= keep;
      }
    }
    lds_char_t* row = smem + slot * kTile + t.crow * 128;  // (64 j leaves the swizzle's bits alone)
    const int x0 = 16 * ((2 * t.cm) ^ swz(t.crow)), x1 = 16 * ((2 * t.cm + 1) ^ swz(t.crow));
#pragma unroll
    for (int j = 0; j < kCPT8; ++j)
      if (j < t.nj) {
        *reinterpret_cast<lds_u32x4_t*>(row + x0) = f16core::chunk_f16(u32x2{stg8[j][0], stg8[j][1]}, kmul);
        *reinterpret_cast<lds_u32x4_t*>(row + x1) = f16core::chunk_f16(u32x2{stg8[j][2], stg8[j][3]}, kmul);
        row += kRowStep8 * 128;
      }
  };

  // ---- fragment read bases (lane constants)
  // K, transposed: rows 16 s + 8 h + 4 e + tq, the 8 bytes of keys 32 cw + 16 (g & 1) + 4 sig .. + 3, so that
  // register i of S^T holds key 32 cw + 16 (i >> 3) + 8 h + (i & 7): P is the B operand of PV as it stands
  const int sig = ((tp & 1) << 1) | (tp >> 1);
  uint32_t kb[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int cr = 8 * h + 4 * e + tq;
    kb[e] = (uint32_t)(cr * 128 + 16 * ((4 * cw + 2 * (g & 1) + (sig >> 1)) ^ swz(cr)) + 8 * (sig & 1));
  }
  // V, row-wise: row 64 G + 32 uu + r, keys 16 s + 8 h .. + 7 (chunk 2 s + h); local k-step sl = 0, 1 are this
  // wave's own 32 keys (s = 2 cw + sl), sl = 2, 3 the other wave's (s = 2 (cw ^ 1) + sl - 2)
  uint32_t vb[4];
#pragma unroll
  for (int sl = 0; sl < 4; ++sl) {
    const int s = 2 * (sl < 2 ? cw : cw ^ 1) + (sl & 1);
    vb[sl] = (uint32_t)(r * 128 + 16 * ((2 * s + h) ^ swz(r)));
  }

  floatx16 o[kVd / 64];  // O^T of group G = 2 gi + cw, half uu: o[2 gi + uu], channel 64 G + 32 uu + 8 (i >> 2) + 4 h + (i & 3)
#pragma unroll
  for (int u = 0; u < kVd / 64; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[u][i] = 0.f;
  float m_run = kNegInf, l_run = 0.f;

  // ---- prologue: tile 0 into slot 0
  int e_next = entry_of(kt0);
  if constexpr (k8) {
    issue8(IC<0>{}, kt0, e_next);
    store8(IC<0>{}, 0, kt0);
  } else {
    issue(IC<0>{}, kt0, e_next);
    store(IC<0>{}, 0, kt0);
    issue(IC<1>{}, kt0, e_next);
    store(IC<1>{}, 0, kt0);
  }
  e_next = entry_of(kt0 + kBN);
  __syncthreads();

  lds_char_t* xw = smem + kOffX + w * kXWave + lane * 16;
  const lds_char_t* xr = smem + kOffX + (w ^ 1) * kXWave + lane * 16;

  for (int it = 0; it < ntiles; ++it) {
    const int k0 = kt0 + it * kBN, slot = it & 1;
    const bool more = it + 1 < ntiles;
    if (more) {  // the whole next tile in flight for the whole of this one
      if constexpr (k8) {
        issue8(IC<0>{}, k0 + kBN, e_next);
      } else {
        issue(IC<0>{}, k0 + kBN, e_next);
        issue(IC<1>{}, k0 + kBN, e_next);
      }
      e_next = entry_of(k0 + 2 * kBN);
    }

    // ---- S^T of this wave's 32 keys.  With one wave per SIMD nothing else hides an LDS round trip, so the
    // fragments of channel group cg + 1 are read before the MFMAs of group cg (the last group reads itself again);
    // two accumulators, so that consecutive MFMAs do not depend on each other
    floatx16 sm, so;
    {
      const lds_char_t* kp = smem + slot * kTile;
      auto kread = [&](half8 (&f)[4], int off) __attribute__((always_inline)) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          f[s4].lo = tr_read(kp + kb[0] + off + s4 * 16 * 128);
          f[s4].hi = tr_read(kp + kb[1] + off + s4 * 16 * 128);
        }
      };
      half8 kf[2][4];
      kread(kf[0], 0);
      floatx16 s0 = {}, s1 = {};
#pragma unroll
      for (int cg = 0; cg < kC / 64; ++cg)
        if (cg < ncg) {
          kread(kf[(cg + 1) & 1], min(cg + 1, ncg - 1) * 64 * 128);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            if (s4 & 1) s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[cg & 1][s4], qf[4 * cg + s4], s1, 0, 0, 0);
            else s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[cg & 1][s4], qf[4 * cg + s4], s0, 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      sm = s0 + s1;
    }
    // ---- hand-over: this wave's scores out, the other wave's in
#pragma unroll
    for (int x = 0; x < 4; ++x)
      *reinterpret_cast<lds_f4_t*>(xw + x * 1024) = floatx4{sm[4 * x], sm[4 * x + 1], sm[4 * x + 2], sm[4 * x + 3]};
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const floatx4 t = *reinterpret_cast<const lds_f4_t*>(xr + x * 1024);
#pragma unroll
      for (int j = 0; j < 4; ++j) so[4 * x + j] = t[j];
    }

    // ---- softmax over the 64 keys (both waves of a row pair compute the same values)
    if (!__all(k0 + kBN - 1 <= hi)) {
      const int bm = k0 + 32 * cw + 8 * h, bo = k0 + 32 * (cw ^ 1) + 8 * h;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int off = 16 * (i >> 3) + (i & 7);
        sm[i] = bm + off <= hi ? sm[i] : kNegInf;
        so[i] = bo + off <= hi ? so[i] : kNegInf;
      }
    }
    float mx = fmaxf(sm[0], so[0]);
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, fmaxf(sm[i], so[i]));
    const float m_new = fmaxf(m_run, max_pair32(mx));
    if (__any(m_new > m_run)) {
      const float alpha = m_new > m_run ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.f;  // (0 from -inf: O and l are 0)
      l_run *= alpha;
#pragma unroll
      for (int u = 0; u < kVd / 64; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[u][i] *= alpha;
      m_run = m_new;
    }
    const float mref = m_run == kNegInf ? 0.f : m_run;  // a row without a key so far: P = exp2(-inf) = 0
    uint32_t pm[8], po[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const half2v a2 = {(_Float16)__builtin_amdgcn_exp2f(sm[2 * x] - mref), (_Float16)__builtin_amdgcn_exp2f(sm[2 * x + 1] - mref)};
      const half2v b2 = {(_Float16)__builtin_amdgcn_exp2f(so[2 * x] - mref), (_Float16)__builtin_amdgcn_exp2f(so[2 * x + 1] - mref)};
      l_run += ((float)a2[0] + (float)a2[1]) + ((float)b2[0] + (float)b2[1]);  // the sum of the ROUNDED P
      pm[x] = __builtin_bit_cast(uint32_t, a2);
      po[x] = __builtin_bit_cast(uint32_t, b2);
    }

    // ---- O^T += V.P^T for this wave's channel groups, the fragments of the next 32 channels read before the
    // MFMAs of these (the last block reads itself again)
    {
      const lds_char_t* vp = smem + slot * kTile;
      auto vread = [&](half8 (&f)[4], int row0) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) f[sl] = read_b128(vp + vb[sl] + row0 * 128);
      };
      half8 vf[2][4];
      vread(vf[0], 64 * cw);  // (v_d >= 64: wave 1 may own no group, and then reads rows nobody uses)
#pragma unroll
      for (int gi = 0; gi < kVd / 128; ++gi)
        if (2 * gi + cw < nvg) {
#pragma unroll
          for (int uu = 0; uu < 2; ++uu) {
            const int row0 = 64 * (2 * gi + cw) + 32 * uu;
            vread(vf[uu ^ 1], uu == 0 ? row0 + 32 : 2 * gi + 2 + cw < nvg ? row0 + 96 : row0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
              const uint32_t* pw = sl < 2 ? pm : po;
              const int x0 = 4 * (sl & 1);
              const half8 pp = __builtin_bit_cast(half8, u32x4{pw[x0], pw[x0 + 1], pw[x0 + 2], pw[x0 + 3]});
              o[2 * gi + uu] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[uu][sl], pp, o[2 * gi + uu], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
    }

    if (more) {
      if constexpr (k8) {
        store8(IC<0>{}, slot ^ 1, k0 + kBN);
      } else {
        store(IC<0>{}, slot ^ 1, k0 + kBN);
        store(IC<1>{}, slot ^ 1, k0 + kBN);
      }
    }
    __syncthreads();
  }

  // ---- the record of (sequence, row block, chunk): all 64 rows (the dead ones hold finite values nobody reads)
  const float l_tot = l_run + xor32(l_run);
  const FewqRecord rc = {vd, kRows};
  float* rec = sa.ws + (((int64_t)seq * ma.nrb + rb) * sa.nchunks + ch) * rc.floats();
  const int row = 32 * rh + r;
#pragma unroll
  for (int gi = 0; gi < kVd / 128; ++gi)
    if (2 * gi + cw < nvg) {
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int v = 64 * (2 * gi + cw) + 32 * uu + 8 * (i >> 2) + 4 * h + (i & 3);
          rec[rc.chan(v, row)] = k8 ? o[2 * gi + uu][i] * omul : o[2 * gi + uu][i];
        }
    }
  if (cw == 0 && h == 0) {  // (the two waves of a row pair hold the same statistics)
    rec[rc.stat(FewqRecord::kMRun, row)] = m_run;  // -inf = kEmpty for a row without a key in the chunk
    rec[rc.stat(FewqRecord::kL, row)] = l_tot;
    rec[rc.stat(FewqRecord::kMMax, row)] = m_run;  // the reference IS the exact maximum
  }
}

// one thread per (sequence, output channel, head, query), the queries fastest: folds the live chunks
// [0, ceil(len / chunk)) of its row in chunk order; len = 0 writes the empty row
__global__ __launch_bounds__(256) void mla_merge_kernel(MlaArgs ma) {
  const SplitArgs& sa = ma.s;
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n, hn = ma.heads * nq;
  const int64_t per = (int64_t)a.v_d * hn;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t seq = gid / per;
  const int rem = (int)(gid - seq * per);
  const int v = rem / hn, t = rem - v * hn, head = t / nq, q = t - head * nq;
  const int len = min(max(ma.k_lens[seq], 0), a.rule.k.n);
  const int nc = min(sa.nchunks, (len + sa.chunk - 1) / sa.chunk);
  const int rho = head * ma.pitch + q;
  f16core::merge_row(sa, kRows, seq * ma.nrb + rho / kRows, rho % kRows, v, nc, seq * ma.heads + head, q);
}

}  // namespace

// the partial kernel of the pool's encoding over `args`, then the merge over its MlaArgs
template <class Args>
static hipError_t launch_mla(const Args& args, const MlaArgs& ma, hipStream_t s) {
  const FwdArgs& a = ma.s.f;
  const hipError_t e = launch_smem(mla_partial_kernel<Args>, (unsigned)(a.b * ma.nrb * ma.s.nchunks), kNW * 64, kSmem, s, args);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * ma.heads * a.rule.q.n;
  hipLaunchKernelGGL(mla_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ma);
  return hipGetLastError();
}

hipError_t launch_fwd_f16_mla(const MlaArgs& ma, hipStream_t s) { return launch_mla(ma, ma, s); }
hipError_t launch_fwd_f16_mla_fp8(const MlaFp8Args& ma8, hipStream_t s) { return launch_mla(ma8, ma8.m, s); }

}  // namespace fa
