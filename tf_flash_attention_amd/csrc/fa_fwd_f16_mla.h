// fa_fwd_f16_mla.h — the partial kernel of the MLA forwards over a paged latent cache (gfx950 MFMA):
// mla_partial_kernel, whose instances are decode (fa_fwd_f16_mla.hip: the design, the LDS image, the staging, the
// numerics) and its query-blocked and tree-masked forms (fa_fwd_f16_mla_prefill.hip; 3.22).
//
// A form is named by the kernel's argument type (PoolOf) and differs from decode in four places, each a compile-time
// branch here so that the decode instances carry none of it: which row block of which query block a workgroup is,
// which (head, query) a lane's row is, where the block's keys end, and the mask words of the draft tiles.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_MLA_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_MLA_H_

#include "fa_device.h"
#include "fa_fwd_f16_fewq.h"
#include "fa_kernels.h"
#include "fa_mfma.h"

namespace fa {
namespace mla {

using namespace mf;
using f16core::FewqRecord;

// the query-blocked arguments `A` with the draft mask applied (a.mask is not null): a type, so that the mask is a
// compile-time variant of the one kernel template
template <class A>
struct MaskedOf {
  A a;
};

// a kernel argument type names the pool's encoding, fp16 halfs or e4m3fn bytes with one device scale (k8), and the
// form: decode (MlaArgs, MlaFp8Args), query blocks (kBlocked: MlaPrefillArgs, MlaPrefillFp8Args) or query blocks
// under the draft mask (kMask: MaskedOf of the two)
template <class Args>
struct PoolOf {
  static constexpr bool k8 = false, kBlocked = false, kMask = false;
  static __device__ __forceinline__ const MlaArgs& mla(const Args& a) { return a; }
};
template <>
struct PoolOf<MlaFp8Args> {
  static constexpr bool k8 = true, kBlocked = false, kMask = false;
  static __device__ __forceinline__ const MlaArgs& mla(const MlaFp8Args& a) { return a.m; }
  static __device__ __forceinline__ const float* scale(const MlaFp8Args& a) { return a.kv_scale; }
};
template <>
struct PoolOf<MlaPrefillArgs> {
  static constexpr bool k8 = false, kBlocked = true, kMask = false;
  static __device__ __forceinline__ const MlaArgs& mla(const MlaPrefillArgs& a) { return a.m; }
  static __device__ __forceinline__ const MlaPrefillArgs& form(const MlaPrefillArgs& a) { return a; }
};
template <>
struct PoolOf<MlaPrefillFp8Args> {
  static constexpr bool k8 = true, kBlocked = true, kMask = false;
  static __device__ __forceinline__ const MlaArgs& mla(const MlaPrefillFp8Args& a) { return a.p.m; }
  static __device__ __forceinline__ const MlaPrefillArgs& form(const MlaPrefillFp8Args& a) { return a.p; }
  static __device__ __forceinline__ const float* scale(const MlaPrefillFp8Args& a) { return a.kv_scale; }
};
template <class A>
struct PoolOf<MaskedOf<A>> {
  static constexpr bool k8 = PoolOf<A>::k8, kBlocked = true, kMask = true;
  static __device__ __forceinline__ const MlaArgs& mla(const MaskedOf<A>& x) { return PoolOf<A>::mla(x.a); }
  static __device__ __forceinline__ const MlaPrefillArgs& form(const MaskedOf<A>& x) { return PoolOf<A>::form(x.a); }
  static __device__ __forceinline__ const float* scale(const MaskedOf<A>& x) { return PoolOf<A>::scale(x.a); }
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

// the chunk swizzle of channel row c (fa_fwd_f16_mla.hip: the LDS image of a tile)
__device__ __forceinline__ int swz(int c) { return (((c >> 1) & 1) << 2) | ((c >> 2) & 3); }

// The three mask words of row `mrow` (nw words) that cover the 64 + 31 draft slots from slot 32 w0 on, slots below 0
// (the keys in front of the drafts) reading as ones and slots past the row's words as zeros; w0 >= -2.
struct MaskWords {
  uint32_t w[3];
  // the bits of slots [32 w0 + p, 32 w0 + p + 8) in bits 0..7, 0 <= p <= 88
  __device__ __forceinline__ uint32_t bits8(int p) const {
    const uint64_t lo = p < 32 ? w[0] : p < 64 ? w[1] : w[2], hi = p < 32 ? w[1] : p < 64 ? w[2] : 0u;
    return (uint32_t)((lo | (hi << 32)) >> (p & 31)) & 0xffu;
  }
};
__device__ __forceinline__ MaskWords mask_words(const uint32_t* mrow, int nw, int w0) {
  MaskWords mw;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const int wi = w0 + x;
    const uint32_t v = mrow[min(max(wi, 0), nw - 1)];  // (always a word of the row)
    mw.w[x] = wi < 0 ? 0xffffffffu : wi < nw ? v : 0u;
  }
  return mw;
}

}  // namespace mla

namespace {

using namespace mla;

// The partial kernel of every form.  (The kernel itself lives in this header, in the including unit's own unnamed
// namespace: as an inlined function under a kernel of each unit the decode instances compile to other code.)
template <class Args>
__global__ __launch_bounds__(kNW * 64, 1) void mla_partial_kernel(Args args) {
  constexpr bool k8 = PoolOf<Args>::k8, kBlocked = PoolOf<Args>::kBlocked, MASK = PoolOf<Args>::kMask;
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
  // ---- where this block's keys end.  Decode: at the length.  Query blocks: block rb holds the P = pitch queries
  // from qb * P on of the 64 / P heads from hb * (64 / P) on, rb = qb * nhb + hb; under the tail rule without a
  // mask no row of it sees a key at or past the position after its last query's
  [[maybe_unused]] int qb = 0, hb = 0;
  if constexpr (kBlocked) {
    const int nhb = PoolOf<Args>::form(args).nhb;
    qb = (int)((uint32_t)rb / (uint32_t)nhb);
    hb = rb - qb * nhb;
  }
  const int end = kBlocked && !MASK && ma.tail_causal ? min(max(len - nq + min((qb + 1) * ma.pitch, nq), 0), len) : len;
  if (kt0 >= end) return;  // a dead chunk: the merge does not read its record
  const int ntiles = (min(kt0 + sa.chunk, end) - kt0 + kBN - 1) / kBN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rh = w >> 1, cw = w & 1;
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const int ncg = C >> 6;   // 64-channel groups of the scores
  const int nvg = vd >> 6;  // 64-channel groups of the values; this wave owns G = 2 gi + cw < nvg

  // ---- this lane's row: query `qi` of head `head`; the keys it sees are [0, hi]
  // (query blocks: the block's own 64 rows, folded the same way over its heads and its queries)
  const int rho = kRows * (kBlocked ? hb : rb) + 32 * rh + r;
  const int qi = kBlocked ? qb * ma.pitch + (rho & (ma.pitch - 1)) : rho & (ma.pitch - 1), head = rho >> ma.log2_pitch;
  const bool live = head < ma.heads && qi < nq;
  // (with a mask the tail rule is the mask's to state: the length alone bounds a row here)
  const int hi = !MASK && ma.tail_causal ? min(len - nq + qi, len - 1) : len - 1;

  // ---- Q * softmax_scale * log2(e) as the B operand of S^T = K^T.Q: lane (r, h) holds channels 16 s + 8 h + e
  // (FP8: kv_scale = kmul * rmul, kmul = 2^e in the conversion of the one image, rmul here and in the record)
  float kmul = 1.f, rmul = 1.f, omul = 1.f;
  if constexpr (k8) {
    const f16core::Kv8Mul sc = f16core::kv8_mul(PoolOf<Args>::scale(args), nullptr, 0);  // (vmul: 1.0, or NaN for an invalid scale)
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
    if constexpr (MASK) {
      // the tiles that overlap the draft slots [len - nq, len): a lane takes the three words of its row that hold
      // the tile's slots, and a score stays if its key is below the length and its slot's bit is set (a key in
      // front of the drafts has a slot below 0: a one).  The tiles in front of them lie below the length whole.
      const int p0 = k0 - (len - nq);  // the slot of the tile's first key, < nq
      if (p0 + kBN > 0) {
        const int nw = (nq + 31) >> 5, w0 = p0 >> 5;
        const uint32_t* mrow = PoolOf<Args>::form(args).mask + ((int64_t)seq * nq + min(qi, nq - 1)) * nw;
        const MaskWords mw = mask_words(mrow, nw, w0);
        const int pm0 = p0 - 32 * w0 + 32 * cw + 8 * h, po0 = p0 - 32 * w0 + 32 * (cw ^ 1) + 8 * h;
        const uint32_t vm = mw.bits8(pm0) | (mw.bits8(pm0 + 16) << 8), vo = mw.bits8(po0) | (mw.bits8(po0 + 16) << 8);
        const int bm = k0 + 32 * cw + 8 * h, bo = k0 + 32 * (cw ^ 1) + 8 * h;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int off = 16 * (i >> 3) + (i & 7);
          sm[i] = bm + off <= hi && ((vm >> i) & 1) ? sm[i] : kNegInf;
          so[i] = bo + off <= hi && ((vo >> i) & 1) ? so[i] : kNegInf;
        }
      }
    } else if (!__all(k0 + kBN - 1 <= hi)) {
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

}  // namespace
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_MLA_H_
