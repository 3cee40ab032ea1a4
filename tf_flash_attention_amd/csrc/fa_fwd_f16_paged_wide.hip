// fa_fwd_f16_paged_wide.hip — the paged few-query forward for heads of more than 128 channels: up to 256 score and
// 256 value channels, several K/V heads, separate K and V pools, GQA folding, tail rule and sliding window
// (gfx950 MFMA).
//
// The shared key loop (fa_fwd_f16_core.h) and its LDS plan end at 128 channels; the MLA kernel (fa_fwd_f16_mla.h)
// reads ONE image two ways because its K and V are the same bytes.  Here they are not: the pools are the paged
// forward's, K [num_pages][Hk][d][page] and V [num_pages][Hk][v_d][page] halfs with the key axis contiguous, so a
// 64-key tile of K is d rows of 128 bytes and one of V is v_d such rows, and each crosses HBM -> LDS once into an
// image of its own: K read transposed (ds_read_b64_tr_b16) as the A operand of S^T = K^T.Q, V read row-wise
// (ds_read_b128) as the A operand of O^T += V.P^T.
//
// The work: the g query heads of a K/V head x P query slots (P the smallest power of two >= nq) are folded into
// R = g * P <= 128 rows, row = head_in_group * P + query (the grouped forward's fold, written out).  One workgroup of
// 4 waves, one per SIMD with the whole register file, takes (K/V slice, block of 64 rows, key chunk of the plan) and
// writes a FewqRecord (fa_fwd_f16_fewq.h) of stride 64; paged_wide_merge_kernel folds the live chunks of a row in
// chunk order with the few-query forwards' merge_row, no atomics.
//
//   wave (rh, cw) = (w >> 1, w & 1) owns rows 32 rh .. 32 rh + 31 and the 64-channel groups G = cw, cw + 2 of O^T.
//   Per 64-key tile it forms S^T for its own 32 keys, 32 cw .. 32 cw + 31, over all d channels (d / 16 MFMAs), hands
//   the fp32 scores to the other wave of its row pair through LDS (4 KB a wave) and takes that wave's; both then run
//   the same softmax over the 64 keys (bit-identical statistics) and each runs the PV MFMAs of its own channel groups
//   (v_d / 32 in all, 2 per group and k-step).  At (256, 256): 16 + 16 v_mfma_f32_32x32x16_f16 per wave and tile.
//
//   registers (512 a wave; MFMA results in VGPRs, Makefile): Q fragments of the 16 k-steps 64, O^T 64, the next
//   tile's 8 + 8 16-byte chunks 64, scores 32, two groups of K or V fragments 32, P 16
//   (profiles/paged_wide_resources.txt: no scratch, no spill).
//   LDS: K ring 2 x 32 KB, V ring 2 x 32 KB (tile i in slot i & 1), hand-over 4 x 4 KB: 144 KB.
//   LDS image of either tile: the MLA image's.  Row c = channel, 128 bytes = 64 keys, the 16-byte chunk x of row c
//   at x ^ f(c), f(c) = bit 1 of c as bit 2 | bits 2..3 of c as bits 0..1 (mla::swz): the four rows of a transposed
//   read fall into four different 32-byte bank groups, and 16 consecutive rows of a b128 read into 8 chunk positions
//   x 2 row parities, so both read modes stay conflict-free in both images.
//   staging: the table entry of tile i + 2 and the global loads of the whole tile i + 1 (K and V) are issued at the
//   head of tile i and stay in flight through it, the LDS stores follow its MFMAs; two barriers a tile (hand-over,
//   publish).  The fragments of an MFMA group are read from LDS one group ahead.
//
// Numerics are the other fp16 forwards': Q pre-scaled by log2(e) / sqrt(d) in fp32 and rounded to fp16 once, scores
// and statistics in fp32 with the exact running maximum as the reference, P rounded to fp16, fp32 accumulation.
// Keys at or past the length are zeroed when their tile is staged and masked in the scores; pages without a live key
// are never looked up, and every entry that is loaded is clamped to [0, num_pages - 1] before it forms an address.
// d and v_d below 256 are uniform loop bounds over 64-channel groups of the one instance.
//
// WINDOW: query i stands at pos = len - nq + i and sees max(0, pos - W + 1) <= j <= pos.  The plan is the un-windowed
// plan over the capacity; with lo_min = max(0, len - nq - W + 1) a workgroup whose chunk has no tile inside
// [lo_min / 64 * 64, len) leaves at once and the merge skips its record by the same arithmetic on the loaded length.
// Tiles below lo_min / 64 * 64 are never staged, and table entries of pages wholly below it never loaded.
#include "fa_device.h"
#include "fa_fwd_f16_fewq.h"
#include "fa_fwd_f16_mla.h"
#include "fa_kernels.h"
#include "fa_mfma.h"

namespace fa {
namespace {

using namespace mf;
using f16core::FewqRecord;
using mla::swz;

constexpr int kWBN = 64;                        // keys per tile
constexpr int kWNW = 4;                         // waves per workgroup, one per SIMD
constexpr int kWRows = 64;                      // folded rows per workgroup: the record stride
constexpr int kWXWave = 64 * 16 * 4;            // hand-over: 16 fp32 scores a lane
constexpr int kWRowStep = kWNW * 64 / 8;        // channel rows between two chunks of a thread: 32

template <int D, int VD>
struct WideLds {
  static constexpr int kKTile = D * kWBN * 2;   // 32 KB at 256
  static constexpr int kVTile = VD * kWBN * 2;
  static constexpr int kOffV = 2 * kKTile;      // the V ring behind the K ring
  static constexpr int kOffX = kOffV + 2 * kVTile;
  static constexpr int kTotal = kOffX + kWNW * kWXWave;
  static constexpr int kKC = D / kWRowStep;     // 16-byte chunks of a full K tile per thread: 8
  static constexpr int kVC = VD / kWRowStep;
};
static_assert(WideLds<256, 256>::kTotal == 144 * 1024, "two rings of two 32 KB tiles and the hand-over");

// the first key a windowed call stages for a slice of `len` keys: the tile of the lowest window start
__device__ __forceinline__ int window_first(int len, int nq, int window) {
  return max(len - nq - window + 1, 0) / kWBN * kWBN;
}

template <int D, int VD, bool WINDOW>
__global__ __launch_bounds__(kWNW * 64, 1) void paged_wide_partial_kernel(PagedWideArgs pa) {
  using L = WideLds<D, VD>;
  static_assert(D % 64 == 0 && VD % 128 == 0, "channel groups of 64, dealt to two waves");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  constexpr float kNegInf = -__builtin_huge_valf();
  const SplitArgs& sa = pa.s;
  const FwdArgs& a = sa.f;

  // ---- this workgroup: (K/V slice, key chunk, row block), the row blocks of a chunk next to each other (they read
  // the same tiles)
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t per_slice = (uint32_t)(pa.nrb * sa.nchunks);
  const uint32_t bkv = bid / per_slice, rem = bid - bkv * per_slice;
  const int ch = (int)(rem / (uint32_t)pa.nrb), rb = (int)(rem - (uint32_t)ch * (uint32_t)pa.nrb);
  const uint32_t seq = bkv / (uint32_t)pa.kv_heads;
  const int hk = (int)(bkv - seq * (uint32_t)pa.kv_heads);
  const int cap = a.rule.k.n, nq = a.rule.q.n, d = a.d, vd = a.v_d, page = pa.page;
  const int len = __builtin_amdgcn_readfirstlane(min(max(pa.k_lens[seq], 0), cap));
  // ---- the chunk's keys: [kbeg, kend), from the window's first tile on
  const int kt0 = ch * sa.chunk;
  const int kbeg = WINDOW ? max(kt0, window_first(len, nq, pa.window)) : kt0;
  const int kend = min(kt0 + sa.chunk, len);
  if (kbeg >= kend) return;  // a dead chunk: the merge does not read its record
  const int ntiles = (kend - kbeg + kWBN - 1) / kWBN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rh = w >> 1, cw = w & 1;
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const int ncg = d >> 6;   // 64-channel groups of the scores
  const int nvg = vd >> 6;  // 64-channel groups of the values; this wave owns G = 2 gi + cw < nvg

  // ---- this lane's row: query `qi` of head `head` of the group; the keys it sees are [lo, hi]
  const int rho = kWRows * rb + 32 * rh + r;
  const int qi = rho & (pa.pitch - 1), head = rho >> pa.log2_pitch;
  const bool live = head < pa.g && qi < nq;
  const int hi = pa.tail_causal ? min(len - nq + qi, len - 1) : len - 1;
  const int lo = WINDOW ? max(len - nq + qi - pa.window + 1, 0) : 0;

  // ---- Q * log2(e) / sqrt(d) as the B operand of S^T = K^T.Q: lane (r, h) holds channels 16 s + 8 h + e
  half8 qf[D / 16];
  {
    const float c2 = (float)a.scale * kLog2e;
    const __half* Qr = static_cast<const __half*>(a.Q) + (((int64_t)bkv * pa.g + head) * d) * nq + qi;
    const bool qvec = nq == 1 && (reinterpret_cast<uintptr_t>(a.Q) & 15) == 0;  // a row's channels are contiguous
#pragma unroll
    for (int cg = 0; cg < D / 64; ++cg)
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

  // ---- staging: chunk j of this thread is the 8 keys 8 cm .. 8 cm + 7 of channel row (tid >> 3) + 32 j, of K and of V
  const int cm = tid & 7, crow = tid >> 3, njk = d >> 5, njv = vd >> 5;
  const __half* kpool = static_cast<const __half*>(a.K);
  const __half* vpool = static_cast<const __half*>(a.V);
  const int32_t* trow = pa.block_table + (int64_t)seq * pa.max_pages;
  const int last_live = (int)((uint32_t)(len - 1) / (uint32_t)page);  // the last page with a live key (< max_pages)
  const uint32_t wo0 = (uint32_t)(crow * 128 + 16 * (cm ^ swz(crow)));  // (32 j leaves the swizzle's bits alone)
  u32x4 stk[L::kKC], stv[L::kVC];
  // the global loads of the tile at k0 of the pool `pool` with `ch_n` channel rows, `nj` chunks of them this thread's;
  // its page has the raw table entry `e_raw`
  auto issue = [&](auto& stg, const __half* pool, int ch_n, int nj, int k0, int e_raw) __attribute__((always_inline)) {
    constexpr int n = sizeof(stg) / sizeof(stg[0]);
    const int entry = __builtin_amdgcn_readfirstlane(min(max(e_raw, 0), pa.last_page));
    const int p = (int)((uint32_t)k0 / (uint32_t)page);
    // (64-bit: a pool of many pages passes 4 GB)
    const __half* src = pool + ((((int64_t)entry * pa.kv_heads + hk) * ch_n) + crow) * page + (k0 - p * page) + 8 * cm;
    const int64_t step = (int64_t)kWRowStep * page;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      if (j < nj) stg[j] = *reinterpret_cast<const u32x4*>(src);
      src += step;
    }
  };
  // the LDS stores of the same chunks into the image at `tile`; in the tile that holds the length the keys at or past
  // it are zeroed, whatever the pool holds there
  auto store = [&](auto& stg, lds_char_t* tile, int nj, int k0) __attribute__((always_inline)) {
    constexpr int n = sizeof(stg) / sizeof(stg[0]);
    if (k0 + kWBN > len) {
      const int nv = len - k0 - 8 * cm;  // this thread's live keys, of 8
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const uint32_t keep = nv >= 2 * x + 2 ? 0xffffffffu : nv == 2 * x + 1 ? 0x0000ffffu : 0u;
#pragma unroll
        for (int j = 0; j < n; ++j)
          if (j < nj) stg[j][x] &= keep;
      }
    }
#pragma unroll
    for (int j = 0; j < n; ++j)
      if (j < nj) *reinterpret_cast<lds_u32x4_t*>(tile + wo0 + j * kWRowStep * 128) = stg[j];
  };
  // both tiles at k0: the loads, and the stores into ring slot `slot`
  auto issue_kv = [&](int k0, int e_raw) __attribute__((always_inline)) {
    issue(stk, kpool, d, njk, k0, e_raw);
    issue(stv, vpool, vd, njv, k0, e_raw);
  };
  auto store_kv = [&](int slot, int k0) __attribute__((always_inline)) {
    store(stk, smem + slot * L::kKTile, njk, k0);
    store(stv, smem + L::kOffV + slot * L::kVTile, njv, k0);
  };
  // the raw entry of the page of key k, looked ahead to no further than the last page with a live key
  auto entry_of = [&](int k) __attribute__((always_inline)) {
    return trow[min((int)((uint32_t)k / (uint32_t)page), last_live)];
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

  floatx16 o[VD / 64];  // O^T of group G = 2 gi + cw, half uu: o[2 gi + uu], channel 64 G + 32 uu + 8 (i >> 2) + 4 h + (i & 3)
#pragma unroll
  for (int u = 0; u < VD / 64; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[u][i] = 0.f;
  float m_run = kNegInf, l_run = 0.f;

  // ---- prologue: tile 0 into slot 0
  int e_next = entry_of(kbeg);
  issue_kv(kbeg, e_next);
  store_kv(0, kbeg);
  e_next = entry_of(kbeg + kWBN);
  __syncthreads();

  lds_char_t* xw = smem + L::kOffX + w * kWXWave + lane * 16;
  const lds_char_t* xr = smem + L::kOffX + (w ^ 1) * kWXWave + lane * 16;

  for (int it = 0; it < ntiles; ++it) {
    const int k0 = kbeg + it * kWBN, slot = it & 1;
    const bool more = it + 1 < ntiles;
    if (more) {  // the whole next tile in flight for the whole of this one
      issue_kv(k0 + kWBN, e_next);
      e_next = entry_of(k0 + 2 * kWBN);
    }

    // ---- S^T of this wave's 32 keys: the fragments of channel group cg + 1 are read before the MFMAs of group cg
    // (the last group reads itself again); two accumulators, so that consecutive MFMAs do not depend on each other
    floatx16 sm, so;
    {
      const lds_char_t* kp = smem + slot * L::kKTile;
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
      for (int cg = 0; cg < D / 64; ++cg)
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
    if (!__all(k0 + kWBN - 1 <= hi && (!WINDOW || k0 >= lo))) {
      const int bm = k0 + 32 * cw + 8 * h, bo = k0 + 32 * (cw ^ 1) + 8 * h;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int off = 16 * (i >> 3) + (i & 7);
        sm[i] = bm + off <= hi && (!WINDOW || bm + off >= lo) ? sm[i] : kNegInf;
        so[i] = bo + off <= hi && (!WINDOW || bo + off >= lo) ? so[i] : kNegInf;
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
      for (int u = 0; u < VD / 64; ++u)
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
      const lds_char_t* vp = smem + L::kOffV + slot * L::kVTile;
      auto vread = [&](half8 (&f)[4], int row0) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) f[sl] = read_b128(vp + vb[sl] + row0 * 128);
      };
      half8 vf[2][4];
      vread(vf[0], 64 * cw);  // (v_d = 64: wave 1 owns no group, and reads rows of the slot that nobody uses)
#pragma unroll
      for (int gi = 0; gi < VD / 128; ++gi)
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

    if (more) store_kv(slot ^ 1, k0 + kWBN);
    __syncthreads();
  }

  // ---- the record of (K/V slice, row block, chunk): all 64 rows (the dead ones hold finite values nobody reads)
  const float l_tot = l_run + xor32(l_run);
  const FewqRecord rc = {vd, kWRows};
  float* rec = sa.ws + (((int64_t)bkv * pa.nrb + rb) * sa.nchunks + ch) * rc.floats();
  const int row = 32 * rh + r;
#pragma unroll
  for (int gi = 0; gi < VD / 128; ++gi)
    if (2 * gi + cw < nvg) {
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int v = 64 * (2 * gi + cw) + 32 * uu + 8 * (i >> 2) + 4 * h + (i & 3);
          rec[rc.chan(v, row)] = o[2 * gi + uu][i];
        }
    }
  if (cw == 0 && h == 0) {  // (the two waves of a row pair hold the same statistics)
    rec[rc.stat(FewqRecord::kMRun, row)] = m_run;  // -inf = kEmpty for a row without a key in the chunk
    rec[rc.stat(FewqRecord::kL, row)] = l_tot;
    rec[rc.stat(FewqRecord::kMMax, row)] = m_run;  // the reference IS the exact maximum
  }
}

// one thread per (K/V slice, output channel, head of the group, query), the queries fastest: folds the live chunks
// of its row in chunk order, [0, ceil(len / chunk)) or under a window from the chunk of the window's first tile on;
// len = 0 writes the empty row
template <bool WINDOW>
__global__ __launch_bounds__(256) void paged_wide_merge_kernel(PagedWideArgs pa) {
  const FwdArgs& a = pa.s.f;
  int64_t bkv;
  int v, j, q;
  if (!f16core::merge_thread(a, pa.g, &bkv, &v, &j, &q)) return;
  const int nq = a.rule.q.n;
  const int len = min(max(pa.k_lens[bkv / pa.kv_heads], 0), a.rule.k.n);
  const int c_end = min(pa.s.nchunks, (len + pa.s.chunk - 1) / pa.s.chunk);
  const int c_lo = WINDOW ? min(window_first(len, nq, pa.window) / pa.s.chunk, c_end) : 0;
  const int rho = j * pa.pitch + q;
  SplitArgs sa = pa.s;
  sa.ws += c_lo * fewq_record_floats(a.v_d, kWRows);  // (the records of a row block's chunks are contiguous)
  f16core::merge_row(sa, kWRows, bkv * pa.nrb + rho / kWRows, rho % kWRows, v, c_end - c_lo, bkv * pa.g + j, q);
}

template <bool WINDOW>
hipError_t launch_wide(const PagedWideArgs& pa, hipStream_t s) {
  const FwdArgs& a = pa.s.f;
  const hipError_t e = launch_smem(paged_wide_partial_kernel<256, 256, WINDOW>, (unsigned)(a.b * pa.nrb * pa.s.nchunks),
                                   kWNW * 64, WideLds<256, 256>::kTotal, s, pa);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * pa.g * a.rule.q.n;
  hipLaunchKernelGGL(paged_wide_merge_kernel<WINDOW>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, pa);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fwd_f16_paged_wide(const PagedWideArgs& pa, hipStream_t s) {
  return pa.window > 0 ? launch_wide<true>(pa, s) : launch_wide<false>(pa, s);
}

}  // namespace fa
