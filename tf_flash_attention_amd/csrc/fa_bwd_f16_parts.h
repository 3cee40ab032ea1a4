// fa_bwd_f16_parts.h — what the fp16 two-pass backward kernels share (fa_bwd_f16_fast.hip: prep, dK/dV;
// fa_bwd_f16_dq.hip: dQ; fa_bwd_f16_wide.hip: D = 256; diag/fa_bwd_f16_k64.hip): the LDS image offsets, the
// resident prologue, the tile stager, the per-wave interval ends and tile classes, the masked exp2, the
// gradient epilogue, two reads of the four-role kernels and the host-side kernel pick and launch.
// profiles/bwd_f16_parts_streams.txt says which parts left the instruction streams as they were and which
// were checked by bits and time instead.
#ifndef TF_FLASH_ATTENTION_AMD_FA_BWD_F16_PARTS_H_
#define TF_FLASH_ATTENTION_AMD_FA_BWD_F16_PARTS_H_

#include <type_traits>

#include "fa_device.h"
#include "fa_kernels.h"
#include "fa_mfma.h"
#include "fa_rules.h"

namespace fa {
namespace bwdp {

using namespace mf;

// ---------------------------------------------------------------------------
// LDS images
// "Q16 image" [D][32] fp16, 64-B rows, 16-B units XOR-swizzled by (row >> 2) & 3: one ds_write_b128
// per staged chunk; conflict-free transposed reads (rows q = 0..3 of a 4-row block fill the four
// 64-B quarters of the bank window) and conflict-free b128 row reads (16 lanes = 16 rows).
// Byte offset of the 8-B half `half8` of unit u (8 queries 8u..8u+7) of row `row`.
__device__ __forceinline__ uint32_t q16_off(int row, int u, int half8 = 0) {
  return row * 64 + 16 * (u ^ ((row >> 2) & 3)) + 8 * half8;
}
// "K2 image" [D][64] fp16, 128-B rows, 16-B chunk j at position j ^ (4·bit1(row) + bits2..3(row)):
// conflict-free for the σ-permuted transposed reads (a 4-row block's rows 0/2 and 1/3 land in
// opposite 64-B halves) AND for b128 row reads (16 consecutive rows hit 16 distinct 16-B slots),
// so one image serves as Kᵀ (Sᵀ = Kᵀ·Q') and as K (dQ += K·dSᵀ).
__device__ __forceinline__ uint32_t k2_off(int row, int j, int half8 = 0) {
  return row * 128 + 16 * (j ^ (4 * ((row >> 1) & 1) + ((row >> 2) & 3))) + 8 * half8;
}

// ---------------------------------------------------------------------------
// Tile class of a wave's 32 rows against one tile of the other sequence.  0: no allowed pair for this
// wave, 1: mixed (per-element mask), 2: all allowed.  The members are references to the kernel's own values
// (wlo / whi: the interval ends of the wave's first and last active lane, POL 1), held as the [&] lambdas
// these replace held them and in their capture order, with plain inline call operators: hipcc simplifies
// a helper on its own before it inlines it, and only this shape keeps the kernels' instruction streams.
// A reorder of the members renumbers SGPRs silently: compare the streams with tools/asm_equal.py after a change.
// key-outer: keys wk0 .. wk0 + 31 against queries qa .. qa + 31
template <int POL>
struct KeyWaveClass {
  const bool& wave_active;
  const int& nq;
  const Rule& rule;
  const int &wk0, &nk, &wlo_min, &whi_max, &wlo_max, &whi_min;
  __device__ int operator()(int qa) const {
    const int qz = qa + 31;
    if (!wave_active) return 0;
    if (POL == 0) return 2;  // q >= nq rows carry -lse2 = -inf -> P = 0; keys >= nk are never stored
    if (POL == 2) return qa < nq ? tile_class(rule, qa, min(qz, nq - 1), wk0, min(wk0 + 31, nk - 1)) : 0;
    if (wlo_min > qz || whi_max < qa) return 0;
    return (wlo_max <= qa && whi_min >= qz) ? 2 : 1;
  }
};
// query-outer: queries wq0 .. wq0 + 31 against keys ka .. ka + kBN - 1.  The staged tail past nk is masked
// per element, so a tile is class 2 only wholly inside nk (POL 0 too: its tail tile is class 1)
template <int POL, int kBN>
struct QueryWaveClass {
  const bool& wave_active;
  const int& nk;
  const Rule& rule;
  const int &wq0, &nq, &wlo_min, &whi_max, &wlo_max, &whi_min;
  __device__ int operator()(int ka) const {
    const int kz = ka + kBN - 1;
    if (!wave_active) return 0;
    if (POL == 0) return kz < nk ? 2 : 1;
    if (POL == 2) {
      if (ka >= nk) return 0;
      const int c = tile_class(rule, wq0, min(wq0 + 31, nq - 1), ka, min(kz, nk - 1));
      return (c == 2 && kz >= nk) ? 1 : c;
    }
    if (wlo_min > kz || whi_max < ka) return 0;
    return (wlo_max <= ka && whi_min >= kz && kz < nk) ? 2 : 1;
  }
};

// ---------------------------------------------------------------------------
// "row image" [D][W] fp16, W = 32 per wave slice, 16-B chunks XOR-swizzled by (row & 3) << 6 (B-operand
// transposed reads conflict-free; the forward's Q tile).  Byte offset of column byte cb of row c.
template <int W>
__device__ __forceinline__ uint32_t row_off(int c, int cb) {
  return c * (2 * W) + (cb ^ ((c & 3) << 6));
}
// Resident-operand prologue of the one-wave and producer / consumer kernels (these change the kernels'
// instruction streams in operand order and register names; bits and time were checked instead,
// profiles/bwd_f16_parts_timing.txt).  The [D][W] blocks (columns x0 .. x0 + W - 1) of the tensors
// A [da][n] and B [db][n] into the row images at smem and smem + D·W·2: every chunk of a thread loaded
// before any is stored, branch-free (chunks past the channel count or n read as zeros): a rolled
// load-store loop serialised 2D/16 memory latencies in every block's prologue.  The caller places the barriers.
template <int D, int W, int kThr, bool ALN>
__device__ __forceinline__ void stage_resident(lds_char_t* smem, const __half* A, const __half* B, int da, int db, int n,
                                               int x0, int tid) {
  constexpr int kRPT = 2 * D * (W / 8) / kThr, kHalf = D * (W / 8) / kThr;
  static_assert(kHalf * kThr == D * (W / 8), "resident chunks must divide over the workgroup");
  const __amdgpu_buffer_rsrc_t ars = make_rsrc(A, 2u * da * n), brs = make_rsrc(B, 2u * db * n);
  u32x4 rv[kRPT];
#pragma unroll
  for (int jj = 0; jj < kRPT; ++jj) {
    const int which = jj >= kHalf, j = tid + kThr * (jj - which * kHalf);
    const int c = j / (W / 8), m = j % (W / 8);
    const bool in = c < (which ? db : da) && x0 + 8 * m < n;
    if constexpr (ALN)
      rv[jj] = __builtin_amdgcn_raw_buffer_load_b128(which ? brs : ars,
                                                     in ? (uint32_t)c * (uint32_t)n * 2u + 16u * m : 0x80000000u, 2 * x0, 0);
    else
      rv[jj] = buf_load8h(which ? brs : ars, (uint32_t)c * (uint32_t)n * 2u, x0 + 8 * m, n, c < (which ? db : da));
  }
#pragma unroll
  for (int jj = 0; jj < kRPT; ++jj) {
    const int which = jj >= kHalf, j = tid + kThr * (jj - which * kHalf);
    const int c = j / (W / 8), m = j % (W / 8);
    *reinterpret_cast<lds_u32x4_t*>(smem + which * (D * W * 2) + row_off<W>(c, m * 16)) = rv[jj];
  }
}
// Wave slice w's resident B operand back from the row image img: lane (r, h) holds X[c = 16s + 8h + j][32w + r]
// (g, tq, tp: the lane's 16-lane group, row and column of the transposed read)
template <int D, int W>
__device__ __forceinline__ void read_resident(const lds_char_t* img, int w, int g, int tq, int tp, half8 (&x)[D / 16]) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int crow = 16 * s + 8 * (g >> 1) + 4 * e + tq;
      const half4 v = tr_read(img + row_off<W>(crow, (32 * w + 16 * (g & 1) + 4 * tp) * 2));
      if (e == 0) x[s].lo = v; else x[s].hi = v;
    }
}

// Tile stager of the one-wave and producer / consumer kernels: a [D][8·CPR] tile of two tensors A [da][n] and
// B [db][n] (8·CPR columns from x0) through registers into two LDS images, 16-B chunks (8 columns of one
// channel row) dealt over kThr staging threads, thread t of them.  CPR = 4: Q16 images (key-outer: Q, dO),
// CPR = 8: K2 images (query-outer: K, V).  A chunk past n or past the channel count is loaded as zeros (ALN:
// vector offset 0x80000000, out of range of any buffer here with or without the scalar offset 2·x0, so x0
// needs no clamp on phantom tiles).  The staging registers belong to the caller (one or two sets).
template <int D, int kThr, int CPR, bool ALN>
struct TileStager {
  static constexpr int kChunks = D * CPR;           // 16-B chunks of one tile
  static constexpr int kCPT = 2 * kChunks / kThr;   // A and B chunks per thread
  static_assert((2 * kChunks) % kThr == 0, "tile chunks must divide over the staging threads");
  uint32_t voff[kCPT];  // byte offset in the tensor (ALN: the chunk's; else the row's)
  int crow[kCPT], cm, t;
  __device__ __forceinline__ TileStager(int t_, int n) : cm(t_ % CPR), t(t_) {
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      crow[j] = ((t + kThr * j) % kChunks) / CPR;
      voff[j] = (uint32_t)crow[j] * (uint32_t)n * 2u + (ALN ? 16u * cm : 0u);
    }
  }
  // chunk j holds B (else A); compile-time when the chunks divide evenly over the threads
  __device__ __forceinline__ bool second(int j) const {
    return (kChunks % kThr == 0) ? (j >= kChunks / kThr) : ((t + kThr * j) >= kChunks);
  }
  __device__ __forceinline__ void load(u32x4 (&x)[kCPT], __amdgpu_buffer_rsrc_t ars, __amdgpu_buffer_rsrc_t brs, int da,
                                       int db, int x0, int n) const {
    const bool out = x0 + 8 * cm >= n;
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      const bool isB = second(j);
      if constexpr (ALN)
        x[j] = buf_load16(isB ? brs : ars, voff[j], 2 * x0, out || crow[j] >= (isB ? db : da));
      else
        x[j] = buf_load8h(isB ? brs : ars, voff[j], x0 + 8 * cm, n, crow[j] < (isB ? db : da));
    }
  }
  __device__ __forceinline__ void store(lds_char_t* imgA, lds_char_t* imgB, const u32x4 (&x)[kCPT]) const {
#pragma unroll
    for (int j = 0; j < kCPT; ++j)
      *reinterpret_cast<lds_u32x4_t*>((second(j) ? imgB : imgA) + (CPR == 4 ? q16_off(crow[j], cm) : k2_off(crow[j], cm))) =
          x[j];
  }
};

// Masked exp2: P of one score of an edge or interior tile (masked: the tile's class is 1).
// key-outer: accumulator register i = query qa + 16(i>>3) + 8h + (i&7) against this lane's key (its allowed
// queries [qlo, qlo + qspan) under POL 1, its order ko under POL 2; POL 0 needs no mask: see KeyWaveClass)
template <int POL>
__device__ __forceinline__ float masked_exp2_q(float s, bool masked, int i, int qa, int h, int qlo, int qspan, int nq,
                                               const Rule& rule, int ko) {
  float pv = __builtin_amdgcn_exp2f(s);
  if (POL == 1 && masked) {
    const int q = qa + 16 * (i >> 3) + 8 * h + (i & 7);
    pv = ((unsigned)(q - qlo) < (unsigned)qspan) ? pv : 0.f;
  }
  if (POL == 2 && masked) {
    const int q = qa + 16 * (i >> 3) + 8 * h + (i & 7);
    pv = (q < nq && check_orders_bf(rule, seq_order(rule.q, rule, min(q, nq - 1)), ko)) ? pv : 0.f;
  }
  return pv;
}
// query-outer: register i = key ka + 16(i>>3) + 8h + (i&7) against this lane's query (POL 0 masks the tail past nk)
template <int POL>
__device__ __forceinline__ float masked_exp2_k(float s, bool masked, int i, int ka, int h, int klo, int kspan, int nk,
                                               const Rule& rule, int qo) {
  float pv = __builtin_amdgcn_exp2f(s);
  if (masked) {
    const int kk = ka + 16 * (i >> 3) + 8 * h + (i & 7);
    const bool ok = (POL == 1)   ? ((unsigned)(kk - klo) < (unsigned)kspan)
                    : (POL == 2) ? (kk < nk && check_orders_bf(rule, qo, seq_order(rule.k, rule, min(kk, nk - 1))))
                                 : (kk < nk);
    pv = ok ? pv : 0.f;
  }
  return pv;
}

// The wave's view of its lanes' allowed intervals [lo, hi] (POL 1; monotone along the lanes): the ends of
// the first lane and of the last active lane `last`, as scalars for the tile classes above
__device__ __forceinline__ void wave_interval_ends(int lo, int hi, int last, int& wlo_min, int& whi_min, int& wlo_max,
                                                   int& whi_max) {
  wlo_min = __builtin_amdgcn_readfirstlane(lo);
  whi_min = __builtin_amdgcn_readfirstlane(hi);
  wlo_max = __builtin_amdgcn_readlane(lo, last);
  whi_max = __builtin_amdgcn_readlane(hi, last);
}
// Gradient epilogue.  One gradient of a wave's 32-column slice: acc[u][i]·sc goes to
// X[32(u0 + u) + (i&3) + 8(i>>2) + 4h][col] of the tensor X [ch][n] (the MFMA accumulator layout of lane
// (r, h); col = the lane's key or query)
template <int kU>
struct GradOut {
  const floatx16 (&acc)[kU];
  __half* X;
  int ch;
  float sc;
};
// All N gradients of the slice.  Every tensor with all D channels: one buffer store per value, the row's
// offset in an SGPR (no per-store 64-bit address, compare or exec branch); else guarded stores.
template <int D, int kU, int N>
__device__ __forceinline__ void store_grad(const GradOut<kU> (&g)[N], int n, int col, int h, int u0) {
  bool whole = true;
#pragma unroll
  for (int k = 0; k < N; ++k) whole = whole && g[k].ch == D;
  if (whole) {
    __amdgpu_buffer_rsrc_t rs[N];
#pragma unroll
    for (int k = 0; k < N; ++k) rs[k] = make_rsrc(g[k].X, 2u * g[k].ch * n);
    const uint32_t vlane = 2u * ((uint32_t)(4 * h) * (uint32_t)n + (uint32_t)col);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t so = 2u * (32u * (u0 + u) + (i & 3) + 8u * (i >> 2)) * (uint32_t)n;
#pragma unroll
        for (int k = 0; k < N; ++k)
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (_Float16)(g[k].acc[u][i] * g[k].sc)), rs[k],
                                                vlane, so, 0);
      }
    return;
  }
#pragma unroll
  for (int u = 0; u < kU; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = 32 * (u0 + u) + (i & 3) + 8 * (i >> 2) + 4 * h;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (c < g[k].ch) g[k].X[(int64_t)c * n + col] = __float2half(g[k].acc[u][i] * g[k].sc);
    }
}

// ---------------------------------------------------------------------------
// Pieces of the four-role kernels (references in capture order, as above).
// A wave's resident B operand back from the plain-row image `which` of [D][W] images at smem:
// lane (r, h) holds X[c = 16s + 8h + j][32·sl + r]
template <int D, int W>
struct ResidentRead {
  const int &g, &tq, &sl, &tp;
  lds_char_t* const& smem;
  __device__ __attribute__((always_inline)) void operator()(int which, half8 (&xb)[D / 16]) const {
#pragma unroll
    for (int s_ = 0; s_ < D / 16; ++s_)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int crow = 16 * s_ + 8 * (g >> 1) + 4 * e + tq;
        const int col = 32 * sl + 16 * (g & 1) + 4 * tp;
        const half4 x = tr_read(smem + which * (D * W * 2) + crow * (2 * W) + col * 2);
        if (e == 0) xb[s_].lo = x; else xb[s_].hi = x;
      }
  }
};
// the A operand of k-step s_ from a Q16 image by transposed reads: rb = the lane's base per half
__device__ __forceinline__ half8 read_op(const lds_char_t* img, const uint32_t (&rb)[2], int s_) {
  half8 x;
  x.lo = tr_read(img + rb[0] + 1024 * s_);
  x.hi = tr_read(img + rb[1] + 1024 * s_);
  return x;
}

// ---------------------------------------------------------------------------
// host side
// kernel POL from the rule: 0 full, 1 interval rules (causal, 1d unit-stride local), 2 any other local rule
inline int bwd_pol(const Rule& r) { return r.policy == 0 ? 0 : rule_is_interval(r) ? 1 : 2; }
// 16-B chunk staging: every tensor 16-B aligned and both lengths multiples of 8 (each channel row starts
// on a 16-B boundary)
inline bool bwd_aligned(const BwdArgs& a) {
  const uintptr_t al = reinterpret_cast<uintptr_t>(a.Q) | reinterpret_cast<uintptr_t>(a.K) |
                       reinterpret_cast<uintptr_t>(a.V) | reinterpret_cast<uintptr_t>(a.dO);
  return (al % 16) == 0 && a.rule.q.n % 8 == 0 && a.rule.k.n % 8 == 0;
}
// the <POL, ALN> instantiation these arguments take: `pick(pol, aln)` receives them as IC<POL> and
// std::bool_constant<ALN> (types, so they can be template arguments) and names the kernel
template <class Pick>
auto with_pol_aln(const BwdArgs& a, Pick&& pick) {
  using T = std::true_type;
  using F = std::false_type;
  const int pol = bwd_pol(a.rule);
  return bwd_aligned(a) ? (pol == 0 ? pick(IC<0>{}, T{}) : pol == 1 ? pick(IC<1>{}, T{}) : pick(IC<2>{}, T{}))
                        : (pol == 0 ? pick(IC<0>{}, F{}) : pol == 1 ? pick(IC<1>{}, F{}) : pick(IC<2>{}, F{}));
}
// (the launch of a picked kernel: launch_smem, fa_device.h)

}  // namespace bwdp

// the passes of launch_bwd_f16_fast / launch_bwd_f16_split (fa_kernels.h) that live in other files
// fa_bwd_f16_dq.hip: the dQ pass for max(d, v_d) <= 128 (variant: FA_BWD_VARIANT in the diagnostic
// library, else -1), and the one-wave pass split over key chunks with its reduce
hipError_t launch_bwd_f16_dq(const BwdArgs& a, hipStream_t s, int variant);
hipError_t launch_bwd_f16_dq_split(const BwdSplitArgs& sa, hipStream_t s);
// fa_bwd_f16_wide.hip: 128 < max(d, v_d) <= 256.  chunked (diagnostic library, FA_BWD_VARIANT=1421): the
// one-wave passes on two 128-channel output chunks, whose kernels stay with their families:
hipError_t launch_bwd_f16_wide(const BwdArgs& a, hipStream_t s, bool chunked);
#ifdef FA_DIAG
hipError_t launch_bwd_f16_dkdv_oc2(const BwdArgs& a, hipStream_t s);  // fa_bwd_f16_fast.hip
hipError_t launch_bwd_f16_dq_oc2(const BwdArgs& a, hipStream_t s);    // fa_bwd_f16_dq.hip
#endif

}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_BWD_F16_PARTS_H_
