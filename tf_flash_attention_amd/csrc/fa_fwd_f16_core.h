// fa_fwd_f16_core.h — the per-workgroup key loop of the general fp16 forward (gfx950 MFMA).
//
// fwd_f16_core runs one workgroup's share of a (batch, head) slice: 32*NW query rows from q0
// against the key tiles [kt0, kt0 + 64*ntiles), from the prologue loads through the last
// ring step, and hands back each wave's unnormalised accumulator and softmax statistics
// (WaveState).  Six
// kernel templates wrap it and differ only in which block gets which rows and keys and in the epilogue:
//   * fwd_f16_kernel (fa_fwd_f16.hip): block -> (slice, query block), the rule-bounded key
//     range of that block, normalises and writes O, l, m;
//   * splitk_partial_kernel (fa_fwd_f16_splitk.hip): block -> (slice, key chunk) of the single
//     query block, writes the partial and its statistics to the workspace;
//   * gqa_partial_kernel (fa_fwd_f16_gqa.hip): block -> (K/V slice, key chunk) with the query heads that
//     share the K/V slice folded into the block's rows (FoldedRows below), the same partial format;
//   * decode_partial_kernel (fa_fwd_f16_decode.hip) over the four K/V caches of fa_fwd_f16_decode.h: the same
//     block with a per-slice key length read on the device (RaggedCache: the row maps' key_limit / lane_interval
//     below); with each key tile read from a page pool through a device block table (PagedCache: the row maps'
//     tile below); and the two over a K/V cache of e4m3fn bytes, converted to fp16 on the way into LDS
//     (RaggedCache8, PagedCache8: KvOf below);
//   * window_partial_kernel and prefill_partial_kernel (fa_fwd_f16_window.h / .hip, fa_fwd_f16_prefill.h / .hip):
//     the same four caches again, with a lower interval end, and over one block of a longer query axis (a map
//     with kQBlock below);
//   * tree_partial_kernel (fa_fwd_f16_tree.h / .hip): the four caches once more, the last nq keys seen through a
//     device bit mask (a map with kTree: HasTree below).
// The partial kernels share what surrounds the core, and their merge, in fa_fwd_f16_fewq.h.
// The structure:
//   * Sᵀ = Kᵀ·Q and Oᵀ = V·Pᵀ on v_mfma_f32_32x32x16_f16 with fp32 accumulation.
//     Computing the TRANSPOSED scores puts the key index in the MFMA rows, so
//     (a) each lane owns one query column — the softmax row reductions are
//     in-register plus one cross-half exchange, and (b) the Sᵀ accumulator
//     is already the B operand of Oᵀ = V·Pᵀ (no LDS round trip for P), and
//     Oᵀ[v][q] comes out channel-first exactly as O is stored in HBM;
//   * the channel-first [c][n] tiles of Q and K are staged in LDS as stored
//     and read as k-contiguous MFMA operands with ds_read_b64_tr_b16
//     (hardware transpose); V goes to LDS as [key/4][v][4] slabs so its
//     operand reads are plain conflict-free ds_read_b64;
//   * masks are rules: per (wave, key tile) the tile is classified from the
//     order bounds (none / all / mixed) and only mixed tiles evaluate the
//     per-element rule (fa_rules.h).
// Online softmax in the log2 domain (exp2 on v_exp_f32), fp32 statistics.
// The order of every floating-point max and sum chain here is part of the library's
// bit-exact behaviour (the split-key path must reproduce the general one tile for tile).
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CORE_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CORE_H_

#include "fa_device.h"
#include "fa_fwd_f16_choice.h"
#include "fa_kernels.h"
#include "fa_mfma.h"

namespace fa {
namespace f16core {

using namespace mf;

constexpr int kBN = 64;      // keys per tile
constexpr int kVPad = 2;     // V slab row padding, in 8-byte rows

// Structure flags (FA_FWD_VARIANT overrides the default for A/B timing runs)
constexpr int kFOcc3 = 4;        // ask for 3 waves/SIMD (VGPR <= 168)
constexpr int kFDot2 = 8;        // row sums of the fp16 P by v_dot2_f32_f16 (half the VALU ops)
constexpr int kFOcc1 = 16;       // one wave per SIMD: the whole 512-entry register file
constexpr int kFSched = 32;      // force a 1-MFMA/5-VALU interleave (sched_group_barrier)
// row sums on the matrix pipe: one more MFMA per PV k-step with an all-ones A operand (every row of
// its accumulator is the query's running sum), instead of v_dot2c on the VALU.  At d <= 32 a tile's
// 8 MFMAs leave the pipe idle two thirds of the time beside the softmax issue, so the 4 extra
// MFMAs are free and the 16 dot2c they replace are not
constexpr int kFMfmaSum = 64;

template <int D, int NW>
struct Smem {
  static constexpr int kBM = 32 * NW;               // query rows per workgroup
  static constexpr int kQRow = 2 * kBM;              // bytes per Q row
  static constexpr int kQ = D * kQRow;               // Q [D][BM] halfs
  static constexpr int kK = D * kBN * 2;             // K [D][64]  halfs, 128-B rows
  static constexpr int kV = 16 * (D + kVPad) * 8;    // V [16][D+pad][4] halfs
  static constexpr int kBuf = kK + kV;
  static constexpr int kNBuf = 3;                    // K/V ring: tile t (V), t+1 (K), t+2 (being written)
  static constexpr int kTotal = (kNBuf * kBuf > kQ) ? kNBuf * kBuf : kQ;  // Q aliases the ring
};

constexpr int waves_per_eu(int D, int F) { return (D >= 128 || (F & kFOcc1)) ? 1 : ((F & kFOcc3) ? 3 : 2); }

// one staging chunk, 8 keys of one channel row: 16 bytes of fp16, or 8 bytes of an 8-bit cache (below)
__device__ __forceinline__ u32x4 load_chunk(const __half* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x2 load_chunk(const uint8_t* p) { return *reinterpret_cast<const u32x2*>(p); }

// the first n of a chunk's 8 halfs, zeros behind them (integer masks: a NaN bit pattern is cleared like any other)
__device__ __forceinline__ u32x4 keep_first(u32x4 v, int n) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] &= (2 * i < n ? 0xffffu : 0u) | (2 * i + 1 < n ? 0xffff0000u : 0u);
  return v;
}
// the same of a chunk's 8 bytes: byte 0 is +0.0 in e4m3fn, and the NaN codes 0x7F / 0xFF are cleared like any other
__device__ __forceinline__ u32x2 keep_first(u32x2 v, int n) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k = n - 4 * i;  // bytes of this word that are kept
    v[i] &= k >= 4 ? 0xffffffffu : k <= 0 ? 0u : (1u << (8 * k)) - 1u;
  }
  return v;
}
// The element format of K / V.  fp16 unless the row map says kKv8 (fa_fwd_f16_decode.h: the FP8 caches): then
// K and V are OCP e4m3fn bytes in the same layouts, a staged chunk is its 8 raw bytes (half the staging registers),
// and store_from converts it to the fp16 LDS image that the key loop reads, so nothing after the staging knows.
// The conversion is exact (v_cvt_scalef32_pk_f16_fp8: every e4m3fn value times a power of two 2^e, -8 <= e <= 7,
// is an fp16 value: |x| <= 448 * 128 < 65504, and the smallest subnormal 2^-9 becomes 2^-17 >= 2^-24).  Such a map
// also carries the scales: kmul = 2^e multiplies K in that conversion, qmul multiplies the Q pre-scale in fp32
// (k_scale = kmul * qmul), and vmul multiplies the accumulator where fewq_partial writes it (fa_fwd_f16_fewq.h).
template <class Map, class = void>
struct KvOf {
  static constexpr bool k8 = false;
  using Elem = __half;
  using Reg = u32x4;
};
template <class Map>
struct KvOf<Map, typename std::enable_if<Map::kKv8>::type> {
  static constexpr bool k8 = true;
  using Elem = uint8_t;
  using Reg = u32x2;
};
__device__ __forceinline__ u32x4 chunk_f16(u32x4 v, float) { return v; }
__device__ __forceinline__ u32x4 chunk_f16(u32x2 v, float mul) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = __builtin_bit_cast(uint32_t, i & 1 ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[i >> 1], mul, true)
                                               : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v[i >> 1], mul, false));
  return o;
}

// Whether the map's rule is a device bit mask over the last nq keys (fa_fwd_f16_tree.h: a map with kTree), which no
// index interval expresses.  Such a map runs at POL 0 and is asked three more things: load_mask(qi), once per lane
// before the key loop, for the row of the lane's query; its `base`, below which every key is seen (the tile class);
// and allowed(k0), the 64 keys of a class-1 tile that the lane's query sees, as bits.  The other maps compile as
// they did without it.
template <class Map, class = void>
struct HasTree {
  static constexpr bool on = false;
};
template <class Map>
struct HasTree<Map, typename std::enable_if<Map::kTree>::type> {
  static constexpr bool on = true;
};

// The loop's register arrays.  The KERNEL declares them (and the WaveState below) and hands them
// in: the compiler optimises fwd_f16_core as a function of its own before it inlines it, without
// the kernel's launch bounds, and arrays that are locals of that function are then cut up under
// a smaller register budget than the kernel's (measured: 16 more AGPRs and 0.8 % slower at
// D = 128).  Arrays that belong to the kernel are promoted there, under its bounds.
template <int D, int NW, class KvReg = u32x4>
struct WaveRegs {
  static constexpr int kCPT = (D * 8 + NW * 64 - 1) / (NW * 64);  // 8-key K (or V) chunks per thread and tile
  KvReg kreg[kCPT], vreg[kCPT], kreg1[kCPT], vreg1[kCPT];        // staged K / V tiles (KvOf<Map>::Reg)
  half8 qf[D / 16];                                               // scaled Q fragments
  floatx16 stA[2], stB[2], negm;                                  // scores of two tiles in flight; -m_run
};

// Row maps: which query each of the workgroup's 32*NW rows is.
//   IdentityRows: row rho of the block at q0 is query q0 + rho of slice `bi`, which is also the K/V slice
//     (every ungrouped kernel).
//   FoldedRows (grouped-query attention, fa_fwd_f16_gqa.hip): the `g` query slices bkv*g .. bkv*g + g-1
//     that share K/V slice `bkv` are folded into the rows of ONE block (q0 = 0): row rho is query
//     i = rho % pitch of head j = rho / pitch, pitch the smallest power of two >= nq (g * pitch <= 32*NW).
//     A row is live iff j < g and i < nq; the other rows stage zeros and are never written out.  A
//     pitch <= 32 divides the wave's 32 rows, so a wave holds whole heads and its rule bounds are those of
//     the queries [0, nq-1]; a larger pitch gives a wave a contiguous run of one head's queries.
// The core asks the map, in the order of the ungrouped code: the first Q slice and the K/V slice; wave w's
// first query; whether the wave holds a live row; lane r's query; its row of the block.
// The map also says how many of a slice's keys are live and which of them a query may see: key_limit(nk)
// bounds the staging guards, the whole-tile path, the tile class and the tail mask, while nk itself stays
// the row stride of K and V; lane_interval is the POL 1 interval of query qi.  These two maps answer nk and
// the rule's own interval.  A map with kRagged (fa_fwd_f16_decode.h) answers a per-slice length below nk,
// and the core then zeroes staged K / V past it element by element: what lies there is not the caller's
// data, and a NaN or Inf times P = 0 would poison the PV product.
// Last, where a key tile lies: for a tile-aligned k0, the K and V pointers of channel row 0 at key k0 and the row
// stride there.  For these maps and RaggedRows (kPaged false) that is K + k0, V + k0 and nk, the contiguous slice,
// and load_into keeps indexing the slice's rows from key 0 as it always has: a hook that had every map hand back
// K + k0, V + k0 and nk moved the register allocation of 72 of the 75 existing kernels
// (profiles/paged_core_asm_equal.txt).  A map with kPaged (fa_fwd_f16_decode.h) is asked, tile(K, V, k0, ...):
// it looks the tile's page up in a block table and answers a pointer into a page pool with the page as the
// stride; a page is a multiple of the 64-key tile, so a tile never straddles two pages.
// A map with kQBlock (fa_fwd_f16_prefill.h) folds one BLOCK of a longer query axis: it carries the block's first
// query q0 and its query count nq, and the core then starts Q q0 elements in, keeps a.rule.q.n as Q's row stride
// only, and counts the live rows and each wave's last lane by the block's nq.  For every other map the three are
// one number, as they always were.
// The core asks none of the next two; the few-query partial and merge kernels (fa_fwd_f16_fewq.h) do: whether
// row rho of the block is a live query (row_live), and the floats per row of a partial record (rec_stride).
struct IdentityRows {
  static constexpr bool kFolded = false;
  static constexpr bool kRagged = false;
  static constexpr bool kPaged = false;
  static constexpr bool kQBlock = false;
  __device__ __forceinline__ int key_limit(int nk) const { return nk; }
  __device__ __forceinline__ void lane_interval(const Rule& r, int qi, int* klo, int* khi) const { key_interval(r, qi, klo, khi); }
  __device__ __forceinline__ int64_t q_slice(int64_t bi, int64_t) const { return bi; }
  __device__ __forceinline__ int64_t kv_slice(int64_t bi, int64_t) const { return bi; }
  __device__ __forceinline__ int wave_q0(int q0, int w) const { return q0 + 32 * w; }
  __device__ __forceinline__ bool wave_active(int wq0, int, int nq) const { return wq0 < nq; }
  __device__ __forceinline__ int lane_q(int wq0, int, int r) const { return wq0 + r; }
  __device__ __forceinline__ int lane_row(int qi, int, int) const { return qi; }
  __device__ __forceinline__ bool row_live(int row, int nq) const { return row < nq; }
  __device__ __forceinline__ int rec_stride(int nq) const { return nq; }
};
struct FoldedRows {
  static constexpr bool kFolded = true;
  static constexpr bool kRagged = false;
  static constexpr bool kPaged = false;
  static constexpr bool kQBlock = false;
  __device__ __forceinline__ int key_limit(int nk) const { return nk; }
  __device__ __forceinline__ void lane_interval(const Rule& r, int qi, int* klo, int* khi) const { key_interval(r, qi, klo, khi); }
  int32_t g, pitch, log2_pitch;
  __device__ __forceinline__ int64_t q_slice(int64_t, int64_t bkv) const { return bkv * g; }
  __device__ __forceinline__ int64_t kv_slice(int64_t, int64_t bkv) const { return bkv; }
  // 0 for a pitch <= 32: the wave holds whole heads, so its queries are [0, nq-1]
  __device__ __forceinline__ int wave_q0(int, int w) const { return (32 * w) & (pitch - 1); }
  __device__ __forceinline__ bool wave_active(int wq0, int w, int nq) const { return 32 * w < g * pitch && wq0 < nq; }
  __device__ __forceinline__ int lane_q(int, int w, int r) const { return (32 * w + r) & (pitch - 1); }
  __device__ __forceinline__ int lane_row(int, int w, int r) const { return 32 * w + r; }
  __device__ __forceinline__ bool row_live(int rho, int nq) const { return rho < g * pitch && (rho & (pitch - 1)) < nq; }
  __device__ __forceinline__ int rec_stride(int) const { return g * pitch; }
};

// What a wave holds after its last key tile.  acc_o and the row sum are relative to m_run, the
// lazily updated softmax reference (log2 units; meaningful once m_set); m_max is the exact row max.
// The row sum is l_run in each half-wave (add lane l^32), or with kFMfmaSum every element of acc_l.
template <int D>
struct WaveState {
  floatx16 acc_o[D / 32];
  floatx16 acc_l;    // kFMfmaSum: the running row sum in every register (rows are identical)
  float m_run, l_run, m_max;
  bool m_set;
  bool wave_active;  // the wave's first query row wq0 < nq (FoldedRows: the wave holds a live row)
  int qi, h;         // this lane's query row (FoldedRows: its row rho of the block); its half-wave
                     // (channel v = 32u + (i&3) + 8(i>>2) + 4h)
};

// One workgroup = NW waves = 32*NW query rows [q0, q0 + 32*NW) of slice `bi`, against the key
// tiles [kt0, kt0 + 64*ntiles) (kt0 a multiple of 64).  `smem` is Smem<D, NW>::kTotal bytes;
// `rg` is scratch, `ws` the result.
//   POL  0: full policy (no rule mask; only the nk tail is masked)
//        1: interval rules (causal, 1d unit-stride local): each query's allowed keys
//           are an index interval [klo, khi]; the tile class is two scalar compares
//           against the wave's bounds and the mixed-tile mask one unsigned compare
//        2: other local rules (2d, strided): tile_class + per-element rule check
//   Tiles with no allowed pair for a wave are skipped by that wave (no MFMAs).
//   FAST d == v_d == D and K/V rows 16-byte aligned (nk % 8 == 0): unguarded
//        dwordx4 staging (an 8-bit cache: rows 8-byte aligned, dwordx2).
//   Map  the row map above; with FoldedRows `bi` is unused, `bkv` is the K/V slice and the queries are
//        those of slices bkv*g + j.  With IdentityRows `bkv` is unused: slice `bi` serves Q, K and V.
// All waves stage K/V whatever nq is; waves whose 32 query rows lie past nq run no MFMA.
// Scores are produced directly as exp2 arguments: Q is pre-scaled by
// scale*log2(e) once (fp16), and the running max enters each Sᵀ MFMA chain as
// its C operand (-m broadcast), so P = exp2(acc) needs no per-element FMA.
// Software pipeline (one barrier per key tile, 3-slot LDS ring): while the
// softmax of tile j runs on the VALU, the Sᵀ MFMAs of tile j+1 are already in
// the matrix pipe, and the PV MFMAs of tile j follow (cdna_hip_programming.md
// T15); the K/V tile j+2 is written to LDS after the barrier and tile j+3 is
// loaded into registers (T14).
template <int D, int NW, int POL, bool FAST, int F, class Map = IdentityRows>
__device__ __forceinline__ void fwd_f16_core(const FwdArgs& a, lds_char_t* smem, int64_t bi, int q0, int kt0, int ntiles,
                                             WaveRegs<D, NW, typename KvOf<Map>::Reg>& rg, WaveState<D>& ws, Map map = Map{},
                                             int64_t bkv = 0) {
  // (the map travels by value: a reference to the default argument's temporary changed the register
  // allocation of the ungrouped kernels, profiles/gqa_core_asm_equal.txt)
  using S = Smem<D, NW>;
  constexpr int kThr = NW * 64;
  constexpr int kBM = S::kBM;
  constexpr int kChunks = D * 8;                                   // 16-B chunks per K (or V) tile
  constexpr int kCPT = WaveRegs<D, NW>::kCPT;                      // chunks per thread
  using KvT = typename KvOf<Map>::Elem;
  using KvReg = typename KvOf<Map>::Reg;
  constexpr float kNegInf = -__builtin_huge_valf();
  __builtin_assume(kt0 % kBN == 0);  // lets key indices fold as they do where kt0 is formed in place

  // nqs: the row stride of Q.  nq: the queries this workgroup's rows stand for, which every live-row test and wave
  // bound below counts by: the same number, except under a map with kQBlock
  const int nqs = a.rule.q.n;
  int nq_block = nqs;
  if constexpr (Map::kQBlock) nq_block = map.nq;
  const int nq = nq_block, nk = a.rule.k.n, d = FAST ? D : a.d, vd = FAST ? D : a.v_d;
  const int nkl = map.key_limit(nk);  // live keys; nk stays the row stride of K and V
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;  // tr-read lane roles

  const __half* Q = static_cast<const __half*>(a.Q) + map.q_slice(bi, bkv) * (int64_t)d * nqs;
  if constexpr (Map::kQBlock) Q += map.q0;
  const KvT* K = static_cast<const KvT*>(a.K) + map.kv_slice(bi, bkv) * (int64_t)d * nk;
  const KvT* V = static_cast<const KvT*>(a.V) + map.kv_slice(bi, bkv) * (int64_t)vd * nk;
  const bool qvec = ((nq & 7) == 0) && ((reinterpret_cast<uintptr_t>(a.Q) & 15) == 0);
  float c2 = (float)a.scale * kLog2e, kmul = 1.f;
  if constexpr (KvOf<Map>::k8) {  // (qmul == 1 leaves c2's bits alone)
    c2 *= map.qmul;
    kmul = map.kmul;
  }

  // ---- register staging of one K/V tile (16-B chunks; chunk = 8 keys of one channel row)
  auto load_into = [&](KvReg (&kr)[kCPT], KvReg (&vr)[kCPT], int k0) {
    // channel row 0 of the slice, the row stride and the key that index 0 stands for; a paged map moves all three
    // to the tile (for the other maps these are new names for K, V, nk and 0, and the code below is unchanged)
    const KvT *Kt = K, *Vt = V;
    int ts = nk, kb = 0;
    if constexpr (Map::kPaged) {
      map.tile(K, V, k0, &Kt, &Vt, &ts);
      kb = k0;
    }
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      const int idx = tid + kThr * j, c = idx >> 3, m = idx & 7;
      const bool in = (kChunks % kThr == 0) || idx < kChunks;
      const int e = k0 + 8 * m;
      if (FAST && (kChunks % kThr == 0) && k0 + kBN <= nkl) {  // whole tile in range: unguarded
        kr[j] = load_chunk(Kt + (int64_t)c * ts + (e - kb));
        vr[j] = load_chunk(Vt + (int64_t)c * ts + (e - kb));
      } else if (FAST) {
        kr[j] = (in && e < nkl) ? load_chunk(Kt + (int64_t)c * ts + (e - kb)) : KvReg{};
        vr[j] = (in && e < nkl) ? load_chunk(Vt + (int64_t)c * ts + (e - kb)) : KvReg{};
        if constexpr (Map::kRagged) {  // a chunk may straddle the length
          kr[j] = keep_first(kr[j], nkl - e);
          vr[j] = keep_first(vr[j], nkl - e);
        }
      } else {
        kr[j] = (in && c < d) ? load_chunk8(Kt + (int64_t)c * ts, e - kb, nkl - kb, false) : KvReg{};
        vr[j] = (in && c < vd) ? load_chunk8(Vt + (int64_t)c * ts, e - kb, nkl - kb, false) : KvReg{};
      }
    }
  };
  auto store_from = [&](const KvReg (&kr)[kCPT], const KvReg (&vr)[kCPT], int buf) {
    lds_char_t* kbuf = smem + buf * S::kBuf;
    lds_char_t* vbuf = kbuf + S::kK;
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      const int idx = tid + kThr * j, c = idx >> 3, m = idx & 7;
      if ((kChunks % kThr == 0) || idx < kChunks) {
        const u32x4 kc = chunk_f16(kr[j], kmul), vc = chunk_f16(vr[j], 1.f);  // (an 8-bit chunk becomes fp16 here)
        // K: [c][64 keys], 64-B halves swapped on rows with c&2 (conflict-free tr reads)
        *reinterpret_cast<lds_u32x4_t*>(kbuf + c * 128 + ((m * 16) ^ ((c & 2) << 5))) = kc;
        // V: [key/4][v][4] slabs -> the PV operand is a plain conflict-free ds_read_b64
        *reinterpret_cast<lds_u32x2_t*>(vbuf + ((2 * m) * (D + kVPad) + c) * 8) = vc.xy;
        *reinterpret_cast<lds_u32x2_t*>(vbuf + ((2 * m + 1) * (D + kVPad) + c) * 8) = vc.zw;
      }
    }
  };
  // prologue loads of tiles 0 and 1 are in flight together with the Q tile
  auto &kreg = rg.kreg, &vreg = rg.vreg, &kreg1 = rg.kreg1, &vreg1 = rg.vreg1;
  if (ntiles > 0) load_into(kreg, vreg, kt0);
  if (ntiles > 1) load_into(kreg1, vreg1, kt0 + kBN);

  // ---- Q tile [D][BM] -> LDS (64-B blocks XOR-swizzled by c&3: conflict-free tr reads)
  for (int idx = tid; idx < D * (kBM / 8); idx += kThr) {
    const int c = idx / (kBM / 8), m = idx % (kBM / 8);
    u32x4 v = {0, 0, 0, 0};
    if constexpr (Map::kFolded) {
      // column rho = 8m + e is query i of head j; below pitch 8 a chunk spans heads, so every element is
      // a guarded load of its own (the tile is loaded once per workgroup, beside >= 128 KB of K/V)
      uint32_t hh[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int rho = 8 * m + e, j = rho >> map.log2_pitch, i = rho & (map.pitch - 1);
        const bool live = c < d && j < map.g && i < nq;
        hh[e] = live ? (uint32_t)__half_as_ushort(Q[((int64_t)j * d + c) * nqs + i]) : 0u;
      }
      v = u32x4{hh[0] | (hh[1] << 16), hh[2] | (hh[3] << 16), hh[4] | (hh[5] << 16), hh[6] | (hh[7] << 16)};
    } else if (c < d) {
      v = load_chunk8(Q + (int64_t)c * nq, q0 + 8 * m, nq, qvec);
    }
    *reinterpret_cast<lds_u32x4_t*>(smem + c * S::kQRow + ((m * 16) ^ ((c & 3) << 6))) = v;
  }
  __syncthreads();
  // Q*scale*log2(e) as the B operand of Sᵀ = Kᵀ·Q: lane (r,h) holds Q[c = 16s + 8h + j][q = 32w + r]
  auto& qf = rg.qf;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int crow = 16 * s + 8 * (g >> 1) + 4 * e + tq;
      const int col = 32 * w + 16 * (g & 1) + 4 * tp;
      const half4 t = tr_read(smem, crow * S::kQRow + ((col * 2) ^ ((crow & 3) << 6)));
      if (e == 0) qf[s].lo = t; else qf[s].hi = t;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[s][j] = (_Float16)((float)qf[s][j] * c2);
  }
  __syncthreads();  // the Q region is reused by the K/V ring

  const int wq0 = map.wave_q0(q0, w);
  const int wq1 = min(wq0 + 31, nq - 1);
  const bool wave_active = map.wave_active(wq0, w, nq);
  const int qi = map.lane_q(wq0, w, r);
  if constexpr (HasTree<Map>::on) map.load_mask(min(qi, nq - 1));  // (padding rows take query nq-1's, as below)
  // (a folded block's padding rows take the rule state of query nq-1, here and in key_interval below)
  const int qo = (POL == 2 && (Map::kFolded || qi < nq)) ? seq_order(a.rule.q, a.rule, Map::kFolded ? min(qi, nq - 1) : qi) : 0;
  // POL 1 (interval rules): this lane's allowed keys [klo, klo + kspan) and the wave's
  // bounds on them (both ends are non-decreasing in the query, so lanes 0 / last bound them)
  int klo = 0, kspan = 0, wlo_min = 0, wlo_max = 0, whi_min = 0, whi_max = 0;
  if (POL == 1 && wave_active) {
    int khi;
    map.lane_interval(a.rule, min(qi, nq - 1), &klo, &khi);
    kspan = max(khi - klo + 1, 0);
    const int last = min(31, nq - 1 - wq0);
    wlo_min = __builtin_amdgcn_readfirstlane(klo);
    whi_min = __builtin_amdgcn_readfirstlane(khi);
    wlo_max = __builtin_amdgcn_readlane(klo, last);
    whi_max = __builtin_amdgcn_readlane(khi, last);
  }
  // tile class for this wave: 0 no allowed pair (skipped), 1 mixed (per-element mask), 2 all
  auto tcls = [&](int k0) -> int {
    const int k1 = k0 + kBN - 1;
    if (!wave_active) return 0;
    if constexpr (HasTree<Map>::on) return k1 < map.base ? 2 : 1;  // (a tile with a draft slot or the key nkl)
    if (POL == 0) return k1 < nkl ? 2 : 1;
    if (POL == 1) {
      if (wlo_min > k1 || whi_max < k0) return 0;
      return (wlo_max <= k0 && whi_min >= k1) ? 2 : 1;
    }
    const int c = tile_class(a.rule, wq0, wq1, k0, min(k1, nkl - 1));
    return (c == 2 && k1 >= nkl) ? 1 : c;
  };

  auto load_tile = [&](int k0) { load_into(kreg, vreg, k0); };
  auto store_tile = [&](int buf) { store_from(kreg, vreg, buf); };

  ws.wave_active = wave_active;
  ws.qi = map.lane_row(qi, w, r);
  ws.h = h;
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) ws.acc_o[u][i] = 0.f;
  ws.m_run = 0.f, ws.l_run = 0.f, ws.m_max = kNegInf;
  ws.m_set = false;
  constexpr bool MSUM = (F & kFMfmaSum) != 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) ws.acc_l[i] = 0.f;
  auto& negm = rg.negm;  // -m_run broadcast: the C operand of every Sᵀ chain
#pragma unroll
  for (int i = 0; i < 16; ++i) negm[i] = 0.f;

  // Sᵀ - m of one tile (both 32-key halves), K fragments streamed from ring slot `buf`
  auto qk = [&](int buf, floatx16 (&st)[2]) {
    const lds_char_t* kbuf = smem + buf * S::kBuf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        half8 kf;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int crow = 16 * s + 8 * (g >> 1) + 4 * e + tq;
          const int col = 32 * t + 16 * (g & 1) + 4 * tp;
          const half4 x = tr_read(kbuf, crow * 128 + ((col * 2) ^ ((crow & 2) << 5)));
          if (e == 0) kf.lo = x; else kf.hi = x;
        }
        st[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], s == 0 ? negm : st[t], 0, 0, 0);
      }
  };

  // Rule/tail mask, row max and (lazy) rebase of the scores of tile `it` (after
  // this, exp2(st) are the tile's probabilities relative to m_run).
  auto prepare = [&](int it, int cls, floatx16 (&st)[2], floatx16 (&nxt)[2], bool has_next) {
    const int k0 = kt0 + it * kBN;
    if constexpr (HasTree<Map>::on) {
      if (cls == 1) {  // a tile with draft slots: one bit of the lane's allowed word per element
        const uint64_t allow = map.allowed(k0) >> (4 * h);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int off = 32 * t + (i & 3) + 8 * (i >> 2);
            st[t][i] = (allow >> off) & 1 ? st[t][i] : kNegInf;
          }
      }
    } else if (cls == 1) {  // mixed / tail tile: per-element mask
      const int base = k0 + 4 * h - klo;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int off = 32 * t + (i & 3) + 8 * (i >> 2);
          bool ok;
          if (POL == 1) {
            ok = (unsigned)(base + off) < (unsigned)kspan;
          } else {
            const int key = k0 + off + 4 * h;
            ok = key < nkl;
            if (POL == 2) ok &= check_orders_bf(a.rule, qo, seq_order(a.rule.k, a.rule, key));
          }
          st[t][i] = ok ? st[t][i] : kNegInf;
        }
    }
    float mt;
    {  // v_max3 chains (2 new values per instruction), two independent chains
      float mx0 = fmaxf(st[0][0], st[0][1]), mx1 = fmaxf(st[1][0], st[1][1]);
#pragma unroll
      for (int i = 2; i < 16; i += 2) {
        mx0 = fmaxf(fmaxf(mx0, st[0][i]), st[0][i + 1]);
        mx1 = fmaxf(fmaxf(mx1, st[1][i]), st[1][i + 1]);
      }
      mt = fmaxf(mx0, mx1);
      mt = fmaxf(mt, xor32(mt));  // tile row max relative to m_run
    }
    ws.m_max = fmaxf(ws.m_max, ws.m_run + mt);
    // lazy rescale (cdna_hip_programming.md T13): move m_run only when the tile max
    // exceeds it by more than kRescaleThr (P <= 2^kRescaleThr), or to seed it
    const bool seed = !ws.m_set && (mt != kNegInf);
    if (__any((mt > kRescaleThr) | seed)) {
      const float delta = ws.m_set ? fmaxf(mt, 0.f) : (seed ? mt : 0.f);
      const float alpha = ws.m_set ? __builtin_amdgcn_exp2f(-delta) : 1.f;
      ws.m_run += delta;
      ws.m_set = ws.m_set || seed;
      ws.l_run *= alpha;
      if constexpr (MSUM) {
#pragma unroll
        for (int i = 0; i < 16; ++i) ws.acc_l[i] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < D / 32; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) ws.acc_o[u][i] *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[0][i] -= delta;
        st[1][i] -= delta;
        negm[i] = -ws.m_run;
      }
      if (has_next) {  // the next tile's in-flight scores were formed against the old m_run
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          nxt[0][i] -= delta;
          nxt[1][i] -= delta;
        }
      }
    }
  };

  // P = exp2(st) (fp16) as the B operand of Oᵀ = V·Pᵀ (k-step s = registers 8(s&1).. of
  // half s>>1), row sums, and the PV MFMAs
  auto exp_pv = [&](floatx16 (&st)[2], int buf) {
    const lds_char_t* vbuf = smem + buf * S::kBuf + S::kK;
    const half2v one2 = {(_Float16)1.f, (_Float16)1.f};
    float ls0 = 0.f, ls1 = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      half8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (_Float16)__builtin_amdgcn_exp2f(st[s >> 1][8 * (s & 1) + j]);
      if constexpr (MSUM) {
        half8 ones;
#pragma unroll
        for (int j = 0; j < 8; ++j) ones[j] = (_Float16)1.f;
        ws.acc_l = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, pf, ws.acc_l, 0, 0, 0);
      } else if (F & kFDot2) {
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
          ls0 = __builtin_amdgcn_fdot2(half2v{pf[j], pf[j + 1]}, one2, ls0, false);
          ls1 = __builtin_amdgcn_fdot2(half2v{pf[j + 2], pf[j + 3]}, one2, ls1, false);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          ls0 += (float)pf[j];
          ls1 += (float)pf[j + 1];
        }
      }
#pragma unroll
      for (int u = 0; u < D / 32; ++u) {
        half8 vf;
        vf.lo = read_b64(vbuf, ((4 * s + h) * (D + kVPad) + 32 * u + r) * 8);
        vf.hi = read_b64(vbuf, ((4 * s + 2 + h) * (D + kVPad) + 32 * u + r) * 8);
        ws.acc_o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, ws.acc_o[u], 0, 0, 0);
      }
    }
    ws.l_run += ls0 + ls1;
  };

  // ---- prologue: tiles 0, 1 in the ring, tile 2 in registers, tile 0 scored
  auto &stA = rg.stA, &stB = rg.stB;
  if (ntiles > 0) {
    store_tile(0);
    if (ntiles > 1) store_from(kreg1, vreg1, 1);
    if (ntiles > 2) load_tile(kt0 + 2 * kBN);
    __syncthreads();
    if (tcls(kt0) != 0) qk(0, stA);
  }
  // iteration it: ring slot it%3 holds tile it (V read now), slot (it+1)%3 tile it+1
  // (K read now), slot (it+2)%3 receives tile it+2.  One branch-free region per
  // iteration interleaves the Sᵀ MFMAs of tile it+1 and the PV MFMAs of tile it
  // with the exp/convert/row-sum VALU of tile it.
  int slot = 0;
  auto step = [&](int it, floatx16 (&cur)[2], floatx16 (&nxt)[2]) {
    const int s1 = (slot == 2) ? 0 : slot + 1;
    const int s2 = (s1 == 2) ? 0 : s1 + 1;
    if (it > 0) __syncthreads();  // tile it+1 complete; slot s2 (tile it-1) free
    if (it + 2 < ntiles) {
      store_tile(s2);
      if (it + 3 < ntiles) load_tile(kt0 + (it + 3) * kBN);
    }
    const int ccur = tcls(kt0 + it * kBN);
    const int cnxt = it + 1 < ntiles ? tcls(kt0 + (it + 1) * kBN) : 0;
    if (cnxt != 0) qk(s1, nxt);   // Sᵀ MFMAs of tile it+1 enter the matrix pipe first
    if (ccur != 0) {              // tiles without an allowed pair for this wave are skipped
      prepare(it, ccur, cur, nxt, cnxt != 0);
      exp_pv(cur, slot);
    }
    if (F & kFSched) {  // MFMA / VALU interleave for the region (cdna_hip_programming.md T19)
#pragma unroll
      for (int i = 0; i < 2 * (D / 16) + 4 * (D / 32); ++i) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x2, 5, 0);   // then up to 5 VALU
      }
    }
    slot = s1;
  };
  for (int it = 0; it < ntiles; it += 2) {
    step(it, stA, stB);
    if (it + 1 < ntiles) step(it + 1, stB, stA);
  }

}

// host: whether these arguments take the FAST staging at channel tile D, where K / V channel rows are `row_keys`
// keys apart: every row then starts 16-byte aligned
// (8 keys' bytes: `chunk_bytes` = 16 of fp16, 8 of an 8-bit cache)
template <int D>
bool fast_staging(const FwdArgs& a, int row_keys, int chunk_bytes = 16) {
  return a.d == D && a.v_d == D && (row_keys % 8 == 0) && (reinterpret_cast<uintptr_t>(a.K) % chunk_bytes == 0) &&
         (reinterpret_cast<uintptr_t>(a.V) % chunk_bytes == 0);
}

// host: the <POL, FAST> instantiation these arguments take at channel tile D.  `launch(pol, fast)`
// receives them as IC<POL> and IC<FAST> (types, so they can be template arguments).
template <class Launch>
hipError_t with_pol_fast(int pol, bool fast, Launch&& launch) {
  return pol == 0 ? (fast ? launch(IC<0>{}, IC<1>{}) : launch(IC<0>{}, IC<0>{}))
       : pol == 1 ? (fast ? launch(IC<1>{}, IC<1>{}) : launch(IC<1>{}, IC<0>{}))
                  : (fast ? launch(IC<2>{}, IC<1>{}) : launch(IC<2>{}, IC<0>{}));
}
template <int D, class Launch>
hipError_t with_pol_fast(const FwdArgs& a, Launch&& launch) {
  return with_pol_fast(fwd_f16_pol(a.rule), fast_staging<D>(a, a.rule.k.n), launch);
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_CORE_H_
