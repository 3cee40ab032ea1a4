// fa_bwd_f16_fast.hip — fp16 fused attention backward on gfx950 MFMA for every rule
// (full, causal, local in 1d/2d with any stride) and max(d, v_d) <= 128 (channels
// zero-padded to D ∈ {64, 128}).  Rows whose 16-B chunks are aligned (16-B aligned
// tensors, nq % 8 == nk % 8 == 0) stage with one 16-B buffer load per chunk; any other
// length or alignment (ALN = false) loads the same chunks element by element.
//
// Replaces the reference's BackwardImpl (flash_attention.cu:1079-1967), which ran
// every (key block, query block) pair as scalar SIMT GEMMs and serialised the dQ
// read-modify-write through a global spin lock.  Here the pass is split the way
// the data wants to flow on this chip — no atomics, no locks, no dQ workspace:
//   prep : -D = -rowsum(dO∘O), -lse2 = -(m·log2e + log2 l)            (per query, negated:
//          the C operands of the S / dP chains)
//   dkdv : key-outer.  A wave owns 32 keys; K·scale·log2e and V stay in registers
//          as MFMA B operands, dK and dV accumulate in registers, and the query
//          tiles (Q, dO, lse2, D) stream through a 2-slot LDS ring:
//              S  = Qᵀ·K'  (C = -lse2)   P  = exp2(S)
//              dP = dOᵀ·V  (C = -D)      dS = P∘dP
//              dV += dO·P,  dK += Q·dS   (P, dS straight from the accumulators)
//   dq   : query-outer, the forward's structure.  A wave owns 32 queries; Q' and
//          dO stay in registers as B operands and the key tiles stream through LDS:
//              Sᵀ = Kᵀ·Q' (C = -lse2)    dPᵀ = Vᵀ·dO (C = -D)
//              dQ += K·(Pᵀ∘dPᵀ)
// The dq pass recomputes Sᵀ and dPᵀ (4d of the 14d MFMA FLOPs per allowed pair
// against the algorithmic 10d) in exchange for writing dQ exactly once; a
// single-kernel backward (round 1's, since removed) spends that in fp32 atomics, which
// cap it at ≈ 1.3 TB/s of added bytes (MI355X_MICROARCH.md 'Global float atomics').
// With one query block against a long key range the dq pass would run one workgroup per slice;
// launch_bwd_f16_split runs it on one workgroup per (slice, key chunk) instead (bwd_dq_kernel's SPLIT
// form: fp32 partials) and sums the partials in chunk order (dq_split_reduce_kernel): still no atomics.
// The mirrored shape, one key block (nk <= 128) against a long query range, would run the dkdv pass on one
// workgroup per slice; launch_bwd_f16_qsplit runs it on one workgroup per (slice, query chunk) (the SPLIT
// forms of both dK/dV kernels) and sums their partials the same way (dkdv_split_reduce_kernel).
// Masks are rules (fa_rules.h): per-lane index intervals (POL 1: full windows of an
// interval rule) or the per-element order check (POL 2: strided / 2d local windows), and
// per-wave tile classes; tiles with no allowed pair are skipped.
// This file: the prep, the dK/dV pass (one-wave and producer / consumer kernels) and the dispatch of the
// whole backward.  The dQ pass is fa_bwd_f16_dq.hip, the D = 256 passes (four roles) fa_bwd_f16_wide.hip,
// and fa_bwd_f16_parts.h holds what they share: the image offsets, the resident prologue, the per-wave
// interval ends and tile classes, the gradient epilogue and the kernel pick and launch (the four-role
// kernels and the diagnostic 64-keys-a-wave kernel keep most of theirs written out).
#include "fa_bwd_f16_parts.h"

namespace fa {
namespace {

using namespace bwdp;

constexpr int kThrPrep = 256;

// ---------------------------------------------------------------------------
// prep: -D = -rowsum(dO∘O) (fp32), -lse2 = -(m*log2e + log2(l)) (-inf if the row attends nothing),
// stored negated: both passes start their S / dP accumulator chains from them
__global__ __launch_bounds__(kThrPrep) void bwd_prep_kernel(BwdArgs a) {
  const int nq = a.rule.q.n, vd = a.v_d;
  const int64_t total = a.b * (int64_t)nq;
  const int64_t i = blockIdx.x * (int64_t)kThrPrep + threadIdx.x;
  if (i >= total) return;
  const int64_t bi = i / nq;
  const int q = (int)(i - bi * nq);
  const __half* O = static_cast<const __half*>(a.O) + bi * (int64_t)vd * nq + q;
  const __half* dO = static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq + q;
  float D0 = 0.f, D1 = 0.f;
  int v = 0;
  for (; v + 1 < vd; v += 2) {
    D0 += __half2float(O[(int64_t)v * nq]) * __half2float(dO[(int64_t)v * nq]);
    D1 += __half2float(O[(int64_t)(v + 1) * nq]) * __half2float(dO[(int64_t)(v + 1) * nq]);
  }
  if (v < vd) D0 += __half2float(O[(int64_t)v * nq]) * __half2float(dO[(int64_t)v * nq]);
  const float l = static_cast<const float*>(a.l)[i];
  const float m = __half2float(static_cast<const __half*>(a.m)[i]);
  static_cast<float*>(a.ws_D)[i] = -(D0 + D1);
  static_cast<float*>(a.ws_lse)[i] = (l > 0.f) ? -(m * kLog2e + __log2f(l)) : -__builtin_huge_valf();
}

// the same per query, eight consecutive queries a thread: one 16-B load per channel row and tensor
// instead of eight 2-B ones (O, dO 16-B aligned, nq % 8 == 0; the workspace is the library's own,
// 16-B aligned).  Each query's sums run in the same order as above, so -D and -lse2 are bitwise equal.
__global__ __launch_bounds__(kThrPrep) void bwd_prep8_kernel(BwdArgs a) {
  const int nq = a.rule.q.n, vd = a.v_d;
  const int64_t i0 = 8 * (blockIdx.x * (int64_t)kThrPrep + threadIdx.x);
  if (i0 >= a.b * (int64_t)nq) return;
  const int64_t bi = i0 / nq;
  const int q = (int)(i0 - bi * nq);
  const __half* O = static_cast<const __half*>(a.O) + bi * (int64_t)vd * nq + q;
  const __half* dO = static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq + q;
  float D0[8], D1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) D0[j] = D1[j] = 0.f;
  auto row = [&](const __half* p, int v) __attribute__((always_inline)) {
    return *reinterpret_cast<const half8*>(p + (int64_t)v * nq);
  };
  int v = 0;
#pragma unroll 2
  for (; v + 1 < vd; v += 2) {
    const half8 o0 = row(O, v), g0 = row(dO, v), o1 = row(O, v + 1), g1 = row(dO, v + 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      D0[j] += (float)o0[j] * (float)g0[j];
      D1[j] += (float)o1[j] * (float)g1[j];
    }
  }
  if (v < vd) {
    const half8 o0 = row(O, v), g0 = row(dO, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) D0[j] += (float)o0[j] * (float)g0[j];
  }
  const float* L = static_cast<const float*>(a.l) + i0;
  const __half* M = static_cast<const __half*>(a.m) + i0;
  floatx4 d[2], s[2];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float l = L[j], m = __half2float(M[j]);
    d[j >> 2][j & 3] = -(D0[j] + D1[j]);
    s[j >> 2][j & 3] = (l > 0.f) ? -(m * kLog2e + __log2f(l)) : -__builtin_huge_valf();
  }
  floatx4* wd = reinterpret_cast<floatx4*>(static_cast<float*>(a.ws_D) + i0);
  floatx4* ws = reinterpret_cast<floatx4*>(static_cast<float*>(a.ws_lse) + i0);
  wd[0] = d[0];
  wd[1] = d[1];
  ws[0] = s[0];
  ws[1] = s[1];
}

// SPLIT forms of the two dK/dV kernels (many queries against one key block, BwdQSplitArgs)
template <bool SPLIT> struct DkdvArgsOf { using type = BwdArgs; };
template <> struct DkdvArgsOf<true> { using type = BwdQSplitArgs; };
__device__ __forceinline__ const BwdArgs& dkdv_bwd_args(const BwdArgs& x) { return x; }
__device__ __forceinline__ const BwdArgs& dkdv_bwd_args(const BwdQSplitArgs& x) { return x.b; }

// the unscaled fp32 partial of (slice, chunk) of the split forms, rec = its record [d + v_d][nk] (dK rows,
// then dV rows): lanes along nk, so the stores coalesce; dkdv_split_reduce_kernel scales and rounds
template <int kU>
__device__ __forceinline__ void store_partial(float* rec, const floatx16 (&dk)[kU], const floatx16 (&dv)[kU], int d, int vd,
                                              int nk, int key, int h) {
#pragma unroll
  for (int u = 0; u < kU; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (c < d) rec[(int64_t)c * nk + key] = dk[u][i];
      if (c < vd) rec[(int64_t)(d + c) * nk + key] = dv[u][i];
    }
}

template <int D, int NW, int NS = 2>
struct DkdvSmem {
  static constexpr int kBK = 32 * NW;                 // keys per workgroup
  static constexpr int kRow = D * kBK * 2;            // K (or V) row image
  static constexpr int kQT = D * 64;                  // one [D][32] QT image
  static constexpr int offQT = 0, offOT = kQT, offLse = 2 * kQT;
  static constexpr int kSlot = offLse + 2 * 32 * 4;   // + lse2[32], D[32]
  static constexpr int kRing = NS * kSlot;
  static constexpr int kTotal = (kRing > 2 * kRow) ? kRing : 2 * kRow;  // the K/V images alias the ring
};

// ---------------------------------------------------------------------------
// dK / dV: key-outer.  One workgroup = NW waves x 32 keys of one (batch, head) slice (the d <= 64
// pass, two waves per SIMD; d = 128 runs the producer / consumer pass below).
// OC > 1 (128 < d <= 256): the workgroup accumulates dK / dV for one of OC chunks of D / OC output
// channels (chunk = block index mod OC), forming S and dP over all D channels as before: the 256-channel
// accumulators of both gradients would not fit one wave beside the resident K' and V (round 4's D = 256
// pass; the four-role pass below replaces it, FA_BWD_VARIANT=1421 keeps it for A/B).
// SPLIT (one key block, nk <= 128, against a long query range, BwdQSplitArgs): the grid is (slice, query
// chunk); the workgroup stages the key block (k0 = 0), walks only the query tiles of its chunk of the block's
// query range and stores its unscaled fp32 accumulators as the partial record of (slice, chunk);
// dkdv_split_reduce_kernel sums them.
template <int D, int NW, int WPE, int POL, bool ALN, int OC = 1, bool SPLIT = false>
__global__ __launch_bounds__(NW * 64, WPE) void bwd_dkdv_kernel(typename DkdvArgsOf<SPLIT>::type args) {
  static_assert(!SPLIT || (OC == 1 && NW == 4), "the split form is one 128-key block at D <= 128");
  const BwdArgs& a = dkdv_bwd_args(args);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  using S = DkdvSmem<D, NW>;
  constexpr int kThr = NW * 64;
  constexpr int kBK = S::kBK;
  constexpr int kQChunks = D * 4;                     // 16-B chunks of one [D][32] tile
  static_assert((2 * kQChunks) % kThr == 0, "tile chunks must divide over the workgroup");
  constexpr int kCPT = 2 * kQChunks / kThr;           // Q and dO chunks per thread

  constexpr int kDO = D / OC;                         // output channels of this workgroup
  const int nq = a.rule.q.n, nk = a.rule.k.n;
  const uint32_t nkb = (nk + kBK - 1) / kBK;
  const uint32_t bidc = xcd_remap(blockIdx.x, gridDim.x);
  const int oc = (int)(bidc % OC), ou0 = oc * (kDO / 32);  // the chunk: channel blocks ou0 .. ou0 + kDO/32 - 1
  const uint32_t bid = bidc / OC;
  uint32_t per_slice = nkb;  // SPLIT: one key block (k0 = 0) and the chunks of its query range
  if constexpr (SPLIT) per_slice = (uint32_t)args.nchunks;
  const int64_t bi = bid / per_slice;
  const int k0 = SPLIT ? 0 : (int)(bid % nkb) * kBK;  // earliest (heaviest under causal) key blocks first
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  // transposed reads of the Q16 images supply query columns 4σ(p)..4σ(p)+3 (σ swaps 1 and 2), so
  // register i of S / dP holds query 16(i>>3) + 8h + (i&7): k-step s of P / dS is queries
  // 16s + 8h + 0..7, and the dV / dK A operands are plain 16-B row reads of the same images
  const int sig = ((tp & 1) << 1) | (tp >> 1);
  const float c2 = (float)a.scale * kLog2e;

  // channels d (Q/K) and v_d (V/O) may be smaller than D: rows past them are staged as zeros
  const int d = a.d, vd = a.v_d;
  const __half* K = static_cast<const __half*>(a.K) + bi * (int64_t)d * nk;
  const __half* V = static_cast<const __half*>(a.V) + bi * (int64_t)vd * nk;
  const __amdgpu_buffer_rsrc_t qrs = make_rsrc(static_cast<const __half*>(a.Q) + bi * (int64_t)d * nq, 2u * d * nq);
  const __amdgpu_buffer_rsrc_t ors = make_rsrc(static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq, 2u * vd * nq);
  const float* glse = static_cast<const float*>(a.ws_lse) + bi * (int64_t)nq;
  const float* gD = static_cast<const float*>(a.ws_D) + bi * (int64_t)nq;

  // ---- resident B operands: lane (r,h) holds X[c = 16s + 8h + j][key = k0 + 32w + r]
  half8 kb[D / 16], vb[D / 16];
  stage_resident<D, kBK, kThr, ALN>(smem, K, V, d, vd, nk, k0, tid);
  __syncthreads();
  read_resident<D, kBK>(smem, w, g, tq, tp, kb);
  read_resident<D, kBK>(smem + S::kRow, w, g, tq, tp, vb);
#pragma unroll
  for (int s = 0; s < D / 16; ++s) kb[s] = scale8(kb[s], c2);  // S in log2 units straight out of the MFMA
  __syncthreads();  // the K/V images are reused by the ring

  // ---- query range of this key block and the per-lane / per-wave query intervals
  const int klast = min(k0 + kBK, nk) - 1;
  int qb = 0, qe = nq;
  if (POL != 0) q_range_for_k_block(a.rule, k0, klast, &qb, &qe);
  int qt0 = (qb / 32) * 32;
  int ntiles = (qe > qb) ? (qe - qt0 + 31) / 32 : 0;
  int qlim = nq;  // queries at or past it are staged as zeros with -lse2 = -inf
  if constexpr (SPLIT) {  // this chunk's share of that range (q_first and chunk are tile-aligned; wave-uniform)
    qt0 = args.q_first + (int)(bid % per_slice) * args.chunk;
    __builtin_assume(qt0 % 32 == 0);  // (the per-element query offsets then fold into the tile base)
    qlim = min(qt0 + args.chunk, args.q_end);
    ntiles = (qlim - qt0 + 31) / 32;
  }
  const int key = k0 + 32 * w + r;
  const int wk0 = k0 + 32 * w;
  const bool wave_active = wk0 < nk;
  const int ko = (POL == 2) ? seq_order(a.rule.k, a.rule, min(key, nk - 1)) : 0;  // this lane's key order
  int qlo = 0, qspan = nq, wlo_min = 0, wlo_max = 0, whi_min = nq - 1, whi_max = nq - 1;
  if (POL == 1 && wave_active) {
    int qhi;
    query_interval(a.rule, min(key, nk - 1), &qlo, &qhi);
    qspan = max(qhi - qlo + 1, 0);
    const int last = min(31, nk - 1 - wk0);
    wave_interval_ends(qlo, qhi, last, wlo_min, whi_min, wlo_max, whi_max);
  }
  const KeyWaveClass<POL> tcls{wave_active, nq, a.rule, wk0, nk, wlo_min, whi_max, wlo_max, whi_min};

  // ---- query-tile staging (Q, dO chunks: 8 queries of one channel row)
  using Stager = TileStager<D, kThr, 4, ALN>;
  const Stager stager(tid, nq);
  // two staging sets (tile t in set t&1): a tile is loaded two steps before it is stored
  u32x4 qr[2][kCPT];
  float lr[2] = {0.f, 0.f};
  // (SPLIT: the phantom tiles past the chunk's end move zeros too, not the next chunk's queries)
  auto load_tile = [&](int qa, int set) {
    stager.load(qr[set], qrs, ors, d, vd, qa, SPLIT ? qlim : nq);
    if (w == 0) {  // lanes 0..31: lse2, 32..63: D (wave-uniform branch; clamped load, select past nq)
      const int q = qa + (lane & 31);
      const float v = (lane < 32 ? glse : gD)[min(q, nq - 1)];
      lr[set] = (q < (SPLIT ? qlim : nq)) ? v : ((lane < 32) ? -__builtin_huge_valf() : 0.f);
    }
  };
  auto store_tile = [&](int slot, int set) {
    lds_char_t* base = smem + slot * S::kSlot;
    stager.store(base + S::offQT, base + S::offOT, qr[set]);
    if (w == 0) reinterpret_cast<lds_f_t*>(base + S::offLse)[lane] = lr[set];
  };

  floatx16 dk[kDO / 32], dv[kDO / 32];
#pragma unroll
  for (int u = 0; u < kDO / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[u][i] = 0.f; dv[u][i] = 0.f; }

  // row constants of the tile in `base` (stored negated) as initial accumulators: S: -lse2[q], dP: -D[q]
  auto init_acc = [&](const lds_char_t* base, floatx16& sacc, floatx16& pacc) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {  // registers 4gq..4gq+3 = queries 16(gq>>1) + 8h + 4(gq&1) + 0..3
      const int q4 = 16 * (gq >> 1) + 8 * h + 4 * (gq & 1);
      const floatx4 l4 = *reinterpret_cast<const lds_f4_t*>(base + S::offLse + 4 * q4);
      const floatx4 d4 = *reinterpret_cast<const lds_f4_t*>(base + S::offLse + 128 + 4 * q4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sacc[4 * gq + j] = l4[j];
        pacc[4 * gq + j] = d4[j];
      }
    }
  };
  // S = Qᵀ·K', dP = dOᵀ·V: A operands (row q, k = channel) by transposed reads
  auto sdp = [&](const lds_char_t* base, floatx16& sacc, floatx16& pacc) {
    constexpr int kAh = 0;
    half8 qa8[kAh + 1], oa8[kAh + 1];
    auto rd = [&](int s) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint32_t off = q16_off(16 * s + 8 * (g >> 1) + 4 * e + tq, 2 * (g & 1) + (sig >> 1), sig & 1);
        const half4 x = tr_read(base + S::offQT + off), y = tr_read(base + S::offOT + off);
        if (e == 0) { qa8[s % (kAh + 1)].lo = x; oa8[s % (kAh + 1)].lo = y; }
        else { qa8[s % (kAh + 1)].hi = x; oa8[s % (kAh + 1)].hi = y; }
      }
    };
#pragma unroll
    for (int s = 0; s < kAh; ++s) rd(s);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      if (s + kAh < D / 16) rd(s + kAh);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa8[s % (kAh + 1)], kb[s], sacc, 0, 0, 0);
      pacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(oa8[s % (kAh + 1)], vb[s], pacc, 0, 0, 0);
    }
  };
  // P = exp2(S), dS = P∘dP; k-step s of the dV / dK products = registers 8s..8s+7
  auto softmax_m = [&](const floatx16& sacc, const floatx16& pacc, int qa, bool masked, half8 (&pf)[2], half8 (&sf)[2])
      __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float pv = masked_exp2_q<POL>(sacc[i], masked, i, qa, h, qlo, qspan, nq, a.rule, ko);
      pf[i >> 3][i & 7] = (_Float16)pv;
      sf[i >> 3][i & 7] = (_Float16)(pv * pacc[i]);
    }
  };
  // the edge-tile mask as a real branch (see the producer / consumer pass)
  auto softmax = [&](const floatx16& sacc, const floatx16& pacc, int qa, int cls, half8 (&pf)[2], half8 (&sf)[2]) {
    if constexpr (POL == 0) {
      softmax_m(sacc, pacc, qa, cls == 1, pf, sf);
    } else if (cls == 1) {
      asm volatile("; edge tile" ::: );
      softmax_m(sacc, pacc, qa, true, pf, sf);
    } else {
      asm volatile("; interior tile" ::: );
      softmax_m(sacc, pacc, qa, false, pf, sf);
    }
  };
  // dV += dO·P, dK += Q·dS: A = X[row 32u + r][queries 16s + 8h + 0..7] (b128 reads of the Q16 images)
  auto dvdk = [&](const lds_char_t* base, const half8 (&pf)[2], const half8 (&sf)[2]) {
    constexpr int kU = kDO / 32, kN = 2 * kU, kAh = 0;
    half8 oa[kAh + 1], qa[kAh + 1];
    auto rd = [&](int n) __attribute__((always_inline)) {  // product n = kU·s + u
      const int s = n / kU, u = n % kU;
      oa[n % (kAh + 1)] = read_b128(base + S::offOT + q16_off(32 * (ou0 + u) + r, 2 * s + h));
      qa[n % (kAh + 1)] = read_b128(base + S::offQT + q16_off(32 * (ou0 + u) + r, 2 * s + h));
    };
#pragma unroll
    for (int n = 0; n < kAh; ++n) rd(n);
#pragma unroll
    for (int n = 0; n < kN; ++n) {
      if (n + kAh < kN) rd(n + kAh);
      const int s = n / kU, u = n % kU;
      dv[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(oa[n % (kAh + 1)], pf[s], dv[u], 0, 0, 0);
      dk[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa[n % (kAh + 1)], sf[s], dk[u], 0, 0, 0);
    }
  };

  load_tile(qt0, 0);  // unconditional, as in the dQ pass
  store_tile(0, 0);
  load_tile(qt0 + 32, 1);
  load_tile(qt0 + 64, 0);

  // iteration it: tile it in slot it&1 (complete after the barrier); tile it+1 -> slot (it+1)&1
  // (read in iteration it-1, finished before this barrier) from staging set (it+1)&1, which then
  // takes tile it+3.  Loads and stores are unconditional (past the end they move zeros into
  // a slot nobody reads), so hipcc's vmcnt waits stay exact: a store waits only for the load
  // issued two steps earlier.
  auto step = [&](auto P_, int it) {
    constexpr int p = decltype(P_)::value;
    __syncthreads();
    const int qa = qt0 + 32 * it;
    store_tile(p ^ 1, p ^ 1);
    load_tile(qa + 96, p ^ 1);
    const int cls = it < ntiles ? tcls(qa) : 0;  // (the loop's last pair may end on a phantom step)
    if (cls == 0) return;
    const lds_char_t* base = smem + p * S::kSlot;
    floatx16 sacc, pacc;
    init_acc(base, sacc, pacc);
    sdp(base, sacc, pacc);
    half8 pf[2], sf[2];
    softmax(sacc, pacc, qa, cls, pf, sf);
    dvdk(base, pf, sf);
  };
  // whole pairs of steps: a conditional second step (it loads) made hipcc's vmcnt waits before the
  // staging stores drain every load in flight, the one issued a step earlier included
  for (int it = 0; it < ntiles; it += 2) {
    step(IC<0>{}, it);
    step(IC<1>{}, it + 1);
  }

  // ---- dK = scale·Σ dS·Q, dV: rows c = 32u + (i&3) + 8(i>>2) + 4h, column = this lane's key
  if (!wave_active || key >= nk) return;
  if constexpr (SPLIT) {  // bid = slice * nchunks + chunk
    store_partial<kDO / 32>(args.ws_part + (int64_t)bid * (d + vd) * nk, dk, dv, d, vd, nk, key, h);
    return;
  }
  __half* dK = static_cast<__half*>(a.dK) + bi * (int64_t)d * nk;
  __half* dV = static_cast<__half*>(a.dV) + bi * (int64_t)vd * nk;
  const float sc = (float)a.scale;
  store_grad<D, kDO / 32>({{dk, dK, d, sc}, {dv, dV, vd, 1.f}}, nk, key, h, ou0);
}

// ---------------------------------------------------------------------------
// dK / dV, producer / consumer (two waves per SIMD).  Waves w and w+4 share a SIMD and the same
// 32 keys.  Wave w (producer) forms S = Qᵀ·K' and dP = dOᵀ·V for query tile i, P = exp2(S) and
// dS = P∘dP, and hands P and dS to wave w+4 through LDS; wave w+4 (consumer) accumulates
// dV += dO·P and dK += Q·dS for tile i-1.  The producer's softmax VALU runs beside the
// consumer's MFMAs on the shared SIMD (the one-wave-per-SIMD kernel above serialises them), and
// the register file splits along the data: K', V and the S / dP accumulators live in the
// producer, the dK / dV accumulators in the consumer, each role inside its own loop so neither
// carries the other's registers (under 256 each at D = 128).  Every step: one barrier, the
// staging of tile i+1 into the ring, the load of tile i+3.
template <int D>
struct PcSmem {
  static constexpr int kBK = 128;            // keys per workgroup: four producer waves x 32
  static constexpr int kRow = D * kBK * 2;   // K (or V) row image (prologue only)
  static constexpr int kQT = D * 64;         // one [D][32] Q16 image
  static constexpr int offQT = 0, offOT = kQT, offLse = 2 * kQT, offD = offLse + 256;
  static constexpr int kSlot = offLse + 2 * 64 * 4;  // + -lse2[32], -D[32] (64-float vectors: LDS-DMA lanes)
  static constexpr int kNS = 4;              // query-tile ring
  static constexpr int offX = kNS * kSlot;   // P / dS hand-over: 2 slots x 4 waves x 4 KB
  static constexpr int kXWave = 4096;
  static constexpr int kXSlot = 4 * kXWave;
  static constexpr int kUsed = offX + 2 * kXSlot;
  static constexpr int kTotal = kUsed > 2 * kRow ? kUsed : 2 * kRow;  // the K/V images alias the ring
};

// SPLIT: as in bwd_dkdv_kernel (the consumers store the partial record).
template <int D, int POL, bool ALN, bool SPLIT = false>
__global__ __launch_bounds__(512, 1) void bwd_dkdv_pc_kernel(typename DkdvArgsOf<SPLIT>::type args) {
  const BwdArgs& a = dkdv_bwd_args(args);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  using S = PcSmem<D>;
  constexpr int kThr = 512;
  constexpr int kBK = S::kBK;
  constexpr int kQChunks = D * 4;                 // 16-B chunks of one [D][32] tile
  static_assert((2 * kQChunks) % kThr == 0, "tile chunks must divide over the workgroup");
  constexpr int kCPT = 2 * kQChunks / kThr;       // Q and dO chunks per thread
  const int nq = a.rule.q.n, nk = a.rule.k.n;
  const uint32_t nkb = (nk + kBK - 1) / kBK;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  uint32_t per_slice = nkb;  // SPLIT: one key block (k0 = 0) and the chunks of its query range
  if constexpr (SPLIT) per_slice = (uint32_t)args.nchunks;
  const int64_t bi = bid / per_slice;
  const int k0 = SPLIT ? 0 : (int)(bid % nkb) * kBK;  // earliest (heaviest under causal) key blocks first
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w >> 2, wl = w & 3;  // group 0 produces, group 1 consumes; wl: the key slice
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const int sig = ((tp & 1) << 1) | (tp >> 1);  // (see the dK/dV kernel above: σ-permuted transposed reads)
  const float c2 = (float)a.scale * kLog2e;

  const int d = a.d, vd = a.v_d;
  const __half* K = static_cast<const __half*>(a.K) + bi * (int64_t)d * nk;
  const __half* V = static_cast<const __half*>(a.V) + bi * (int64_t)vd * nk;
  const __amdgpu_buffer_rsrc_t qrs = make_rsrc(static_cast<const __half*>(a.Q) + bi * (int64_t)d * nq, 2u * d * nq);
  const __amdgpu_buffer_rsrc_t ors = make_rsrc(static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq, 2u * vd * nq);
  const float* glse = static_cast<const float*>(a.ws_lse) + bi * (int64_t)nq;
  const float* gD = static_cast<const float*>(a.ws_D) + bi * (int64_t)nq;

  // ---- K, V blocks into LDS (every thread); the producers read their resident B operands below
  stage_resident<D, kBK, kThr, ALN>(smem, K, V, d, vd, nk, k0, tid);
  __syncthreads();

  // ---- query range of this key block and the per-lane / per-wave query intervals (both roles)
  const int klast = min(k0 + kBK, nk) - 1;
  int qb = 0, qe = nq;
  if (POL != 0) q_range_for_k_block(a.rule, k0, klast, &qb, &qe);
  int qt0 = (qb / 32) * 32;
  int ntiles = (qe > qb) ? (qe - qt0 + 31) / 32 : 0;
  int qlim = nq;  // queries at or past it are staged as zeros with -lse2 = -inf
  if constexpr (SPLIT) {  // this chunk's share of that range (q_first and chunk are tile-aligned; wave-uniform)
    qt0 = args.q_first + (int)(bid % per_slice) * args.chunk;
    __builtin_assume(qt0 % 32 == 0);
    qlim = min(qt0 + args.chunk, args.q_end);
    ntiles = (qlim - qt0 + 31) / 32;
  }
  const int key = k0 + 32 * wl + r;
  const int wk0 = k0 + 32 * wl;
  const bool wave_active = wk0 < nk;
  int qlo = 0, qspan = nq, wlo_min = 0, wlo_max = 0, whi_min = nq - 1, whi_max = nq - 1;
  if (POL == 1 && wave_active) {
    int qhi;
    query_interval(a.rule, min(key, nk - 1), &qlo, &qhi);
    qspan = max(qhi - qlo + 1, 0);
    const int last = min(31, nk - 1 - wk0);
    wave_interval_ends(qlo, qhi, last, wlo_min, whi_min, wlo_max, whi_max);
  }
  const KeyWaveClass<POL> tcls{wave_active, nq, a.rule, wk0, nk, wlo_min, whi_max, wlo_max, whi_min};

  // ---- query-tile staging, every thread (Q, dO chunks: 8 queries of one channel row)
  using Stager = TileStager<D, kThr, 4, ALN>;
  const Stager stager(tid, nq);
  u32x4 qr[2][kCPT];  // two staging sets: tile t in set t&1, loaded two steps before it is stored
  float lr[2] = {0.f, 0.f};
  auto load_tile = [&](int qa, int set) __attribute__((always_inline)) {
    stager.load(qr[set], qrs, ors, d, vd, qa, SPLIT ? qlim : nq);
    if (w == 0) {  // lanes 0..31: -lse2, 32..63: -D (a wave-uniform scalar branch; the load itself is
                   // unconditional, clamped into the row, and the select replaces rows past nq)
      const int q = qa + (lane & 31);
      const float v = (lane < 32 ? glse : gD)[min(q, nq - 1)];
      lr[set] = (q < (SPLIT ? qlim : nq)) ? v : ((lane < 32) ? -__builtin_huge_valf() : 0.f);
    }
  };
  auto store_tile = [&](int slot, int set) __attribute__((always_inline)) {
    lds_char_t* base = smem + slot * S::kSlot;
    stager.store(base + S::offQT, base + S::offOT, qr[set]);
    // (PcSmem keeps -lse2 and -D 256 B apart, a 64-float vector each as the removed LDS-DMA staging wrote
    // them; DkdvSmem / W4Smem 128 B apart, where this select folds away.  Needed for this layout; the
    // layout's padding costs 4 x 256 B of LDS and no kernel depends on it.)
    if (w == 0) reinterpret_cast<lds_f_t*>(base + (lane < 32 ? S::offLse : S::offD - 128))[lane] = lr[set];
  };
  // hand-over slot of this wave pair: four b128 per lane (P k-steps 0/1, dS k-steps 0/1), lane-linear
  auto xoff = [&](int xs, int j) -> uint32_t { return S::offX + xs * S::kXSlot + wl * S::kXWave + j * 1024 + lane * 16; };

  // Steps it = 0 .. ntiles: the producer handles tile it (it < ntiles), the consumer tile it-1 (it >= 1).
  // Whole groups of four steps (ring slot it % 4, staging set (it+1) % 2, hand-over slot it % 2 are
  // compile-time); loads and stores are unconditional (phantom tiles move zeros), so hipcc's vmcnt
  // waits stay exact.
  const int nsteps = ntiles + 1;
  auto stage = [&](auto C_, int it) __attribute__((always_inline)) {
    constexpr int c = decltype(C_)::value;
    __syncthreads();
    store_tile((c + 1) % 4, (c + 1) % 2);         // tile it+1 (loaded in step it-2)
    load_tile(qt0 + 32 * (it + 3), (c + 1) % 2);  // tile it+3 into the set just stored
  };
  // first tiles: tile 0's loads issued now, its store after the barrier that retires the K/V images
  load_tile(qt0, 0);
  auto stage0 = [&]() __attribute__((always_inline)) {
    __syncthreads();
    store_tile(0, 0);
    load_tile(qt0 + 32, 1);
    load_tile(qt0 + 64, 0);
  };

  if (grp == 0) {
    // ================= producer
    half8 kb[D / 16], vb[D / 16];  // resident B operands: lane (r,h) holds X[c = 16s + 8h + j][key]
    read_resident<D, kBK>(smem, wl, g, tq, tp, kb);
    read_resident<D, kBK>(smem + S::kRow, wl, g, tq, tp, vb);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) kb[s] = scale8(kb[s], c2);  // S in log2 units straight out of the MFMA
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every image read done before the ring reuses it
    stage0();
    const int ko = (POL == 2) ? seq_order(a.rule.k, a.rule, min(key, nk - 1)) : 0;
    // row constants (-lse2, -D) of a tile: registers 4gq..4gq+3 = queries 16(gq>>1) + 8h + 4(gq&1) + 0..3
    auto read_rowc = [&](const lds_char_t* base, floatx16& sa, floatx16& pa) __attribute__((always_inline)) {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int q4 = 16 * (gq >> 1) + 8 * h + 4 * (gq & 1);
        const floatx4 l4 = *reinterpret_cast<const lds_f4_t*>(base + S::offLse + 4 * q4);
        const floatx4 d4 = *reinterpret_cast<const lds_f4_t*>(base + S::offD + 4 * q4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sa[4 * gq + j] = l4[j];
          pa[4 * gq + j] = d4[j];
        }
      }
    };
    // the S / dP A operands of k-step s_ (transposed reads of the Q16 images)
    auto read_ops = [&](const lds_char_t* base, int s_, half8& q8, half8& o8) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint32_t off = q16_off(16 * s_ + 8 * (g >> 1) + 4 * e + tq, 2 * (g & 1) + (sig >> 1), sig & 1);
        const half4 x = tr_read(base + S::offQT + off), y = tr_read(base + S::offOT + off);
        if (e == 0) { q8.lo = x; o8.lo = y; } else { q8.hi = x; o8.hi = y; }
      }
    };
    auto pstep = [&](auto C_, int it) __attribute__((always_inline)) {
      constexpr int c = decltype(C_)::value;
      stage(C_, it);
      const int qa = qt0 + 32 * it;
      const int cls = it < ntiles ? tcls(qa) : 0;
      const lds_char_t* base = smem + c * S::kSlot;
      floatx16 sacc, pacc;
      if (cls != 0) {
        // S = Qᵀ·K', dP = dOᵀ·V: A operands by transposed reads, two k-steps ahead of their MFMAs
        constexpr int kS = D / 16, kAh = 2;
        half8 qa8[kAh + 1], oa8[kAh + 1];
        auto rd = [&](int s_) __attribute__((always_inline)) {
          read_ops(base, s_, qa8[s_ % (kAh + 1)], oa8[s_ % (kAh + 1)]);
        };
        read_rowc(base, sacc, pacc);
#pragma unroll
        for (int s_ = 0; s_ < kAh; ++s_) rd(s_);
#pragma unroll
        for (int s_ = 0; s_ < kS; ++s_) {
          if (s_ + kAh < kS) rd(s_ + kAh);
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa8[s_ % (kAh + 1)], kb[s_], sacc, 0, 0, 0);
          pacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(oa8[s_ % (kAh + 1)], vb[s_], pacc, 0, 0, 0);
        }
      }
      if (cls == 0) return;
      // P = exp2(S), dS = P∘dP; register i = query 16(i>>3) + 8h + (i&7) = k-step i>>3 of the consumer
      half8 pf[2], sf[2];
      auto softmax = [&](bool masked) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pv = masked_exp2_q<POL>(sacc[i], masked, i, qa, h, qlo, qspan, nq, a.rule, ko);
          pf[i >> 3][i & 7] = (_Float16)pv;
          sf[i >> 3][i & 7] = (_Float16)(pv * pacc[i]);
        }
      };
      // the edge-tile mask as a real branch: in one basic block hipcc if-converts it into an index add,
      // a compare and two selects per score on every tile (c3 backward 8.35 -> 7.72 ms)
      if (POL != 0 && cls == 1) {
        asm volatile("; edge tile" ::: );
        softmax(true);
      } else {
        asm volatile("; interior tile" ::: );
        softmax(false);
      }
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) {
        *reinterpret_cast<lds_half8_t*>(smem + xoff(c % 2, s_)) = pf[s_];
        *reinterpret_cast<lds_half8_t*>(smem + xoff(c % 2, 2 + s_)) = sf[s_];
      }
    };
    for (int it = 0; it < nsteps; it += 4) {
      pstep(IC<0>{}, it);
      pstep(IC<1>{}, it + 1);
      pstep(IC<2>{}, it + 2);
      pstep(IC<3>{}, it + 3);
    }
    return;
  }

  // ================= consumer
  stage0();
  floatx16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[u][i] = 0.f; dv[u][i] = 0.f; }
  auto cstep = [&](auto C_, int it) __attribute__((always_inline)) {
    constexpr int c = decltype(C_)::value;
    stage(C_, it);
    const int qa = qt0 + 32 * (it - 1);
    const int cls = (it >= 1 && it - 1 < ntiles) ? tcls(qa) : 0;
    const lds_char_t* base = smem + ((c + 3) % 4) * S::kSlot;
    // dV += dO·P, dK += Q·dS: A = X[row 32u + r][queries 16s + 8h + 0..7] (b128 reads, two ahead)
    constexpr int kU = D / 32, kN = 2 * kU, kAh = 2;
    half8 pf[2], sf[2], oa[kAh + 1], qa_[kAh + 1];
    auto rd = [&](int n) __attribute__((always_inline)) {
      const int s_ = n / kU, u = n % kU;
      oa[n % (kAh + 1)] = read_b128(base + S::offOT + q16_off(32 * u + r, 2 * s_ + h));
      qa_[n % (kAh + 1)] = read_b128(base + S::offQT + q16_off(32 * u + r, 2 * s_ + h));
    };
    if (cls != 0) {
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) {
        pf[s_] = read_b128(smem + xoff((c + 1) % 2, s_));
        sf[s_] = read_b128(smem + xoff((c + 1) % 2, 2 + s_));
      }
#pragma unroll
      for (int n = 0; n < kAh; ++n) rd(n);
    }
    if (cls == 0) return;
#pragma unroll
    for (int n = 0; n < kN; ++n) {
      if (n + kAh < kN) rd(n + kAh);
      const int s_ = n / kU, u = n % kU;
      dv[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(oa[n % (kAh + 1)], pf[s_], dv[u], 0, 0, 0);
      dk[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa_[n % (kAh + 1)], sf[s_], dk[u], 0, 0, 0);
    }
  };
  for (int it = 0; it < nsteps; it += 4) {
    cstep(IC<0>{}, it);
    cstep(IC<1>{}, it + 1);
    cstep(IC<2>{}, it + 2);
    cstep(IC<3>{}, it + 3);
  }

  // ---- dK = scale·Σ dS·Q, dV: rows c = 32u + (i&3) + 8(i>>2) + 4h, column = this lane's key
  if (!wave_active || key >= nk) return;
  if constexpr (SPLIT) {  // bid = slice * nchunks + chunk
    store_partial<D / 32>(args.ws_part + (int64_t)bid * (d + vd) * nk, dk, dv, d, vd, nk, key, h);
    return;
  }
  __half* dK = static_cast<__half*>(a.dK) + bi * (int64_t)d * nk;
  __half* dV = static_cast<__half*>(a.dV) + bi * (int64_t)vd * nk;
  const float sc = (float)a.scale;
  store_grad<D, D / 32>({{dk, dK, d, sc}, {dv, dV, vd, 1.f}}, nk, key, h, 0);
}

// dK and dV of the split forms: one thread per (slice, row of the record, key), keys fastest.  The chunk
// partials are added in chunk order in fp32 (no atomics: the result is deterministic and a slice's bits do
// not depend on the batch), then scaled (dK; dV by 1) and rounded as store_grad does.  The loads of a group
// of eight chunks are issued together; only the additions are a chain.
__global__ __launch_bounds__(256) void dkdv_split_reduce_kernel(BwdQSplitArgs sa) {
  const BwdArgs& a = sa.b;
  const int nc = sa.nchunks;
  const int64_t nk = a.rule.k.n;
  const int64_t per = (int64_t)(a.d + a.v_d) * nk, perk = (int64_t)a.d * nk;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bi = gid / per, e = gid - bi * per;
  const float* part = sa.ws_part + bi * nc * per + e;
  float sum = 0.f;
  int c = 0;
  for (; c + 8 <= nc; c += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(c + j) * per];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += v[j];
  }
  for (; c < nc; ++c) sum += part[c * per];
  if (e < perk)
    static_cast<__half*>(a.dK)[bi * perk + e] = __float2half(sum * (float)a.scale);
  else
    static_cast<__half*>(a.dV)[bi * (per - perk) + (e - perk)] = __float2half(sum * 1.f);
}

template <int D, int NW, int WPE>
hipError_t launch_dkdv(const BwdArgs& a, hipStream_t s) {
  using S = DkdvSmem<D, NW>;
  const int64_t nkb = (a.rule.k.n + S::kBK - 1) / S::kBK;
  return launch_smem(with_pol_aln(a, [](auto pol, auto aln) { return &bwd_dkdv_kernel<D, NW, WPE, pol.value, aln.value>; }),
                     (unsigned)(a.b * nkb), NW * 64, S::kTotal, s, a);
}

template <int D>
hipError_t launch_dkdv_pc(const BwdArgs& a, hipStream_t s) {
  using S = PcSmem<D>;
  const int64_t nkb = (a.rule.k.n + S::kBK - 1) / S::kBK;
  return launch_smem(with_pol_aln(a, [](auto pol, auto aln) { return &bwd_dkdv_pc_kernel<D, pol.value, aln.value>; }),
                     (unsigned)(a.b * nkb), 512, S::kTotal, s, a);
}

// the same two passes on one workgroup per (slice, query chunk), at the unsplit instances' launch bounds (no
// split instance spills there, profiles/bwd_dkdv_split_resources.txt), then the reduce over the chunks
hipError_t launch_dkdv_qsplit(const BwdQSplitArgs& sa, hipStream_t s) {
  const BwdArgs& a = sa.b;
  hipError_t e;
  if (max(a.d, a.v_d) <= 64)
    e = launch_smem(with_pol_aln(a, [](auto pol, auto aln) {
                      return &bwd_dkdv_kernel<64, 4, 2, pol.value, aln.value, 1, true>;
                    }),
                    (unsigned)(a.b * sa.nchunks), 256, DkdvSmem<64, 4>::kTotal, s, sa);
  else
    e = launch_smem(
        with_pol_aln(a, [](auto pol, auto aln) { return &bwd_dkdv_pc_kernel<128, pol.value, aln.value, true>; }),
        (unsigned)(a.b * sa.nchunks), 512, PcSmem<128>::kTotal, s, sa);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)(a.d + a.v_d) * a.rule.k.n;
  hipLaunchKernelGGL(dkdv_split_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, sa);
  return hipGetLastError();
}

// -D and -lse2 of every query; eight queries a thread where the rows allow 16-B loads
hipError_t launch_prep(const BwdArgs& a, hipStream_t s, bool allow_prep8 = true) {
  const int64_t nrows = a.b * (int64_t)a.rule.q.n;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool prep8 = allow_prep8 && (a.rule.q.n % 8) == 0 && al16(a.O) && al16(a.dO) && al16(a.ws_D) && al16(a.ws_lse);
  if (prep8)
    hipLaunchKernelGGL(bwd_prep8_kernel, dim3((unsigned)((nrows / 8 + kThrPrep - 1) / kThrPrep)), dim3(kThrPrep), 0, s, a);
  else
    hipLaunchKernelGGL(bwd_prep_kernel, dim3((unsigned)((nrows + kThrPrep - 1) / kThrPrep)), dim3(kThrPrep), 0, s, a);
  return hipGetLastError();
}

// The dK/dV pass for max(d, v_d) <= 128.  d <= 64: the one-wave pass at two waves per SIMD; d = 128, tuned
// on c3: the producer / consumer pass (one-process A/B: 9.20 -> 8.59 ms backward; two barriers per step,
// 1402, and a prioritised producer, 1401, measured 8.70 / 8.77).
// variant (diagnostic library, FA_BWD_VARIANT; else -1): 82 eight-wave blocks at d <= 64; 1700-1799 the
// 64-keys-a-wave pass at d = 128 where it applies.  The other A/B variants of rounds 2-4 (stamp builds,
// LDS-DMA staging, the four-role dK/dV pass) were measured and removed.
hipError_t launch_dkdv_pass(const BwdArgs& a, hipStream_t s, int variant) {
  (void)variant;
  if (max(a.d, a.v_d) <= 64) {
#ifdef FA_DIAG
    if (variant == 82) return launch_dkdv<64, 8, 2>(a, s);
#endif
    return launch_dkdv<64, 4, 2>(a, s);
  }
#ifdef FA_DIAG
  if (variant >= 1700 && variant < 1800 && bwd_dkdv_k64_supported(a)) return launch_dkdv_k64(a, s);
#endif
  return launch_dkdv_pc<128>(a, s);
}

}  // namespace

bool bwd_f16_fast_supported(const BwdArgs& a) {
  const int nq = a.rule.q.n, nk = a.rule.k.n;
  const int dm = max(a.d, a.v_d);
  // (buffer offsets are 32-bit: a channel row set of one slice stays below 2^31 bytes; the element-wise
  // staging of the unaligned form addresses up to 2·n + 14 bytes past a row start)
  return dm >= 1 && dm <= 256 && nq > 0 && nk > 0 &&
         (int64_t)dm * (nq + 8) * 2 < (1ll << 31) &&
         (int64_t)dm * (nk + 8) * 2 < (1ll << 31) && a.b * ((nk + 127) / 128) * 2 < (1ll << 31) &&
         a.b * ((nq + 127) / 128) * 2 < (1ll << 31);
}

// Slices per call of launch_bwd_f16_split: every grid (prep, dK/dV, split dQ, reduce) stays below 2^31 blocks.
int64_t bwd_f16_split_max_batch(const BwdSplitArgs& sa) {
  const BwdArgs& a = sa.b;
  const int64_t reduce_blocks = ((int64_t)a.d * a.rule.q.n + 255) / 256;
  const int64_t dkdv_blocks = 2 * (((int64_t)a.rule.k.n + 127) / 128);  // (the bound of bwd_f16_fast_supported)
  int64_t per = sa.nchunks > reduce_blocks ? sa.nchunks : reduce_blocks;
  if (dkdv_blocks > per) per = dkdv_blocks;
  return ((1ll << 31) - 1) / per;
}

// One query block (nq <= 128), max(d, v_d) <= 128: the prep and the dK/dV pass launch_bwd_f16_fast runs
// for the shape, then the dQ pass split over key chunks (fa_bwd_f16_dq.hip)
hipError_t launch_bwd_f16_split(const BwdSplitArgs& sa, hipStream_t s) {
  hipError_t e = launch_prep(sa.b, s);
  if (e != hipSuccess) return e;
  e = launch_dkdv_pass(sa.b, s, -1);
  if (e != hipSuccess) return e;
  return launch_bwd_f16_dq_split(sa, s);
}

// Slices per call of launch_bwd_f16_qsplit: every grid (prep, split dK/dV, reduce, dQ) stays below 2^31 blocks.
int64_t bwd_f16_qsplit_max_batch(const BwdQSplitArgs& sa) {
  const BwdArgs& a = sa.b;
  const int64_t reduce_blocks = ((int64_t)(a.d + a.v_d) * a.rule.k.n + 255) / 256;
  const int64_t dq_blocks = 2 * (((int64_t)a.rule.q.n + 127) / 128);  // (the bound of bwd_f16_fast_supported; the prep's too)
  int64_t per = sa.nchunks > reduce_blocks ? sa.nchunks : reduce_blocks;
  if (dq_blocks > per) per = dq_blocks;
  return ((1ll << 31) - 1) / per;
}

// One key block (nk <= 128), max(d, v_d) <= 128, against a long query range: the prep launch_bwd_f16_fast
// runs for the shape, the dK/dV pass split over query chunks with its reduce, then the dQ pass
// launch_bwd_f16_fast runs for the shape (dQ is bitwise its dQ)
hipError_t launch_bwd_f16_qsplit(const BwdQSplitArgs& sa, hipStream_t s) {
  hipError_t e = launch_prep(sa.b, s);
  if (e != hipSuccess) return e;
  e = launch_dkdv_qsplit(sa, s);
  if (e != hipSuccess) return e;
  return launch_bwd_f16_dq(sa.b, s, -1);
}

hipError_t launch_bwd_f16_fast(const BwdArgs& a, hipStream_t s) {
  int v = -1;  // FA_BWD_VARIANT (diagnostic library): A/B structures of the passes
#ifdef FA_DIAG
  v = diag_variant("FA_BWD_VARIANT");
#endif
  hipError_t e = launch_prep(a, s, v != 1430);  // (1430: the one-query-a-thread prep, for A/B)
  if (e != hipSuccess) return e;
  // (1421: round 4's D = 256 passes, two 128-channel chunks with S / dP formed in each; 16-B chunk staging only)
  if (max(a.d, a.v_d) > 128) return launch_bwd_f16_wide(a, s, v == 1421 && bwd_aligned(a));
  e = launch_dkdv_pass(a, s, v);
  if (e != hipSuccess) return e;
  return launch_bwd_f16_dq(a, s, v);
}

#ifdef FA_DIAG
// round 4's D = 256 dK/dV pass for launch_bwd_f16_wide: the one-wave kernel on two 128-channel chunks
hipError_t launch_bwd_f16_dkdv_oc2(const BwdArgs& a, hipStream_t s) {
  using S = DkdvSmem<256, 4>;
  const int64_t nkb = (a.rule.k.n + S::kBK - 1) / S::kBK;
  const int pol = bwd_pol(a.rule);
  return launch_smem(pol == 0   ? bwd_dkdv_kernel<256, 4, 1, 0, true, 2>
                     : pol == 1 ? bwd_dkdv_kernel<256, 4, 1, 1, true, 2>
                                : bwd_dkdv_kernel<256, 4, 1, 2, true, 2>,
                     (unsigned)(a.b * nkb * 2), 256, S::kTotal, s, a);
}
#endif

}  // namespace fa
