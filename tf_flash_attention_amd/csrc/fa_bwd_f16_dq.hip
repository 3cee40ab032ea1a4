// fa_bwd_f16_dq.hip — the dQ pass of the fp16 two-pass backward for max(d, v_d) <= 128, every rule
// (fa_bwd_f16_fast.hip describes the passes and runs the prep and the dK/dV pass first):
//   bwd_dq_kernel           query-outer, a wave owns 32 queries; also the form split over key chunks
//   dq_split_reduce_kernel  the sum of the split form's fp32 partials
//   bwd_dq_pc_kernel        producer / consumer at D = 128, two waves per SIMD
// The pieces shared with the other backward kernels are in fa_bwd_f16_parts.h.
// Replaces the query side of the reference's BackwardImpl (flash_attention.cu:1079-1967) and its
// spin-locked dQ read-modify-write.
#include "fa_bwd_f16_parts.h"

namespace fa {
namespace {

using namespace bwdp;

// ---------------------------------------------------------------------------
template <int D, int NW>
struct DqSmem {
  static constexpr int kBM = 32 * NW;                 // queries per workgroup
  static constexpr int kRow = D * kBM * 2;            // Q (or dO) row image
  static constexpr int kKT = D * 128;                 // one [D][64] KT image
  static constexpr int offKT = 0, offVT = kKT;
  static constexpr int kSlot = 2 * kKT;
  static constexpr int kRing = 2 * kSlot;
  static constexpr int kTotal = (kRing > 2 * kRow) ? kRing : 2 * kRow;  // the Q/dO images alias the ring
};

// dQ: query-outer.  One workgroup = NW waves x 32 queries of one (batch, head) slice.
// OC > 1 (128 < d <= 256): the workgroup accumulates dQ for one of OC chunks of D / OC channels (chunk =
// block index mod OC), recomputing Sᵀ and dPᵀ over all D channels.  ONESET: one staging register set
// (tile it+1 loaded at the head of step it and stored after its MFMAs, into the slot tile it-1 left)
// instead of two sets loaded two steps ahead: at D = 256 a set is 64 registers.
// SPLIT (one query block against a long key range, BwdSplitArgs): the grid is (slice, key chunk);
// the workgroup walks only the tiles of its chunk of the block's key range and stores its unscaled
// fp32 accumulator as the partial record [d][nq] of (slice, chunk); dq_split_reduce_kernel sums them.
template <bool SPLIT> struct DqArgsOf { using type = BwdArgs; };
template <> struct DqArgsOf<true> { using type = BwdSplitArgs; };
__device__ __forceinline__ const BwdArgs& dq_bwd_args(const BwdArgs& x) { return x; }
__device__ __forceinline__ const BwdArgs& dq_bwd_args(const BwdSplitArgs& x) { return x.b; }

template <int D, int NW, int WPE, int POL, bool ALN, bool PRE = false, bool MSPEC = false, int OC = 1, bool ONESET = false,
          bool SPLIT = false>
__global__ __launch_bounds__(NW * 64, WPE) void bwd_dq_kernel(typename DqArgsOf<SPLIT>::type args) {
  static_assert(!SPLIT || (OC == 1 && !ONESET), "the split form is the one-wave pass at D <= 128");
  const BwdArgs& a = dq_bwd_args(args);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  using S = DqSmem<D, NW>;
  constexpr int kThr = NW * 64;
  constexpr int kBM = S::kBM;
  constexpr int kBN = 64;
  constexpr int kKChunks = D * 8;                     // 16-B chunks of one [D][64] tile
  static_assert((2 * kKChunks) % kThr == 0, "tile chunks must divide over the workgroup");
  constexpr int kCPT = 2 * kKChunks / kThr;           // K and V chunks per thread
  constexpr float kNegInf = -__builtin_huge_valf();

  constexpr int kDO = D / OC;  // dQ channels of this workgroup
  const int nq = a.rule.q.n, nk = a.rule.k.n;
  const uint32_t nqb = (nq + kBM - 1) / kBM;
  const uint32_t bidc = xcd_remap(blockIdx.x, gridDim.x);
  const int oc = (int)(bidc % OC), ou0 = oc * (kDO / 32);
  const uint32_t bid = bidc / OC;
  uint32_t per_slice = nqb;  // SPLIT: one query block (q0 = 0) and the chunks of its key range
  if constexpr (SPLIT) per_slice = (uint32_t)args.nchunks;
  const int64_t bi = bid / per_slice;
  const int q0 = SPLIT ? 0 : (int)(nqb - 1 - (bid % nqb)) * kBM;  // latest (heaviest under causal) blocks first
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const float c2 = (float)a.scale * kLog2e;

  const int d = a.d, vd = a.v_d;
  const __half* Q = static_cast<const __half*>(a.Q) + bi * (int64_t)d * nq;
  const __half* dO = static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq;
  const __amdgpu_buffer_rsrc_t krs = make_rsrc(static_cast<const __half*>(a.K) + bi * (int64_t)d * nk, 2u * d * nk);
  const __amdgpu_buffer_rsrc_t vrs = make_rsrc(static_cast<const __half*>(a.V) + bi * (int64_t)vd * nk, 2u * vd * nk);

  const int wq0 = q0 + 32 * w;
  const int qi = wq0 + r;
  const bool wave_active = wq0 < nq;

  // ---- resident B operands: lane (r,h) holds X[c = 16s + 8h + j][q = wq0 + r]
  half8 qf[D / 16], of[D / 16];
  stage_resident<D, kBM, kThr, ALN>(smem, Q, dO, d, vd, nq, q0, tid);
  __syncthreads();
  read_resident<D, kBM>(smem, w, g, tq, tp, qf);
  read_resident<D, kBM>(smem + S::kRow, w, g, tq, tp, of);
#pragma unroll
  for (int s = 0; s < D / 16; ++s) qf[s] = scale8(qf[s], c2);
  __syncthreads();  // the Q/dO images are reused by the ring
  // row constants (this lane's query) as the C operands of the Sᵀ / dPᵀ chains
  floatx16 negl, negd;
  {
    const float* glse = static_cast<const float*>(a.ws_lse) + bi * (int64_t)nq;
    const float* gD = static_cast<const float*>(a.ws_D) + bi * (int64_t)nq;
    const float lv = (qi < nq) ? glse[qi] : kNegInf, dv = (qi < nq) ? gD[qi] : 0.f;  // (stored negated)
#pragma unroll
    for (int i = 0; i < 16; ++i) { negl[i] = lv; negd[i] = dv; }
  }

  // ---- key range of this query block (rule-bounded), per-lane key intervals
  const int qlast = min(q0 + kBM, nq) - 1;
  int kb = 0, ke = nk;
  if (POL != 0) k_range_for_q_block(a.rule, q0, qlast, &kb, &ke);
  int kt0 = (kb / kBN) * kBN;
  int ntiles = (ke > kb) ? (ke - kt0 + kBN - 1) / kBN : 0;
  if constexpr (SPLIT) {  // this chunk's share of that range (k_first and chunk are tile-aligned; wave-uniform)
    kt0 = args.k_first + (int)(bid % per_slice) * args.chunk;
    __builtin_assume(kt0 % kBN == 0);  // (the per-element key offsets then fold into the tile base)
    ntiles = (min(kt0 + args.chunk, args.k_end) - kt0 + kBN - 1) / kBN;
  }
  int klo = 0, kspan = nk, wlo_min = 0, wlo_max = 0, whi_min = nk - 1, whi_max = nk - 1;
  if (POL == 1 && wave_active) {
    int khi;
    key_interval(a.rule, min(qi, nq - 1), &klo, &khi);
    kspan = max(khi - klo + 1, 0);
    const int last = min(31, nq - 1 - wq0);
    wave_interval_ends(klo, khi, last, wlo_min, whi_min, wlo_max, whi_max);
  }
  const QueryWaveClass<POL, kBN> tcls{wave_active, nk, a.rule, wq0, nq, wlo_min, whi_max, wlo_max, whi_min};

  const int qo = (POL == 2) ? seq_order(a.rule.q, a.rule, min(qi, nq - 1)) : 0;  // this lane's query order

  // ---- key-tile staging (K, V chunks: 8 keys of one channel row)
  using Stager = TileStager<D, kThr, 8, ALN>;
  const Stager stager(tid, nk);
  // two staging sets (tile t in set t&1): a tile is loaded two steps before it is stored
  u32x4 kr[ONESET ? 1 : 2][kCPT];
  auto load_tile = [&](int ka, int set) { stager.load(kr[set], krs, vrs, d, vd, ka, nk); };
  auto store_tile = [&](int slot, int set) {
    stager.store(smem + slot * S::kSlot + S::offKT, smem + slot * S::kSlot + S::offVT, kr[set]);
  };
  floatx16 dq[kDO / 32];
#pragma unroll
  for (int u = 0; u < kDO / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[u][i] = 0.f;

  // A-operand (Kᵀ / Vᵀ) read bases: lane 4q+p of a 16-lane group supplies channel row q, keys
  // 4σ(p)..4σ(p)+3 (σ swaps 1 and 2), so register i of Sᵀ / dPᵀ half t holds key 32t + 16(i>>3) +
  // 8h + (i&7): k-step s of dSᵀ is keys 16s + 8h + 0..7 and K's dQ A operand is one b128 row read
  const int sig = ((tp & 1) << 1) | (tp >> 1);
  uint32_t tb[2][2];  // [e][t], row 8(g>>1) + 4e + tq (+16s: immediate)
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int t = 0; t < 2; ++t) tb[e][t] = k2_off(8 * (g >> 1) + 4 * e + tq, 4 * t + 2 * (g & 1) + (sig >> 1), sig & 1);
  uint32_t kb2[4];  // dQ A operand: row 32u + r (+32u·128: immediate), chunk 2s + h
#pragma unroll
  for (int s = 0; s < 4; ++s) kb2[s] = k2_off(r, 2 * s + h);

  // unconditional (with no tiles it moves zeros): a conditional load here left hipcc's vmcnt
  // state merged, and the loop's first step then drained every load in flight
  load_tile(kt0, 0);
  store_tile(0, 0);
  if constexpr (!ONESET) {
    load_tile(kt0 + kBN, 1);
    load_tile(kt0 + 2 * kBN, 0);
  }

  auto step = [&](auto P_, int it) {
    constexpr int p = decltype(P_)::value;
    __syncthreads();
    const int ka = kt0 + it * kBN;
    const int cls = it < ntiles ? tcls(ka) : 0;  // (the loop's last pair may end on a phantom step)
    // unconditional (past the end they move zeros into a slot nobody reads): exact vmcnt waits
    if constexpr (ONESET) {
      load_tile(ka + kBN, 0);
    } else {
      store_tile(p ^ 1, p ^ 1);
      load_tile(ka + 3 * kBN, p ^ 1);
    }
    struct StoreAtExit {  // ONESET: tile it+1 into slot p^1 after this step's MFMAs (on every return)
      decltype(store_tile)& f;
      __device__ ~StoreAtExit() { if constexpr (ONESET) f(p ^ 1, 0); }
    } store_at_exit{store_tile};
    if (cls == 0) return;
    const lds_char_t* base = smem + p * S::kSlot;
    floatx16 st[2], dp[2];
    // PRE: every operand read two MFMA pairs ahead of its MFMAs (one wave per SIMD: nothing else
    // hides an LDS round trip between a read and the MFMA that consumes it)
    half8 ka8p[3];
    auto rka = [&](int n) __attribute__((always_inline)) {  // dQ operand n = (kDO/32)·s + u
      ka8p[n % 3] = read_b128(base + S::offKT + kb2[n / (kDO / 32)] + 32 * (ou0 + n % (kDO / 32)) * 128);
    };
    if constexpr (PRE) {
      constexpr int kN = 2 * (D / 16);
      half8 kf[3], vf[3];
      auto rd = [&](int n) __attribute__((always_inline)) {  // n = 2s + t
        const int s_ = n >> 1, t = n & 1;
        const uint32_t b0 = tb[0][t] + (16 * s_) * 128, b1 = tb[1][t] + (16 * s_) * 128;
        kf[n % 3].lo = tr_read(base + S::offKT + b0);
        kf[n % 3].hi = tr_read(base + S::offKT + b1);
        vf[n % 3].lo = tr_read(base + S::offVT + b0);
        vf[n % 3].hi = tr_read(base + S::offVT + b1);
      };
      rd(0);
      rd(1);
#pragma unroll
      for (int n = 0; n < kN; ++n) {
        if (n + 2 < kN) rd(n + 2);
        if (n == kN - 2) rka(0);
        if (n == kN - 1) rka(1);
        const int s_ = n >> 1, t = n & 1;
        st[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[n % 3], qf[s_], s_ == 0 ? negl : st[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[n % 3], of[s_], s_ == 0 ? negd : dp[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < (PRE ? 0 : D / 16); ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        half8 kf, vf;
        const uint32_t b0 = tb[0][t] + (16 * s) * 128, b1 = tb[1][t] + (16 * s) * 128;
        kf.lo = tr_read(base + S::offKT + b0);
        kf.hi = tr_read(base + S::offKT + b1);
        vf.lo = tr_read(base + S::offVT + b0);
        vf.hi = tr_read(base + S::offVT + b1);
        st[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], s == 0 ? negl : st[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, of[s], s == 0 ? negd : dp[t], 0, 0, 0);
      }
    // dSᵀ = exp2(Sᵀ)∘dPᵀ; keys of register i of half t: 32t + 16(i>>3) + 8h + (i&7)
    auto dsq = [&](int cl) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      half8 dsf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = s >> 1, i = 8 * (s & 1) + j;
        const float pv = masked_exp2_k<POL>(st[t][i], cl == 1, i, ka + 32 * t, h, klo, kspan, nk, a.rule, qo);
        dsf[j] = (_Float16)(pv * dp[t][i]);
      }
#pragma unroll
      for (int u = 0; u < kDO / 32; ++u) {
        if constexpr (PRE) {
          const int n = (kDO / 32) * s + u;
          if (n + 2 < 4 * (kDO / 32)) rka(n + 2);
          dq[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka8p[n % 3], dsf, dq[u], 0, 0, 0);
        } else {
          const half8 ka8 = read_b128(base + S::offKT + kb2[s] + 32 * (ou0 + u) * 128);
          dq[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka8, dsf, dq[u], 0, 0, 0);
        }
      }
    }
    };
    // the edge-tile mask as a real branch (see bwd_dkdv_pc_kernel, fa_bwd_f16_fast.hip; MSPEC: the if-converted form)
    if constexpr (MSPEC) {
      dsq(cls);
    } else if (cls == 1) {
      asm volatile("; edge tile" ::: );
      dsq(1);
    } else {
      asm volatile("; interior tile" ::: );
      dsq(2);
    }
  };
  for (int it = 0; it < ntiles; it += 2) {  // whole pairs (see bwd_dkdv_kernel, fa_bwd_f16_fast.hip)
    step(IC<0>{}, it);
    step(IC<1>{}, it + 1);
  }

  if (!wave_active || qi >= nq) return;
  if constexpr (SPLIT) {
    // the unscaled fp32 partial of (slice, chunk), bid = slice * nchunks + chunk: record [d][nq],
    // lanes along nq so the stores coalesce; the reduce kernel scales and rounds
    float* rec = args.ws_part + (int64_t)bid * d * nq;
#pragma unroll
    for (int u = 0; u < kDO / 32; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (c < d) rec[(int64_t)c * nq + qi] = dq[u][i];
      }
    return;
  }
  __half* dQ = static_cast<__half*>(a.dQ) + bi * (int64_t)d * nq;
  const float sc = (float)a.scale;
  store_grad<D, kDO / 32>({{dq, dQ, d, sc}}, nq, qi, h, ou0);
}

// dQ of the split form: one thread per (slice, channel, query), queries fastest.  The chunk partials
// are added in chunk order in fp32 (no atomics: the result is deterministic and a slice's bits do not
// depend on the batch), then scaled and rounded as the unsplit epilogue does.  The loads of a group
// of eight chunks are issued together; only the additions are a chain.
__global__ __launch_bounds__(256) void dq_split_reduce_kernel(BwdSplitArgs sa) {
  const BwdArgs& a = sa.b;
  const int nc = sa.nchunks;
  const int64_t per = (int64_t)a.d * a.rule.q.n;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bi = gid / per;
  const float* part = sa.ws_part + bi * nc * per + (gid - bi * per);
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
  static_cast<__half*>(a.dQ)[gid] = __float2half(sum * (float)a.scale);
}

// ---------------------------------------------------------------------------
// dQ, producer / consumer (two waves per SIMD): the dK/dV pass's split applied to the query-outer
// pass.  Waves w and w+4 share a SIMD and the same 32 queries.  Wave w (producer) keeps Q' and dO
// resident, forms Sᵀ = Kᵀ·Q' and dPᵀ = Vᵀ·dO for key tile i one 32-key half at a time and
// dSᵀ = exp2(Sᵀ)∘dPᵀ, and hands dSᵀ to wave w+4 through LDS (four lane-linear b128 per lane);
// wave w+4 (consumer) stages the key tiles and accumulates dQ += K·dSᵀ for tile i-1.  The
// one-wave-per-SIMD pass above (332-345 registers) serialises its softmax and every LDS round trip
// behind its own MFMAs; here the producer's softmax runs beside the consumer's MFMAs and staging.
// Ring: four K/V slots (tile t in slot t % 4), two hand-over slots, one barrier per step;
// 4 x 32 KB + 32 KB = 160 KB at D = 128.
template <int D>
struct DqPcSmem {
  static constexpr int kBM = 128;           // queries per workgroup: four producer waves x 32
  static constexpr int kRow = D * kBM * 2;  // Q (or dO) row image (prologue only)
  static constexpr int kKT = D * 128;       // one [D][64] K2 image
  static constexpr int offKT = 0, offVT = kKT;
  static constexpr int kSlot = 2 * kKT;
  static constexpr int kNS = 4;
  static constexpr int offX = kNS * kSlot;  // dSᵀ hand-over: 2 slots x 4 waves x 4 KB
  static constexpr int kXWave = 4096, kXSlot = 4 * kXWave;
  static constexpr int kUsed = offX + 2 * kXSlot;
  static constexpr int kTotal = kUsed > 2 * kRow ? kUsed : 2 * kRow;  // the Q/dO images alias the ring
};

template <int D, int POL, bool ALN>
__global__ __launch_bounds__(512, 1) void bwd_dq_pc_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  using S = DqPcSmem<D>;
  constexpr int kThr = 512, kHalfThr = 256;  // one half of the workgroup stages
  constexpr int kBM = S::kBM, kBN = 64;
  constexpr int kKChunks = D * 8;  // 16-B chunks of one [D][64] tile
  static_assert((2 * kKChunks) % kHalfThr == 0, "tile chunks must divide over the staging waves");
  constexpr int kCPT = 2 * kKChunks / kHalfThr;  // K and V chunks per staging thread
  constexpr float kNegInf = -__builtin_huge_valf();

  const int nq = a.rule.q.n, nk = a.rule.k.n;
  const uint32_t nqb = (nq + kBM - 1) / kBM;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t bi = bid / nqb;
  const int q0 = (int)(nqb - 1 - (bid % nqb)) * kBM;  // latest (heaviest under causal) blocks first
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w >> 2, wl = w & 3;  // group 0 produces, group 1 consumes; wl: the query slice
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  const float c2 = (float)a.scale * kLog2e;
  const int d = a.d, vd = a.v_d;
  const __half* Q = static_cast<const __half*>(a.Q) + bi * (int64_t)d * nq;
  const __half* dO = static_cast<const __half*>(a.dO) + bi * (int64_t)vd * nq;

  const int wq0 = q0 + 32 * wl;
  const int qi = wq0 + r;
  const bool wave_active = wq0 < nq;

  // ---- Q, dO blocks into LDS (every thread); the producers read their resident B operands below
  stage_resident<D, kBM, kThr, ALN>(smem, Q, dO, d, vd, nq, q0, tid);
  __syncthreads();

  // ---- key range of this query block (rule-bounded), per-lane / per-wave key intervals (both roles)
  const int qlast = min(q0 + kBM, nq) - 1;
  int kb = 0, ke = nk;
  if (POL != 0) k_range_for_q_block(a.rule, q0, qlast, &kb, &ke);
  const int kt0 = (kb / kBN) * kBN;
  const int ntiles = (ke > kb) ? (ke - kt0 + kBN - 1) / kBN : 0;
  int klo = 0, kspan = nk, wlo_min = 0, wlo_max = 0, whi_min = nk - 1, whi_max = nk - 1;
  if (POL == 1 && wave_active) {
    int khi;
    key_interval(a.rule, min(qi, nq - 1), &klo, &khi);
    kspan = max(khi - klo + 1, 0);
    const int last = min(31, nq - 1 - wq0);
    wave_interval_ends(klo, khi, last, wlo_min, whi_min, wlo_max, whi_max);
  }
  const QueryWaveClass<POL, kBN> tcls{wave_active, nk, a.rule, wq0, nq, wlo_min, whi_max, wlo_max, whi_min};
  // hand-over slot of this wave pair: k-steps 0..3 of dSᵀ, one b128 each, lane-linear
  auto xoff = [&](int xs, int j) -> uint32_t { return S::offX + xs * S::kXSlot + wl * S::kXWave + j * 1024 + lane * 16; };
  // Steps it = 0 .. ntiles: the producer handles tile it (it < ntiles), the consumer tile it-1 (it >= 1),
  // in whole groups of four (ring slot it % 4, staging set (it+1) % 2, hand-over slot it % 2 compile-time)
  const int nsteps = ntiles + 1;

  // ---- key-tile staging (K, V chunks: 8 keys of one channel row) by the consumer half of the workgroup
  const int ct = tid & (kHalfThr - 1);
  const __amdgpu_buffer_rsrc_t krs = make_rsrc(static_cast<const __half*>(a.K) + bi * (int64_t)d * nk, 2u * d * nk);
  const __amdgpu_buffer_rsrc_t vrs = make_rsrc(static_cast<const __half*>(a.V) + bi * (int64_t)vd * nk, 2u * vd * nk);
  using Stager = TileStager<D, kHalfThr, 8, ALN>;
  const Stager stager(ct, nk);
  u32x4 kr[2][kCPT];  // two staging sets: tile t in set t&1, loaded two steps before it is stored
  auto load_tile = [&](int ka, int set) __attribute__((always_inline)) { stager.load(kr[set], krs, vrs, d, vd, ka, nk); };
  auto store_tile = [&](int slot, int set) __attribute__((always_inline)) {
    stager.store(smem + slot * S::kSlot + S::offKT, smem + slot * S::kSlot + S::offVT, kr[set]);
  };
  // first tiles (after tile 0's loads): the barrier that retires the Q / dO images, tile 0 stored
  auto stage0 = [&]() __attribute__((always_inline)) {
    __syncthreads();
    store_tile(0, 0);
    load_tile(kt0 + kBN, 1);
    load_tile(kt0 + 2 * kBN, 0);
  };
  // the row constants of the producer's resident operands (this lane's query)
  auto rowconst = [&](const void* ws, float dflt) -> floatx16 {
    const float* p = static_cast<const float*>(ws) + bi * (int64_t)nq;
    const float v = (qi < nq) ? p[qi] : dflt;
    floatx16 x;
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = v;
    return x;
  };
  // A-operand (Kᵀ / Vᵀ) read bases, σ-permuted as in the one-wave pass: register i of half t holds
  // key 32t + 16(i>>3) + 8h + (i&7), so k-step s of dSᵀ is keys 16s + 8h + 0..7
  const int sig = ((tp & 1) << 1) | (tp >> 1);
  uint32_t tb[2][2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int t = 0; t < 2; ++t) tb[e][t] = k2_off(8 * (g >> 1) + 4 * e + tq, 4 * t + 2 * (g & 1) + (sig >> 1), sig & 1);
  // Sᵀ (or dPᵀ) of key half t: 8 MFMAs over the channels, transposed A reads two k-steps ahead
  auto half_chain = [&](const lds_char_t* img, const half8* bres, floatx16 init, int t) __attribute__((always_inline)) -> floatx16 {
    constexpr int kS = D / 16;
    half8 af[3];
    auto rd = [&](int s_) __attribute__((always_inline)) {
      af[s_ % 3].lo = tr_read(img + tb[0][t] + (16 * s_) * 128);
      af[s_ % 3].hi = tr_read(img + tb[1][t] + (16 * s_) * 128);
    };
    rd(0);
    rd(1);
    floatx16 acc = init;
#pragma unroll
    for (int s_ = 0; s_ < kS; ++s_) {
      if (s_ + 2 < kS) rd(s_ + 2);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s_ % 3], bres[s_], acc, 0, 0, 0);
    }
    return acc;
  };
  const int qo = (POL == 2) ? seq_order(a.rule.q, a.rule, min(qi, nq - 1)) : 0;  // this lane's query order

  if (grp == 0) {
    // ================= producer
    half8 qf[D / 16];
    read_resident<D, kBM>(smem, wl, g, tq, tp, qf);  // lane (r,h) holds Q'[c = 16s + 8h + j][q = wq0 + r]
#pragma unroll
    for (int s = 0; s < D / 16; ++s) qf[s] = scale8(qf[s], c2);
    const floatx16 negl = rowconst(a.ws_lse, kNegInf);
    {
      half8 of[D / 16];
      read_resident<D, kBM>(smem + S::kRow, wl, g, tq, tp, of);
      const floatx16 negd = rowconst(a.ws_D, 0.f);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __syncthreads();  // (stage0 of the consumers)
      auto pstep = [&](auto C_, int it) __attribute__((always_inline)) {
        constexpr int c = decltype(C_)::value;
        __syncthreads();
        const int ka = kt0 + it * kBN;
        const int cls = it < ntiles ? tcls(ka) : 0;
        if (cls == 0) return;
        const lds_char_t* base = smem + c * S::kSlot;
#pragma unroll
        for (int t = 0; t < 2; ++t) {  // one 32-key half at a time: 16 MFMAs, then its two dSᵀ k-steps
          const floatx16 st = half_chain(base + S::offKT, qf, negl, t);
          const floatx16 dp = half_chain(base + S::offVT, of, negd, t);
          auto softmax = [&](int cl) __attribute__((always_inline)) {
#pragma unroll
            for (int sh = 0; sh < 2; ++sh) {
              half8 dsf;
#pragma unroll
              for (int j = 0; j < 8; ++j)
                dsf[j] = (_Float16)(masked_exp2_k<POL>(st[8 * sh + j], cl == 1, 8 * sh + j, ka + 32 * t, h, klo, kspan, nk, a.rule, qo) *
                                    dp[8 * sh + j]);
              *reinterpret_cast<lds_half8_t*>(smem + xoff(c % 2, 2 * t + sh)) = dsf;
            }
          };
          // the edge-tile mask as a real branch (see bwd_dkdv_pc_kernel, fa_bwd_f16_fast.hip)
          if (cls == 1) {
            asm volatile("; edge tile" ::: );
            softmax(1);
          } else {
            asm volatile("; interior tile" ::: );
            softmax(2);
          }
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
  }

  // ================= consumer: dQ += K·dSᵀ for tile it-1; it stages the key tiles
  load_tile(kt0, 0);
  stage0();
  floatx16 dq[D / 32];
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[u][i] = 0.f;
  uint32_t kb2[4];  // dQ A operand: row 32u + r (+32u·128: immediate), chunk 2s + h
#pragma unroll
  for (int s = 0; s < 4; ++s) kb2[s] = k2_off(r, 2 * s + h);

  auto cwork = [&](auto C_, int it) __attribute__((always_inline)) {
    constexpr int c = decltype(C_)::value;
    const int ka = kt0 + (it - 1) * kBN;
    const int cls = (it >= 1 && it - 1 < ntiles) ? tcls(ka) : 0;
    if (cls == 0) return;
    const lds_char_t* base = smem + ((c + 3) % 4) * S::kSlot;
    half8 dsf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) dsf[s] = read_b128(smem + xoff((c + 1) % 2, s));
    constexpr int kN = 4 * (D / 32);
    half8 ka8p[3];
    auto rka = [&](int n) __attribute__((always_inline)) {  // operand n = (D/32)·s + u, two ahead
      ka8p[n % 3] = read_b128(base + S::offKT + kb2[n / (D / 32)] + 32 * (n % (D / 32)) * 128);
    };
    rka(0);
    rka(1);
#pragma unroll
    for (int n = 0; n < kN; ++n) {
      if (n + 2 < kN) rka(n + 2);
      const int s = n / (D / 32), u = n % (D / 32);
      dq[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka8p[n % 3], dsf[s], dq[u], 0, 0, 0);
    }
  };
  // one step: the barrier, tile it+1 stored (loaded in step it-2), tile it+3 loaded into the set just
  // stored (unconditional: past the end they move zeros into a slot nobody reads, so the vmcnt waits
  // stay exact), then dQ += K·dSᵀ of tile it-1
  auto cstep = [&](auto C_, int it) __attribute__((always_inline)) {
    constexpr int c = decltype(C_)::value;
    __syncthreads();
    store_tile((c + 1) % 4, (c + 1) % 2);
    load_tile(kt0 + kBN * (it + 3), (c + 1) % 2);
    cwork(C_, it);
  };
  for (int it = 0; it < nsteps; it += 4) {
    cstep(IC<0>{}, it);
    cstep(IC<1>{}, it + 1);
    cstep(IC<2>{}, it + 2);
    cstep(IC<3>{}, it + 3);
  }

  if (!wave_active || qi >= nq) return;
  __half* dQ = static_cast<__half*>(a.dQ) + bi * (int64_t)d * nq;
  const float sc = (float)a.scale;
  store_grad<D, D / 32>({{dq, dQ, d, sc}}, nq, qi, h, 0);
}
template <int D, int NW, int WPE, bool PRE = false, bool MSPEC = false>
hipError_t launch_dq(const BwdArgs& a, hipStream_t s) {
  using S = DqSmem<D, NW>;
  const int64_t nqb = (a.rule.q.n + S::kBM - 1) / S::kBM;
  return launch_smem(
      with_pol_aln(a, [](auto pol, auto aln) { return &bwd_dq_kernel<D, NW, WPE, pol.value, aln.value, PRE, MSPEC>; }),
      (unsigned)(a.b * nqb), NW * 64, S::kTotal, s, a);
}

// the same pass on one workgroup per (slice, key chunk), then the reduce over the chunks.  WPEU: the
// launch bound of the element-wise staging instances (at D = 64 under two waves per SIMD they spill
// 8-336 bytes a lane once the tile base is a chunk's, as the unsplit ones do by 16-40; one wave per
// SIMD holds them in registers)
template <int D, int NW, int WPE, int WPEU, bool PRE = false, bool MSPEC = false>
hipError_t launch_dq_split(const BwdSplitArgs& sa, hipStream_t s) {
  const BwdArgs& a = sa.b;
  const hipError_t e = launch_smem(
      with_pol_aln(a, [](auto pol, auto aln) {
        return &bwd_dq_kernel<D, NW, aln.value ? WPE : WPEU, pol.value, aln.value, PRE, MSPEC, 1, false, true>;
      }),
      (unsigned)(a.b * sa.nchunks), NW * 64, DqSmem<D, NW>::kTotal, s, sa);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.d * a.rule.q.n;
  hipLaunchKernelGGL(dq_split_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, sa);
  return hipGetLastError();
}

template <int D>
hipError_t launch_dq_pc(const BwdArgs& a, hipStream_t s) {
  using S = DqPcSmem<D>;
  const int64_t nqb = (a.rule.q.n + S::kBM - 1) / S::kBM;
  return launch_smem(with_pol_aln(a, [](auto pol, auto aln) { return &bwd_dq_pc_kernel<D, pol.value, aln.value>; }),
                     (unsigned)(a.b * nqb), 512, S::kTotal, s, a);
}

}  // namespace

// The dQ pass for max(d, v_d) <= 128.  d <= 64: the one-wave pass, two waves per SIMD, with the
// if-converted edge mask (the branch form spills 8-42 VGPRs there).  d = 128, tuned on c3: for 16-B chunk
// staging the producer / consumer pass (8.58 -> 8.36 ms backward, gradients bit-identical); its
// element-wise staging form spills, so other shapes keep the one-wave pass with operand reads two MFMA
// pairs ahead (10.97 -> 9.93 ms backward before).
// variant (diagnostic library, FA_BWD_VARIANT): d <= 64 — 82 eight-wave blocks, 1068 / 1069 the operand
// reads run ahead, 1071 the edge mask as a branch; d = 128 — 1599 the one-wave pass on aligned shapes.
hipError_t launch_bwd_f16_dq(const BwdArgs& a, hipStream_t s, int variant) {
  (void)variant;
  if (max(a.d, a.v_d) <= 64) {
#ifdef FA_DIAG
    switch (variant) {
      case 82: return launch_dq<64, 8, 2, false, true>(a, s);
      case 1068: case 1069: return launch_dq<64, 4, 2, true>(a, s);
      case 1071: return launch_dq<64, 4, 2>(a, s);
      default: break;
    }
#endif
    return launch_dq<64, 4, 2, false, true>(a, s);
  }
#ifdef FA_DIAG
  if (variant == 1599) return launch_dq<128, 4, 1, true>(a, s);
#endif
  if (bwd_aligned(a)) return launch_dq_pc<128>(a, s);
  return launch_dq<128, 4, 1, true>(a, s);
}

// One query block against a long key range: the one-wave pass split over key chunks and its reduce (the
// producer / consumer pass holds 160 KB of LDS, one workgroup a CU, and is not split: few queries need
// occupancy, not the per-workgroup MFMA rate)
hipError_t launch_bwd_f16_dq_split(const BwdSplitArgs& sa, hipStream_t s) {
  if (max(sa.b.d, sa.b.v_d) <= 64) return launch_dq_split<64, 4, 2, 1, false, true>(sa, s);
  return launch_dq_split<128, 4, 1, 1, true>(sa, s);
}

#ifdef FA_DIAG
// round 4's D = 256 dQ pass: two 128-channel chunks, Sᵀ / dPᵀ formed in each, one staging set (16-B chunk staging)
hipError_t launch_bwd_f16_dq_oc2(const BwdArgs& a, hipStream_t s) {
  using S = DqSmem<256, 4>;
  const int64_t nqb = (a.rule.q.n + S::kBM - 1) / S::kBM;
  const int pol = bwd_pol(a.rule);
  return launch_smem(pol == 0   ? bwd_dq_kernel<256, 4, 1, 0, true, false, false, 2, true>
                     : pol == 1 ? bwd_dq_kernel<256, 4, 1, 1, true, false, false, 2, true>
                                : bwd_dq_kernel<256, 4, 1, 2, true, false, false, 2, true>,
                     (unsigned)(a.b * nqb * 2), 256, S::kTotal, s, a);
}
#endif

}  // namespace fa
