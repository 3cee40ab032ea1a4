// fa_fwd_f16_splitk.hip — split-key fp16 forward for few queries and many keys (gfx950 MFMA).
//
// Every other forward gives one workgroup a (slice, query block) and walks the keys inside it,
// which leaves the GPU empty when a slice has one query block and a long key range (b = 16,
// nq <= 128, nk = 16384: 16 workgroups on 256 CUs).  Here the rule-bounded key range of the
// single query block is cut into chunks (fa_api.hip: split_plan):
//   * splitk_partial_kernel: one workgroup per (slice, chunk) runs the key loop of
//     fwd_f16_kernel (fa_fwd_f16.hip: same staging, transposed scores, log2-domain online
//     softmax, tile classes, three POL forms) over its chunk only and writes the UNNORMALISED
//     fp32 accumulator with its statistics to the workspace;
//   * splitk_merge_kernel: folds the chunks of a query in fixed order (no atomics, so the result
//     is deterministic and independent of the batch) into the usual O, l, m.
// Workspace record of one (slice, chunk): (v_d + 3) rows of nq floats — O[v_d][nq] relative to
// m_run, then m_run[nq] (log2 units; -inf where the row attends nothing in the chunk), l[nq]
// and the exact row max m_max[nq].
#include "fa_device.h"
#include "fa_kernels.h"

namespace fa {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef short v4i16 __attribute__((__vector_size__(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16_t;
typedef __attribute__((address_space(3))) char lds_char_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
typedef __attribute__((address_space(3))) u32x2 lds_u32x2_t;

constexpr int kBN = 64;      // keys per tile
constexpr int kNW = 4;       // waves per workgroup: one query block of 128 rows
constexpr int kBM = 32 * kNW;
constexpr int kThr = 64 * kNW;
constexpr int kVPad = 2;     // V slab row padding, in 8-byte rows
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kRescaleThr = 8.f;  // log2 units, as in fwd_f16_kernel

// value of lane l^32
__device__ __forceinline__ float xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// LDS layout of fwd_f16_kernel: Q [D][128] aliases a 3-slot ring of K [D][64] / V [16][D+pad][4] tiles
template <int D>
struct Smem {
  static constexpr int kQRow = 2 * kBM;
  static constexpr int kQ = D * kQRow;
  static constexpr int kK = D * kBN * 2;
  static constexpr int kV = 16 * (D + kVPad) * 8;
  static constexpr int kBuf = kK + kV;
  static constexpr int kNBuf = 3;
  static constexpr int kTotal = (kNBuf * kBuf > kQ) ? kNBuf * kBuf : kQ;
};

__device__ __forceinline__ half4 tr_read(const lds_char_t* base, uint32_t off) {
  const v4i16 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t*)(base + off));
  return __builtin_bit_cast(half4, t);
}

__device__ __forceinline__ half4 read_b64(const lds_char_t* base, uint32_t off) {
  return *reinterpret_cast<const __attribute__((address_space(3))) half4*>(base + off);
}

__device__ __forceinline__ u32x4 load16(const __half* p) { return *reinterpret_cast<const u32x4*>(p); }

// 8 consecutive halfs starting at element `e` of a row of length n (zero past n).
__device__ __forceinline__ u32x4 load_chunk(const __half* row, int e, int n, bool vec) {
  if (vec) return (e < n) ? load16(row + e) : u32x4{0, 0, 0, 0};
  unsigned short h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (e + j < n) ? __half_as_ushort(row[e + j]) : (unsigned short)0;
  return u32x4{h[0] | (uint32_t(h[1]) << 16), h[2] | (uint32_t(h[3]) << 16), h[4] | (uint32_t(h[5]) << 16),
               h[6] | (uint32_t(h[7]) << 16)};
}

// One workgroup = 4 waves = the (single) query block of one slice x one key chunk.
//   POL / FAST as in fwd_f16_kernel: 0 full, 1 interval rules, 2 per-element rule check;
//   FAST = d == v_d == D with 16-byte aligned K/V rows (unguarded dwordx4 staging).
// All four waves stage K/V whatever nq is; waves whose 32 query rows lie past nq run no MFMA, so
// at nq <= 32 one wave computes and the other three only keep loads in flight.
template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kThr, D >= 128 ? 1 : 2) void splitk_partial_kernel(SplitArgs sa) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char_t* smem = (lds_char_t*)smem_raw;
  using S = Smem<D>;
  const FwdArgs& a = sa.f;
  constexpr int kChunks = D * 8;                                   // 16-B chunks per K (or V) tile
  constexpr int kCPT = (kChunks + kThr - 1) / kThr;                // chunks per thread
  constexpr float kNegInf = -__builtin_huge_valf();

  const int nq = a.rule.q.n, nk = a.rule.k.n, d = FAST ? D : a.d, vd = FAST ? D : a.v_d;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t bi = bid / (uint32_t)sa.nchunks;
  const int ch = (int)(bid % (uint32_t)sa.nchunks);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;  // tr-read lane roles

  const __half* Q = static_cast<const __half*>(a.Q) + bi * (int64_t)d * nq;
  const __half* K = static_cast<const __half*>(a.K) + bi * (int64_t)d * nk;
  const __half* V = static_cast<const __half*>(a.V) + bi * (int64_t)vd * nk;
  const bool qvec = ((nq & 7) == 0) && ((reinterpret_cast<uintptr_t>(a.Q) & 15) == 0);
  const float c2 = (float)a.scale * kLog2e;

  // ---- this chunk's share [kt0, ce) of the block's key range (kt0 is tile-aligned)
  const int kt0 = sa.k_first + ch * sa.chunk;
  const int ce = min(kt0 + sa.chunk, sa.k_end);
  const int ntiles = (ce - kt0 + kBN - 1) / kBN;

  // ---- register staging of one K/V tile (16-B chunks; chunk = 8 keys of one channel row)
  auto load_into = [&](u32x4 (&kr)[kCPT], u32x4 (&vr)[kCPT], int k0) {
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      const int idx = tid + kThr * j, c = idx >> 3, m = idx & 7;
      const bool in = (kChunks % kThr == 0) || idx < kChunks;
      const int e = k0 + 8 * m;
      if (FAST && (kChunks % kThr == 0) && k0 + kBN <= nk) {  // whole tile in range: unguarded
        kr[j] = load16(K + (int64_t)c * nk + e);
        vr[j] = load16(V + (int64_t)c * nk + e);
      } else if (FAST) {
        kr[j] = (in && e < nk) ? load16(K + (int64_t)c * nk + e) : u32x4{0, 0, 0, 0};
        vr[j] = (in && e < nk) ? load16(V + (int64_t)c * nk + e) : u32x4{0, 0, 0, 0};
      } else {
        kr[j] = (in && c < d) ? load_chunk(K + (int64_t)c * nk, e, nk, false) : u32x4{0, 0, 0, 0};
        vr[j] = (in && c < vd) ? load_chunk(V + (int64_t)c * nk, e, nk, false) : u32x4{0, 0, 0, 0};
      }
    }
  };
  auto store_from = [&](const u32x4 (&kr)[kCPT], const u32x4 (&vr)[kCPT], int buf) {
    lds_char_t* kbuf = smem + buf * S::kBuf;
    lds_char_t* vbuf = kbuf + S::kK;
#pragma unroll
    for (int j = 0; j < kCPT; ++j) {
      const int idx = tid + kThr * j, c = idx >> 3, m = idx & 7;
      if ((kChunks % kThr == 0) || idx < kChunks) {
        // K: [c][64 keys], 64-B halves swapped on rows with c&2 (conflict-free tr reads)
        *reinterpret_cast<lds_u32x4_t*>(kbuf + c * 128 + ((m * 16) ^ ((c & 2) << 5))) = kr[j];
        // V: [key/4][v][4] slabs -> the PV operand is a plain conflict-free ds_read_b64
        *reinterpret_cast<lds_u32x2_t*>(vbuf + ((2 * m) * (D + kVPad) + c) * 8) = vr[j].xy;
        *reinterpret_cast<lds_u32x2_t*>(vbuf + ((2 * m + 1) * (D + kVPad) + c) * 8) = vr[j].zw;
      }
    }
  };
  // prologue loads of tiles 0 and 1 are in flight together with the Q tile
  u32x4 kreg[kCPT], vreg[kCPT], kreg1[kCPT], vreg1[kCPT];
  if (ntiles > 0) load_into(kreg, vreg, kt0);
  if (ntiles > 1) load_into(kreg1, vreg1, kt0 + kBN);

  // ---- Q tile [D][BM] -> LDS (64-B blocks XOR-swizzled by c&3: conflict-free tr reads)
  for (int idx = tid; idx < D * (kBM / 8); idx += kThr) {
    const int c = idx / (kBM / 8), m = idx % (kBM / 8);
    u32x4 v = {0, 0, 0, 0};
    if (c < d) v = load_chunk(Q + (int64_t)c * nq, 8 * m, nq, qvec);
    *reinterpret_cast<lds_u32x4_t*>(smem + c * S::kQRow + ((m * 16) ^ ((c & 3) << 6))) = v;
  }
  __syncthreads();
  // Q*scale*log2(e) as the B operand of Sᵀ = Kᵀ·Q: lane (r,h) holds Q[c = 16s + 8h + j][q = 32w + r]
  half8 qf[D / 16];
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

  const int wq0 = 32 * w;
  const int wq1 = min(wq0 + 31, nq - 1);
  const bool wave_active = wq0 < nq;
  const int qi = wq0 + r;
  const int qo = (POL == 2 && qi < nq) ? seq_order(a.rule.q, a.rule, qi) : 0;
  // POL 1 (interval rules): this lane's allowed keys [klo, klo + kspan) and the wave's bounds
  int klo = 0, kspan = 0, wlo_min = 0, wlo_max = 0, whi_min = 0, whi_max = 0;
  if (POL == 1 && wave_active) {
    int khi;
    key_interval(a.rule, min(qi, nq - 1), &klo, &khi);
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
    if (POL == 0) return k1 < nk ? 2 : 1;
    if (POL == 1) {
      if (wlo_min > k1 || whi_max < k0) return 0;
      return (wlo_max <= k0 && whi_min >= k1) ? 2 : 1;
    }
    const int c = tile_class(a.rule, wq0, wq1, k0, min(k1, nk - 1));
    return (c == 2 && k1 >= nk) ? 1 : c;
  };

  auto load_tile = [&](int k0) { load_into(kreg, vreg, k0); };
  auto store_tile = [&](int buf) { store_from(kreg, vreg, buf); };

  floatx16 acc_o[D / 32];
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_o[u][i] = 0.f;
  // m_run: lazily updated softmax reference (log2 units) that l_run / acc_o are relative to;
  // negm = -m_run broadcast (the C operand of every Sᵀ chain); m_max: exact row max.
  float m_run = 0.f, l_run = 0.f, m_max = kNegInf;
  bool m_set = false;
  floatx16 negm;
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

  // Rule/tail mask, row max and (lazy) rebase of the scores of the tile at k0
  auto prepare = [&](int k0, int cls, floatx16 (&st)[2], floatx16 (&nxt)[2], bool has_next) {
    if (cls == 1) {  // mixed / tail tile: per-element mask
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
            ok = key < nk;
            if (POL == 2) ok &= check_orders_bf(a.rule, qo, seq_order(a.rule.k, a.rule, key));
          }
          st[t][i] = ok ? st[t][i] : kNegInf;
        }
    }
    float mt;
    {
      float mx0 = fmaxf(st[0][0], st[0][1]), mx1 = fmaxf(st[1][0], st[1][1]);
#pragma unroll
      for (int i = 2; i < 16; i += 2) {
        mx0 = fmaxf(fmaxf(mx0, st[0][i]), st[0][i + 1]);
        mx1 = fmaxf(fmaxf(mx1, st[1][i]), st[1][i + 1]);
      }
      mt = fmaxf(mx0, mx1);
      mt = fmaxf(mt, xor32(mt));  // tile row max relative to m_run
    }
    m_max = fmaxf(m_max, m_run + mt);
    // lazy rescale: move m_run only when the tile max exceeds it by more than kRescaleThr, or to seed it
    const bool seed = !m_set && (mt != kNegInf);
    if (__any((mt > kRescaleThr) | seed)) {
      const float delta = m_set ? fmaxf(mt, 0.f) : (seed ? mt : 0.f);
      const float alpha = m_set ? __builtin_amdgcn_exp2f(-delta) : 1.f;
      m_run += delta;
      m_set = m_set || seed;
      l_run *= alpha;
#pragma unroll
      for (int u = 0; u < D / 32; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc_o[u][i] *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[0][i] -= delta;
        st[1][i] -= delta;
        negm[i] = -m_run;
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

  // P = exp2(st) (fp16) as the B operand of Oᵀ = V·Pᵀ, row sums (v_dot2_f32_f16), and the PV MFMAs
  auto exp_pv = [&](floatx16 (&st)[2], int buf) {
    const lds_char_t* vbuf = smem + buf * S::kBuf + S::kK;
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const half2v one2 = {(_Float16)1.f, (_Float16)1.f};
    float ls0 = 0.f, ls1 = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      half8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (_Float16)__builtin_amdgcn_exp2f(st[s >> 1][8 * (s & 1) + j]);
#pragma unroll
      for (int j = 0; j < 8; j += 4) {
        ls0 = __builtin_amdgcn_fdot2(half2v{pf[j], pf[j + 1]}, one2, ls0, false);
        ls1 = __builtin_amdgcn_fdot2(half2v{pf[j + 2], pf[j + 3]}, one2, ls1, false);
      }
#pragma unroll
      for (int u = 0; u < D / 32; ++u) {
        half8 vf;
        vf.lo = read_b64(vbuf, ((4 * s + h) * (D + kVPad) + 32 * u + r) * 8);
        vf.hi = read_b64(vbuf, ((4 * s + 2 + h) * (D + kVPad) + 32 * u + r) * 8);
        acc_o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, acc_o[u], 0, 0, 0);
      }
    }
    l_run += ls0 + ls1;
  };

  // ---- prologue: tiles 0, 1 in the ring, tile 2 in registers, tile 0 scored
  floatx16 stA[2], stB[2];
  if (ntiles > 0) {
    store_tile(0);
    if (ntiles > 1) store_from(kreg1, vreg1, 1);
    if (ntiles > 2) load_tile(kt0 + 2 * kBN);
    __syncthreads();
    if (tcls(kt0) != 0) qk(0, stA);
  }
  // iteration it: ring slot it%3 holds tile it (V read now), slot (it+1)%3 tile it+1 (K read
  // now), slot (it+2)%3 receives tile it+2 while tile it+3 is loaded into registers
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
      prepare(kt0 + it * kBN, ccur, cur, nxt, cnxt != 0);
      exp_pv(cur, slot);
    }
    slot = s1;
  };
  for (int it = 0; it < ntiles; it += 2) {
    step(it, stA, stB);
    if (it + 1 < ntiles) step(it + 1, stB, stA);
  }

  // ---- epilogue: the unnormalised partial of (slice bi, chunk ch); stores coalesce along nq
  if (!wave_active || qi >= nq) return;
  const float l_tot = l_run + xor32(l_run);
  float* rec = sa.ws + (bi * sa.nchunks + ch) * (int64_t)(vd + 3) * nq;
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (FAST || v < vd) rec[(int64_t)v * nq + qi] = acc_o[u][i];
    }
  if (h == 0) {
    float* st = rec + (int64_t)vd * nq;
    st[qi] = m_set ? m_run : kNegInf;  // sentinel: the row attends nothing in this chunk
    st[nq + qi] = m_set ? l_tot : 0.f;
    st[2 * nq + qi] = m_max;
  }
}

// One thread per (slice, output channel, query), queries fastest.  The chunk loops run in fixed
// order on plain loads, so every thread of a query derives the same ref and L, and the result
// does not depend on the batch or on timing.  The threads of channel 0 also write l and m.
__global__ __launch_bounds__(256) void splitk_merge_kernel(SplitArgs sa) {
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n, vd = a.v_d, nc = sa.nchunks;
  const int64_t per = (int64_t)vd * nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bi = gid / per;
  const int rem = (int)(gid - bi * per);
  const int v = rem / nq, q = rem - v * nq;
  constexpr float kNegInf = -__builtin_huge_valf();
  const int64_t rstride = (int64_t)(vd + 3) * nq;
  const float* rec = sa.ws + bi * nc * rstride;
  const float* stat = rec + (int64_t)vd * nq + q;

  float ref = kNegInf, mmax = kNegInf;
  for (int s = 0; s < nc; ++s) {
    ref = fmaxf(ref, stat[s * rstride]);
    mmax = fmaxf(mmax, stat[s * rstride + 2 * nq]);
  }
  __half* O = static_cast<__half*>(a.O) + bi * per;
  float* lo = static_cast<float*>(a.l) + bi * (int64_t)nq;
  __half* mo = static_cast<__half*>(a.m) + bi * (int64_t)nq;
  if (ref == kNegInf) {  // no allowed key anywhere
    O[(int64_t)v * nq + q] = __float2half(0.f);
    if (v == 0) {
      lo[q] = 0.f;
      mo[q] = neg_inf_approx<__half>();
    }
    return;
  }
  float L = 0.f, o = 0.f;
  for (int s = 0; s < nc; ++s) {
    const float wgt = __builtin_amdgcn_exp2f(stat[s * rstride] - ref);  // 0 for an empty chunk
    L += stat[s * rstride + nq] * wgt;
    o += rec[s * rstride + (int64_t)v * nq + q] * wgt;
  }
  O[(int64_t)v * nq + q] = __float2half(o / L);
  if (v == 0) {
    const __half mT = __float2half(mmax * kLn2);
    // l relative to the STORED (rounded) m, as every other fp16 kernel writes it
    lo[q] = L * __builtin_amdgcn_exp2f(ref - __half2float(mT) * kLog2e);
    mo[q] = mT;
  }
}

template <int D>
hipError_t launch_partial_t(const SplitArgs& sa, hipStream_t s) {
  using S = Smem<D>;
  const FwdArgs& a = sa.f;
  const bool fast = a.d == D && a.v_d == D && (a.rule.k.n % 8 == 0) &&
                    (reinterpret_cast<uintptr_t>(a.K) % 16 == 0) && (reinterpret_cast<uintptr_t>(a.V) % 16 == 0);
  const int pol = a.rule.policy == 0 ? 0 : (rule_is_interval(a.rule) ? 1 : 2);
  auto kern = pol == 0 ? (fast ? splitk_partial_kernel<D, 0, true> : splitk_partial_kernel<D, 0, false>)
            : pol == 1 ? (fast ? splitk_partial_kernel<D, 1, true> : splitk_partial_kernel<D, 1, false>)
                       : (fast ? splitk_partial_kernel<D, 2, true> : splitk_partial_kernel<D, 2, false>);
  hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), S::kTotal);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.b * sa.nchunks)), dim3(kThr), S::kTotal, s, sa);
  return hipGetLastError();
}

}  // namespace

// Slices per launch pair: both grids stay below 2^31 blocks.
int64_t fwd_f16_splitk_max_batch(const SplitArgs& sa) {
  const int64_t merge_blocks = ((int64_t)sa.f.v_d * sa.f.rule.q.n + 255) / 256;
  const int64_t per = sa.nchunks > merge_blocks ? sa.nchunks : merge_blocks;
  return ((1ll << 31) - 1) / per;
}

hipError_t launch_fwd_f16_splitk(const SplitArgs& sa, hipStream_t s) {
  const FwdArgs& a = sa.f;
  const int dm = max(a.d, a.v_d);
  hipError_t e = dm <= 32 ? launch_partial_t<32>(sa, s) : dm <= 64 ? launch_partial_t<64>(sa, s)
                                                                     : launch_partial_t<128>(sa, s);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * a.rule.q.n;
  hipLaunchKernelGGL(splitk_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, sa);
  return hipGetLastError();
}

}  // namespace fa
