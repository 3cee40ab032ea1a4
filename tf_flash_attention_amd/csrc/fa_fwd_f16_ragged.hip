// fa_fwd_f16_ragged.hip — few-query fp16 forward over a padded K/V cache with per-sequence key lengths
// (gfx950 MFMA).
//
// A decode batch is ragged: K and V are laid out for a common capacity nk, and K/V slice bkv holds only
// len = k_lens[bkv / kv_per_len] live keys, a DEVICE value that changes from step to step (the call is
// replayed from a captured graph, so the host never sees it).  The structure is fa_fwd_f16_gqa.hip's —
// FoldedRows blocks of g heads x pitch rows, one workgroup per (K/V slice, key chunk) of grouped_plan's
// chunks over the capacity, fp32 partials in the same record format, a merge in chunk order without
// atomics — with the length threaded through:
//   * ragged_partial_kernel loads and clamps its slice's length as a wave-uniform value.  A chunk that
//     starts at or past it returns before the core and writes nothing; the others run fwd_f16_core over
//     [chunk start, min(chunk end, len)) with RaggedRows, whose key_limit is len while the capacity stays
//     the row stride.  Tiles wholly below len keep the unguarded 16-byte staging; in the tile that holds
//     len the core zeroes staged K and V past it element by element.
//   * ragged_merge_kernel folds only the chunks below len, so no unwritten workspace word reaches an output;
//     len = 0 writes the empty rows (O = 0, l = 0, m = bytes 0xFA).
// Two forms.  Full (POL 0): every query sees keys [0, len).  Tail-causal (POL 1): the nq queries are the last
// nq positions of the sequence, query i sees keys [0, len - nq + i]; queries i < nq - len see nothing.
// With every length equal to the capacity and g >= 2 the full form runs gqa_partial_kernel's loop over the
// same chunks, and the result is bitwise fa_forward_grouped's.
#include "fa_fwd_f16_ragged.h"

namespace fa {
namespace {

using namespace f16core;

constexpr int kNW = 4;       // waves per workgroup: 128 folded rows
constexpr int kF = kFDot2;   // the core's structure flags: fwd_f16_kernel's default form

template <int D, int POL, bool FAST>
__global__ __launch_bounds__(kNW * 64, waves_per_eu(D, kF)) void ragged_partial_kernel(RaggedArgs ra) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const GqaArgs& ga = ra.g;
  const SplitArgs& sa = ga.s;
  const FwdArgs& a = sa.f;
  constexpr float kNegInf = -__builtin_huge_valf();

  const int nq = a.rule.q.n, vd = FAST ? D : a.v_d;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t bkv32 = bid / (uint32_t)sa.nchunks;
  const int64_t bkv = bkv32;
  const int ch = (int)(bid % (uint32_t)sa.nchunks);

  // ---- this chunk's share [kt0, ce) of the slice's live keys [0, len) (kt0 is tile-aligned)
  const int len = __builtin_amdgcn_readfirstlane(slice_len(ra, bkv32));
  const int kt0 = ch * sa.chunk;
  if (kt0 >= len) return;  // a dead chunk: the merge does not read its record
  const int ce = min(kt0 + sa.chunk, len);
  const int ntiles = (ce - kt0 + kBN - 1) / kBN;

  const RaggedRows map = {ga.g, ga.pitch, ga.log2_pitch, len, nq};
  WaveRegs<D, kNW> rg;
  WaveState<D> ws;
  fwd_f16_core<D, kNW, POL, FAST, kF, RaggedRows>(a, (lds_char_t*)smem_raw, 0, 0, kt0, ntiles, rg, ws, map, bkv);

  // ---- epilogue: the unnormalised partial of the live rows; stores coalesce along the rows
  const int rho = ws.qi, gp = ga.g * ga.pitch;
  if (!ws.wave_active || rho >= gp || (rho & (ga.pitch - 1)) >= nq) return;
  const float l_tot = ws.l_run + xor32(ws.l_run);
  float* rec = sa.ws + (bkv * sa.nchunks + ch) * (int64_t)(vd + 3) * gp;
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * ws.h;
      if (FAST || v < vd) rec[(int64_t)v * gp + rho] = ws.acc_o[u][i];
    }
  if (ws.h == 0) {
    float* st = rec + (int64_t)vd * gp;
    st[rho] = ws.m_set ? ws.m_run : kNegInf;  // sentinel: the row sees no key of this chunk (tail-causal)
    st[gp + rho] = ws.m_set ? l_tot : 0.f;
    st[2 * gp + rho] = ws.m_max;
  }
}

// gqa_merge_kernel over the live chunks [0, ceil(len / chunk)) of the thread's K/V slice: every live chunk
// wrote the records of all live rows, and the dead ones are not read.
__global__ __launch_bounds__(256) void ragged_merge_kernel(RaggedArgs ra) {
  const GqaArgs& ga = ra.g;
  const SplitArgs& sa = ga.s;
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n, vd = a.v_d, g = ga.g, gp = ga.g * ga.pitch;
  const int64_t per = (int64_t)vd * g * nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return;
  const int64_t bkv = gid / per;
  const int rem = (int)(gid - bkv * per);
  const int v = rem / (g * nq), t = rem - v * (g * nq);
  const int j = t / nq, q = t - j * nq;
  const int rho = j * ga.pitch + q;
  constexpr float kNegInf = -__builtin_huge_valf();
  const int64_t rstride = (int64_t)(vd + 3) * gp;
  const float* rec = sa.ws + bkv * sa.nchunks * rstride;
  const float* stat = rec + (int64_t)vd * gp + rho;
  const int len = slice_len(ra, (uint32_t)bkv);
  const int nc = min(sa.nchunks, (len + sa.chunk - 1) / sa.chunk);

  float ref = kNegInf, mmax = kNegInf;
  for (int s = 0; s < nc; ++s) {
    ref = fmaxf(ref, stat[s * rstride]);
    mmax = fmaxf(mmax, stat[s * rstride + 2 * gp]);
  }
  const int64_t bi = bkv * g + j;  // the query slice
  __half* O = static_cast<__half*>(a.O) + bi * (int64_t)vd * nq;
  float* lo = static_cast<float*>(a.l) + bi * (int64_t)nq;
  __half* mo = static_cast<__half*>(a.m) + bi * (int64_t)nq;
  if (ref == kNegInf) {  // no key: an empty slice, or a query before the sequence's first position
    O[(int64_t)v * nq + q] = __float2half(0.f);
    if (v == 0) store_lm(lo, mo, q, 0.f, ref, mmax);
    return;
  }
  float L = 0.f, o = 0.f;
  for (int s = 0; s < nc; ++s) {
    const float wgt = __builtin_amdgcn_exp2f(stat[s * rstride] - ref);  // 0 for a chunk the row does not see
    L += stat[s * rstride + gp] * wgt;
    o += rec[s * rstride + (int64_t)v * gp + rho] * wgt;
  }
  O[(int64_t)v * nq + q] = __float2half(o / L);
  if (v == 0) store_lm(lo, mo, q, L, ref, mmax);  // L > 0: the chunk that set ref has l >= 1
}

template <int D, int POL, bool FAST>
hipError_t launch_partial_pf(const RaggedArgs& ra, hipStream_t s) {
  auto kern = ragged_partial_kernel<D, POL, FAST>;
  const int smem = Smem<D, kNW>::kTotal;
  hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(ra.g.s.f.b * ra.g.s.nchunks)), dim3(kNW * 64), smem, s, ra);
  return hipGetLastError();
}

// FAST as with_pol_fast takes it, over the capacity: K / V rows of every slice start 16-byte aligned.  One
// query under the tail rule sees [0, len): the full form, so that its bits are the full form's.
template <int D>
hipError_t launch_partial_t(const RaggedArgs& ra, hipStream_t s) {
  const FwdArgs& a = ra.g.s.f;
  const bool fast = a.d == D && a.v_d == D && (a.rule.k.n % 8 == 0) &&
                    (reinterpret_cast<uintptr_t>(a.K) % 16 == 0) && (reinterpret_cast<uintptr_t>(a.V) % 16 == 0);
  const bool tail = ra.tail_causal != 0 && a.rule.q.n > 1;
  return tail ? (fast ? launch_partial_pf<D, 1, true>(ra, s) : launch_partial_pf<D, 1, false>(ra, s))
              : (fast ? launch_partial_pf<D, 0, true>(ra, s) : launch_partial_pf<D, 0, false>(ra, s));
}

}  // namespace

// (also the merge of the paged forward, fa_fwd_f16_paged.hip: the same records, lengths and outputs)
hipError_t launch_fwd_f16_ragged_merge(const RaggedArgs& ra, hipStream_t s) {
  const FwdArgs& a = ra.g.s.f;
  const int64_t threads = a.b * (int64_t)a.v_d * ra.g.g * a.rule.q.n;
  hipLaunchKernelGGL(ragged_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ra);
  return hipGetLastError();
}

hipError_t launch_fwd_f16_ragged(const RaggedArgs& ra, hipStream_t s) {
  const FwdArgs& a = ra.g.s.f;
  const int dm = max(a.d, a.v_d);
  hipError_t e = dm <= 32 ? launch_partial_t<32>(ra, s) : dm <= 64 ? launch_partial_t<64>(ra, s)
                                                                     : launch_partial_t<128>(ra, s);
  if (e != hipSuccess) return e;
  return launch_fwd_f16_ragged_merge(ra, s);
}

}  // namespace fa
