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
//
// mla_partial_kernel itself is in fa_fwd_f16_mla.h, which the query-blocked forms share
// (fa_fwd_f16_mla_prefill.hip); the decode instances' machine code is what it was when the kernel was written out
// here (profiles/mla_prefill_asm_equal.txt).
#include "fa_fwd_f16_mla.h"

namespace fa {
namespace {

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
