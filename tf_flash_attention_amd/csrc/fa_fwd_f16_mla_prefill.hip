// fa_fwd_f16_mla_prefill.hip — MLA attention for ANY number of queries over the paged latent cache, with an optional
// tree mask over the draft slots: the query-blocked forms of fa_fwd_f16_mla.hip (gfx950 MFMA).
//
// Decode folds heads x query slots into at most 512 rows of one key walk.  Here the nq queries (the sequence's last
// nq positions) are cut into blocks: a 64-row workgroup holds P consecutive queries of 64 / P heads, P the power of
// two that lets a block hold as many heads as it can (P = max(1, 64 / next_pow2(heads))), because the heads of a
// query share its key end and its mask row and the queries of a head do not.  heads = 128: two head blocks a query;
// heads = 16: 16 heads x 4 queries; heads = 1: 64 queries.  Rows past the last query or the last head are dead.
//
//   grid: (sequence, key chunk, row block), the row blocks fastest, so the workgroups that read one tile run next to
//   each other; row block rb = query block * nhb + head block.  The tile walk, the LDS image, the hand-over, the
//   table look-ahead, the FP8 staging and the record are mla_partial's (fa_fwd_f16_mla.h), unchanged.
//
//   key ends: under the tail rule without a mask query i sees keys j <= len - nq + i, so block b ends at
//   L_b = clamp(len - nq + (its last query) + 1, 0, len): a workgroup whose chunk starts at or past L_b leaves at
//   once, its tiles are counted from L_b, and the merge folds only the chunks below L_b.  Keys are still zeroed at
//   `len` where they are staged and the per-row score mask stays exact, so a block's last tiles serve its rows'
//   different ends.  The blocks are launched in query order, not heaviest first: with the row blocks fastest the
//   light and the heavy blocks of one tile alternate anyway.
//
//   the mask (a compile-time variant): every block ends at `len`; a tile that overlaps the draft slots
//   [len - nq, len), at most (nq + 63) / 64 + 1 of them, has each lane load the three words of its row that hold the
//   tile's 64 slots and apply their bits together with the length mask before the row maximum.  A masked score is
//   -inf, its P is exp2(-inf) = 0 under the exact running maximum, and a tile or a chunk that a row sees nothing of
//   adds exactly nothing: a lower-triangle mask gives the unmasked tail call's bits.
//
// mla_prefill_merge_kernel: one thread per (sequence, channel, head, query), the queries fastest, folds the chunks
// below ITS block's key end in chunk order with merge_row; no chunk (L_b = 0, or len = 0) writes the empty row.
#include "fa_fwd_f16_mla.h"

namespace fa {
namespace {

__global__ __launch_bounds__(256) void mla_prefill_merge_kernel(MlaPrefillArgs pa) {
  const MlaArgs& ma = pa.m;
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
  // the block of (head, q), its row there and its key end: the partial kernel's
  const int qb = q >> ma.log2_pitch, hpb = kRows >> ma.log2_pitch, hb = head / hpb;
  const int end = !pa.mask && ma.tail_causal ? min(max(len - nq + min((qb + 1) * ma.pitch, nq), 0), len) : len;
  const int nc = min(sa.nchunks, (end + sa.chunk - 1) / sa.chunk);
  const int row = (head - hb * hpb) * ma.pitch + (q & (ma.pitch - 1));
  f16core::merge_row(sa, kRows, seq * ma.nrb + qb * pa.nhb + hb, row, v, nc, seq * ma.heads + head, q);
}

// the partial kernel of the pool's encoding and of the mask's presence over `args`, then the merge
template <class Args>
hipError_t launch_mla_prefill(const Args& args, const MlaPrefillArgs& pa, hipStream_t s) {
  const MlaArgs& ma = pa.m;
  const FwdArgs& a = ma.s.f;
  const unsigned grid = (unsigned)(a.b * ma.nrb * ma.s.nchunks);
  const hipError_t e = pa.mask ? launch_smem(mla_partial_kernel<MaskedOf<Args>>, grid, kNW * 64, kSmem, s, MaskedOf<Args>{args})
                               : launch_smem(mla_partial_kernel<Args>, grid, kNW * 64, kSmem, s, args);
  if (e != hipSuccess) return e;
  const int64_t threads = a.b * (int64_t)a.v_d * ma.heads * a.rule.q.n;
  hipLaunchKernelGGL(mla_prefill_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, pa);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fwd_f16_mla_prefill(const MlaPrefillArgs& pa, hipStream_t s) { return launch_mla_prefill(pa, pa, s); }
hipError_t launch_fwd_f16_mla_prefill_fp8(const MlaPrefillFp8Args& pa8, hipStream_t s) {
  return launch_mla_prefill(pa8, pa8.p, s);
}

}  // namespace fa
