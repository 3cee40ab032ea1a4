// fa_fwd_f16_prefill.h — the query-blocked form of the ragged and paged few-query forwards: what its kernel
// template over the four caches (fa_fwd_f16_prefill.hip; the caches: fa_fwd_f16_decode.h) is made of.
//
// The twins stop at one workgroup's 128 rows.  Here the nq queries are cut into nqb = ceil(nq / P) blocks of
// P = GqaArgs::pitch queries, P the largest power of two with g * P <= 128, and the g heads of a group are folded
// into the g * P rows of one workgroup as before.  Block qb holds the queries [q0, q0 + nq_b), q0 = qb * P,
// nq_b = min(P, nq - q0), and is the twin's problem on a strided view of Q:
//   * under the tail rule its newest query sits at position len - nq + q0 + nq_b - 1, so the block sees the keys
//     [0, L_b), L_b = clamp(len - nq + q0 + nq_b, 0, len), and query q0 + i sees j <= L_b - nq_b + i: RaggedRows'
//     own interval with (len, nq) = (L_b, nq_b).  Under the full rule L_b = len.
//   * the map is the twin's with those two numbers, plus q0 and kQBlock: the core (fa_fwd_f16_core.h) then starts
//     Q q0 elements in, keeps the whole nq as Q's row stride, and counts live rows and each wave's last lane by nq_b.
//   * one workgroup per (K/V slice, query block, key chunk), chunks fastest.  It loads and clamps its slice's
//     length, forms L_b, and returns before any other load where its chunk starts at or past L_b (so the blocks
//     of queries before position 0 leave at once); otherwise it runs the core over [chunk start,
//     min(chunk end, L_b)): tiles past the block's newest key are not staged, and a paged map's look-ahead is
//     capped at the last page with a key below L_b.  Its record is filed under slice * nqb + qb.
//   * the merge, one thread per (slice, channel, head, query) with the queries fastest, folds the
//     ceil(L_b / chunk) live chunks of the query's block in order; none: the empty row.
// The instance (POL 1 for the tail form, POL 0 for the full form) is picked per call, never per block, so a last
// block of one query does not change the bits of the others.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_PREFILL_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_PREFILL_H_

#include "fa_fwd_f16_fewq.h"

namespace fa {
namespace f16core {

// a map over one query block; Base: RaggedRows, PagedRows or their 8-bit forms, with len = L_b and nq = nq_b
template <class Base>
struct BlockRowsOf : Base {
  static constexpr bool kQBlock = true;
  int32_t q0;  // the block's first query
  __device__ __forceinline__ bool row_live(int rho, int) const {
    return rho < this->g * this->pitch && (rho & (this->pitch - 1)) < this->nq;
  }
};
using BlockRows = BlockRowsOf<RaggedRows>;
using BlockPagedRows = BlockRowsOf<PagedRows>;
using BlockRows8 = BlockRowsOf<RaggedRows8>;
using BlockPagedRows8 = BlockRowsOf<PagedRows8>;

// the queries of the block at q0 and the end L_b of the keys they see, of a slice of `len` live keys
__device__ __forceinline__ int block_queries(const GqaArgs& ga, int q0) { return min(ga.pitch, ga.s.f.rule.q.n - q0); }
__device__ __forceinline__ int block_len(const GqaArgs& ga, bool tail, int len, int q0) {
  return tail ? min(max(len - ga.s.f.rule.q.n + q0 + block_queries(ga, q0), 0), len) : len;
}

// What workgroup blockIdx.x of a query-blocked partial kernel works: K/V slice *bkv, query block *qb at *q0,
// chunk *ch, the block's key end *lb, and the tiles [*kt0, *kt0 + 64 * *ntiles).  False: nothing (no record is read).
__device__ __forceinline__ bool prefill_block(const RaggedArgs& ra, int nqb, bool tail, uint32_t* bkv, int* qb, int* q0,
                                              int* ch, int* lb, int* kt0, int* ntiles) {
  const SplitArgs& sa = ra.g.s;
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x), t = bid / (uint32_t)sa.nchunks;
  *ch = (int)(bid - t * (uint32_t)sa.nchunks);
  *bkv = t / (uint32_t)nqb;
  *qb = (int)(t - *bkv * (uint32_t)nqb);
  *q0 = *qb << ra.g.log2_pitch;
  *kt0 = *ch * sa.chunk;
  *lb = block_len(ra.g, tail, __builtin_amdgcn_readfirstlane(slice_len(ra, *bkv)), *q0);
  if (*kt0 >= *lb) return false;
  *ntiles = chunk_tiles(sa, *kt0, *lb);
  return true;
}

// the merge thread of a query-blocked forward: query q of head j is row j * P + q % P of block q / P
__device__ __forceinline__ void prefill_merge(const RaggedArgs& ra, int nqb) {
  const GqaArgs& ga = ra.g;
  const SplitArgs& sa = ga.s;
  int64_t bkv;
  int v, j, q;
  if (!merge_thread(sa.f, ga.g, &bkv, &v, &j, &q)) return;
  const int qb = q >> ga.log2_pitch, q0 = qb << ga.log2_pitch;
  const int lb = block_len(ga, ra.tail_causal != 0, slice_len(ra, (uint32_t)bkv), q0);
  merge_row(sa, ga.g * ga.pitch, bkv * nqb + qb, j * ga.pitch + (q - q0), v, min(sa.nchunks, (lb + sa.chunk - 1) / sa.chunk),
            bkv * ga.g + j, q);
}

// host: one workgroup per (slice, query block, chunk) of `sa` on partial kernel `kern` at channel tile D
template <int D, class Args>
hipError_t launch_prefill_partial(IC<D>, void (*kern)(Args), const Args& args, const SplitArgs& sa, int nqb, hipStream_t s) {
  const int smem = Smem<D, kFewqNW>::kTotal;
  hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(sa.f.b * nqb * sa.nchunks)), dim3(kFewqNW * 64), smem, s, args);
  return hipGetLastError();
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_PREFILL_H_
