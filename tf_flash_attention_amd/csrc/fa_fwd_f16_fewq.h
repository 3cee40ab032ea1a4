// fa_fwd_f16_fewq.h — the partial + merge pair of the few-query fp16 forwards (gfx950 MFMA).
//
// Few queries against many keys leave the GPU empty when one workgroup walks a slice's whole key range, so the
// split-key, grouped and decode forwards (fa_fwd_f16_splitk.hip, _gqa.hip, _decode.hip, _window.hip, _prefill.hip,
// _tree.hip) cut
// the key range into the chunks of a plan (fa_api.hip) and run two kernels:
//   * a partial kernel, one workgroup of 4 waves per (slice, chunk), runs fwd_f16_core (fa_fwd_f16_core.h) over
//     its chunk only and writes the UNNORMALISED fp32 accumulator of its live rows with their statistics to the
//     workspace: one record (below) per (slice, chunk);
//   * a merge kernel, one thread per (slice, output channel, head, query) with the queries fastest, folds the
//     chunks of its row and writes the usual O, l, m.  The threads of channel 0 also write l and m.
// The chunk loops of the merge run in fixed order on plain loads and there are no atomics, so every thread of a
// row derives the same reference and sum, and the result does not depend on the batch or on timing.
// A variant supplies its row map (fa_fwd_f16_core.h: which row is which query, whether it is live, the record
// stride, where a key tile lies), its chunk's key range and its argument struct; everything else is here:
// fewq_block, chunk_tiles, fewq_partial, merge_thread, merge_row, merge_folded on the device, and the launch helpers.
#ifndef TF_FLASH_ATTENTION_AMD_FA_FWD_F16_FEWQ_H_
#define TF_FLASH_ATTENTION_AMD_FA_FWD_F16_FEWQ_H_

#include "fa_fwd_f16_core.h"

namespace fa {
namespace f16core {

constexpr int kFewqNW = 4;      // waves per workgroup: one query block of 128 rows
constexpr int kFewqF = kFDot2;  // the core's structure flags: fwd_f16_kernel's default form

// The workspace record of one (slice, chunk): fewq_record_floats (fa_kernels.h) = (vd + kStats) rows of `stride`
// floats, `stride` the row map's rec_stride.  Channel row v holds O[v] of every row of the block relative to
// m_run, then come the statistics rows: m_run (log2 units; kEmpty where the row attends nothing in the chunk), the
// row sum l relative to m_run (0 there) and the exact row max m_max.  Only live rows are written or read.
struct FewqRecord {
  enum Stat { kMRun = 0, kL = 1, kMMax = 2, kStats = 3 };
  static constexpr float kEmpty = -__builtin_huge_valf();
  int vd, stride;
  __device__ __forceinline__ int64_t floats() const { return fewq_record_floats(vd, stride); }
  __device__ __forceinline__ int64_t chan(int v, int row) const { return (int64_t)v * stride + row; }
  __device__ __forceinline__ int64_t stat(int k, int row) const { return (int64_t)vd * stride + (k * stride + row); }
};
static_assert(fewq_record_floats(1, 1) == 1 + FewqRecord::kStats, "the host sizes the workspace by the same record");

// FoldedRows with a per-slice key length (fa_fwd_f16_core.h: the row maps): the ragged and the paged forward
struct RaggedRows : FoldedRows {
  static constexpr bool kRagged = true;
  int32_t len, nq;
  __device__ __forceinline__ int key_limit(int) const { return len; }
  // the tail-causal interval (POL 1): empty (khi < 0) for a query before the sequence's first position
  __device__ __forceinline__ void lane_interval(const Rule&, int qi, int* klo, int* khi) const {
    *klo = 0;
    *khi = len - nq + qi;
  }
};

// the length of K/V slice bkv of this launch, clamped to [0, nk]; the same value in every lane
__device__ __forceinline__ int slice_len(const RaggedArgs& ra, uint32_t bkv) {
  const int len = ra.k_lens[ra.len0 + ((uint32_t)ra.rem0 + bkv) / (uint32_t)ra.kv_per_len];
  return min(max(len, 0), ra.g.s.f.rule.k.n);
}

// partial kernel: this workgroup's slice and chunk, and the chunk's first key where chunk 0 starts at the
// tile-aligned `first`
__device__ __forceinline__ void fewq_block(const SplitArgs& sa, int first, uint32_t* slice, int* ch, int* kt0) {
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  *slice = bid / (uint32_t)sa.nchunks;
  *ch = (int)(bid % (uint32_t)sa.nchunks);
  *kt0 = first + *ch * sa.chunk;
}

// the tiles of the chunk at kt0 of a key range that ends at `end`; `or_none`: the chunk may lie at or past `end`
// (0 tiles), otherwise kt0 < end
__device__ __forceinline__ int chunk_tiles(const SplitArgs& sa, int kt0, int end, bool or_none = false) {
  const int ce = min(kt0 + sa.chunk, end);
  return !or_none || ce > kt0 ? (ce - kt0 + kBN - 1) / kBN : 0;
}

// The partial of (slice, chunk ch): the core over the key tiles [kt0, kt0 + 64 * ntiles), then the record of the
// live rows; the stores coalesce along the rows.  POL / FAST: see fwd_f16_core.  With few live rows the waves
// without one only keep loads in flight.  `rg` and `ws` are the kernel's, for fwd_f16_core's reason.  Register
// allocation of the D = 128 instances is sensitive to the form of what surrounds the core: the map by value, the
// single live-row test and chunk_tiles' optional guard keep every kernel's AGPR count and occupancy where they
// were before the kernels shared this body (profiles/fewq_skeleton_asm.txt).
template <int D, int POL, bool FAST, class Map>
__device__ __forceinline__ void fewq_partial(const SplitArgs& sa, lds_char_t* smem, Map map, int64_t slice, int ch,
                                             int kt0, int ntiles, WaveRegs<D, kFewqNW, typename KvOf<Map>::Reg>& rg,
                                             WaveState<D>& ws, int64_t rec_slice = -1) {
  // rec_slice: the slice that the record is filed under, where that is not the K/V slice (a query-blocked
  // forward files block qb of slice s under s * nqb + qb: fa_fwd_f16_prefill.h)
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n;
  fwd_f16_core<D, kFewqNW, POL, FAST, kFewqF, Map>(a, smem, slice, 0, kt0, ntiles, rg, ws, map, slice);

  const int row = ws.qi;
  if (!(ws.wave_active & map.row_live(row, nq))) return;  // (&: one test, not a branch per condition)
  const float l_tot = ws.l_run + xor32(ws.l_run);
  const FewqRecord r = {FAST ? D : a.v_d, map.rec_stride(nq)};
  float* rec = sa.ws + ((rec_slice < 0 ? slice : rec_slice) * sa.nchunks + ch) * r.floats();
#pragma unroll
  for (int u = 0; u < D / 32; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * ws.h;
      float o = ws.acc_o[u][i];
      if constexpr (KvOf<Map>::k8) o *= map.vmul;  // an 8-bit cache's v_scale: the merge stays the fp16 forwards'
      if (FAST || v < r.vd) rec[r.chan(v, row)] = o;
    }
  if (ws.h == 0) {
    rec[r.stat(FewqRecord::kMRun, row)] = ws.m_set ? ws.m_run : FewqRecord::kEmpty;
    rec[r.stat(FewqRecord::kL, row)] = ws.m_set ? l_tot : 0.f;
    rec[r.stat(FewqRecord::kMMax, row)] = ws.m_max;
  }
}

// merge kernel: this thread's K/V slice, output channel v and query q of head j of the slice's g; false past the end
__device__ __forceinline__ bool merge_thread(const FwdArgs& a, int g, int64_t* slice, int* v, int* j, int* q) {
  const int nq = a.rule.q.n;
  const int64_t per = (int64_t)a.v_d * g * nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.b * per) return false;
  *slice = gid / per;
  const int rem = (int)(gid - *slice * per);
  *v = rem / (g * nq);
  const int t = rem - *v * (g * nq);
  *j = t / nq;
  *q = t - *j * nq;
  return true;
}

// Folds row `row`, channel v of the first `nc` records of K/V slice `slice` (records of `stride` floats a row) and
// writes O[v][q], and for channel 0 l[q] and m[q], of query slice bi: the maximum of the references first, then
// each chunk weighted by exp2 of its distance to it, l and O summed in chunk order, one division.
__device__ __forceinline__ void merge_row(const SplitArgs& sa, int stride, int64_t slice, int row, int v, int nc,
                                          int64_t bi, int q) {
  const FwdArgs& a = sa.f;
  const int nq = a.rule.q.n;
  const FewqRecord r = {a.v_d, stride};
  const int64_t rstride = r.floats();
  const float* rec = sa.ws + slice * sa.nchunks * rstride;
  const float* stat = rec + r.stat(FewqRecord::kMRun, row);
  float ref = FewqRecord::kEmpty, mmax = FewqRecord::kEmpty;
  for (int s = 0; s < nc; ++s) {
    ref = fmaxf(ref, stat[s * rstride]);
    mmax = fmaxf(mmax, stat[s * rstride + FewqRecord::kMMax * stride]);
  }
  __half* O = static_cast<__half*>(a.O) + bi * (int64_t)r.vd * nq;
  float* lo = static_cast<float*>(a.l) + bi * (int64_t)nq;
  __half* mo = static_cast<__half*>(a.m) + bi * (int64_t)nq;
  if (ref == FewqRecord::kEmpty) {  // no allowed key anywhere (ragged: an empty slice, or a query before position 0)
    O[(int64_t)v * nq + q] = __float2half(0.f);
    if (v == 0) store_lm(lo, mo, q, 0.f, ref, mmax);
    return;
  }
  float L = 0.f, o = 0.f;
  for (int s = 0; s < nc; ++s) {
    const float wgt = __builtin_amdgcn_exp2f(stat[s * rstride] - ref);  // 0 for a chunk the row sees nothing of
    L += stat[s * rstride + FewqRecord::kL * stride] * wgt;
    o += rec[s * rstride + r.chan(v, row)] * wgt;
  }
  O[(int64_t)v * nq + q] = __float2half(o / L);
  if (v == 0) store_lm(lo, mo, q, L, ref, mmax);  // L > 0: the chunk that set ref has l >= 1
}

__device__ __forceinline__ FoldedRows folded_rows(const GqaArgs& ga) { return {ga.g, ga.pitch, ga.log2_pitch}; }

// the merge thread of a forward with folded rows: row j * pitch + q of K/V slice bkv, over that slice's first
// chunks(bkv) chunks, is query q of query slice bkv * g + j
template <class Chunks>
__device__ __forceinline__ void merge_folded(const GqaArgs& ga, Chunks&& chunks) {
  int64_t bkv;
  int v, j, q;
  if (!merge_thread(ga.s.f, ga.g, &bkv, &v, &j, &q)) return;
  merge_row(ga.s, folded_rows(ga).rec_stride(ga.s.f.rule.q.n), bkv, j * ga.pitch + q, v, chunks(bkv), bkv * ga.g + j, q);
}

// RaggedRows plus the block table (fa_fwd_f16_core.h: the row maps; the layout: fa_fwd_f16_decode.h).  K and V
// handed to tile() are the pools.
// The core asks for its tiles in ascending order, one per key-loop step, and the entry is a dependent load in
// front of the tile's K / V loads; asked for on the spot it stalls the wave for a memory round trip per tile
// (2 to 12 % over the ragged forward).  So tile() loads the entry of the NEXT tile's page, a whole
// tile ahead of its use, and takes its own from `pre_e`, where the call before left it; the kernel loads the first
// tile's.  This rests on the core's order of asking: kt0, kt0 + 64, kt0 + 128, ... without a gap (a different
// order would read a neighbouring page of the same sequence: wrong bits, which every bitwise test shows, never an
// access outside the pools).  The page looked ahead to is capped at last_live, the last page with a live key, so
// no entry of a page without one is ever loaded.
struct PagedRows : RaggedRows {
  static constexpr bool kPaged = true;
  const int32_t* row;   // this sequence's table row
  int32_t last_live;    // (len - 1) / page, len >= 1: the last page that holds a live key (< max_pages)
  int32_t page, last_page;
  int32_t heads, hk;    // Hk; this slice's head
  int32_t kd, vd;       // channels of a K / V page
  int32_t pre_e;        // the raw entry of the page of the tile that is asked for next
  // the pools are not sliced per K/V slice: the table says where a slice's keys are
  __device__ __forceinline__ int64_t kv_slice(int64_t, int64_t) const { return 0; }
  // (T: the pools' element, __half or the byte of an 8-bit cache; the offsets are in elements)
  template <class T>
  __device__ __forceinline__ void tile(const T* K, const T* V, int k0, const T** Kt, const T** Vt, int* ts) {
    const int p = min((int)((uint32_t)k0 / (uint32_t)page), last_live);
    const int entry = __builtin_amdgcn_readfirstlane(min(max(pre_e, 0), last_page));
    pre_e = row[min((int)((uint32_t)(k0 + kBN) / (uint32_t)page), last_live)];
    const int64_t blk = ((int64_t)entry * heads + hk) * page;  // in rows of `page` keys per channel
    const int off = k0 - p * page;
    *Kt = K + blk * kd + off;
    *Vt = V + blk * vd + off;
    *ts = page;
  }
};

// the map of K/V slice bkv of this launch, of `len` >= 1 live keys, for the chunk at kt0 < len at channel tile D
template <int D, bool FAST>
__device__ __forceinline__ PagedRows paged_rows(const PagedArgs& pa, uint32_t bkv, int len, int kt0) {
  const RaggedArgs& ra = pa.r;
  const FwdArgs& a = ra.g.s.f;
  // ---- the slice's sequence and head, as slice_len forms its k_lens index (kv_per_len = Hk)
  const uint32_t idx = (uint32_t)ra.rem0 + bkv, seq = idx / (uint32_t)ra.kv_per_len;
  const int hk = (int)(idx - seq * (uint32_t)ra.kv_per_len);
  const int32_t* row = pa.block_table + (ra.len0 + (int64_t)seq) * pa.max_pages;
  return {{folded_rows(ra.g), len, a.rule.q.n}, row, (int)((uint32_t)(len - 1) / (uint32_t)pa.page),
          pa.page, pa.last_page, ra.kv_per_len, hk, FAST ? D : a.d, FAST ? D : a.v_d,
          row[(uint32_t)kt0 / (uint32_t)pa.page]};  // (kt0 < len: a page with a live key)
}

// ---- an 8-bit K/V cache (fa_fwd_f16_core.h: KvOf; fa_fwd_f16_decode.h: RaggedCache8, PagedCache8)

// The scales of head hk as the core takes them.  k_scale = 2^e * r with e = round(log2 k_scale) clamped to
// [-8, 7]: kmul = 2^e multiplies K exactly in the conversion to fp16, and qmul = r, in [2^-0.5, 2^0.5) inside the
// clamp, multiplies the Q pre-scale in fp32 before Q is rounded to fp16; all of k_scale there would push Q' towards
// fp16 subnormals for small scales.  vmul = v_scale.  A null array means 1.0: kmul = qmul = vmul = 1, the fp16
// forward's bits.  A k_scale or v_scale that is not finite and positive makes vmul NaN, so O is NaN rather than
// plausible.  The NaN must not go through the scores: under -fno-honor-nans a row whose scores are all NaN keeps no
// reference, its record says "no key" and the merge writes O = 0 (tests/test_gpu_fp8_cache.py, the invalid-scale
// test); so a bad k_scale leaves qmul at 1 and the finite scores carry the NaN accumulator to the merge.  All of
// this is integer work on the scale's bits (-fno-honor-nans cannot touch it) and wave-uniform.
struct Kv8Mul {
  float kmul, qmul, vmul;
};
__device__ __forceinline__ Kv8Mul kv8_mul(const float* k_scale, const float* v_scale, int hk) {
  constexpr uint32_t kOne = 0x3f800000u, kNaN = 0x7fc00000u, kMaxFinite = 0x7f7fffffu;
  const uint32_t kb = k_scale ? __float_as_uint(k_scale[hk]) : kOne;
  const uint32_t vb = v_scale ? __float_as_uint(v_scale[hk]) : kOne;
  // the exponent field, one more where the mantissa is at or above sqrt(2) (0x3fb504f3): round(log2)
  int e = (int)(kb >> 23) - 127 + ((kb & 0x7fffffu) >= 0x3504f3u ? 1 : 0);
  e = min(max(e, -8), 7);
  const float r = __uint_as_float(kb) * __uint_as_float((uint32_t)(127 - e) << 23);  // exact: a power of two
  Kv8Mul s;
  s.kmul = __uint_as_float((uint32_t)(127 + e) << 23);
  const bool k_ok = kb - 1u < kMaxFinite, v_ok = vb - 1u < kMaxFinite;
  s.qmul = __uint_as_float(k_ok ? __float_as_uint(r) : kOne);
  s.vmul = __uint_as_float(k_ok & v_ok ? vb : kNaN);
  return s;
}

// RaggedRows / PagedRows over an 8-bit cache
struct RaggedRows8 : RaggedRows {
  static constexpr bool kKv8 = true;
  float kmul, qmul, vmul;
};
struct PagedRows8 : PagedRows {
  static constexpr bool kKv8 = true;
  float kmul, qmul, vmul;
};

// host: the channel tile of these arguments; `f(d)` receives it as IC<D>
template <class F>
hipError_t with_fewq_d(const FwdArgs& a, F&& f) {
  const int dm = max(a.d, a.v_d);
  return dm <= 32 ? f(IC<32>{}) : dm <= 64 ? f(IC<64>{}) : f(IC<128>{});
}

// host: the <D, POL, FAST> instantiation of a forward under the rule (with_pol_fast); `launch(d, pol, fast)`
template <class Launch>
hipError_t with_fewq_rule(const FwdArgs& a, Launch&& launch) {
  return with_fewq_d(a, [&](auto d) {
    return with_pol_fast<decltype(d)::value>(a, [&](auto pol, auto fast) { return launch(d, pol, fast); });
  });
}

// host: the same of a forward with key lengths.  `row_keys`: the keys between two channel rows of K / V (the
// capacity, or the page), `chunk_bytes` those of 8 keys.  One query under the tail rule sees [0, len): the full
// form, so that its bits are the full form's.
template <class Launch>
hipError_t with_fewq_tail(const RaggedArgs& ra, int row_keys, Launch&& launch, int chunk_bytes = 16) {
  const FwdArgs& a = ra.g.s.f;
  return with_fewq_d(a, [&](auto d) {
    const bool fast = fast_staging<decltype(d)::value>(a, row_keys, chunk_bytes);
    const bool tail = ra.tail_causal != 0 && a.rule.q.n > 1;
    return tail ? (fast ? launch(d, IC<1>{}, IC<1>{}) : launch(d, IC<1>{}, IC<0>{}))
                : (fast ? launch(d, IC<0>{}, IC<1>{}) : launch(d, IC<0>{}, IC<0>{}));
  });
}

// host: one workgroup per (slice, chunk) of `sa` on partial kernel `kern` at channel tile D
template <int D, class Args>
hipError_t launch_fewq_partial(IC<D>, void (*kern)(Args), const Args& args, const SplitArgs& sa, hipStream_t s) {
  const int smem = Smem<D, kFewqNW>::kTotal;
  hipError_t e = set_smem_once(reinterpret_cast<const void*>(kern), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(sa.f.b * sa.nchunks)), dim3(kFewqNW * 64), smem, s, args);
  return hipGetLastError();
}

// host: one thread per (slice, channel, head of g, query) on merge kernel `kern`
template <class Args>
hipError_t launch_fewq_merge(void (*kern)(Args), const Args& args, const FwdArgs& a, int g, hipStream_t s) {
  const int64_t threads = a.b * (int64_t)a.v_d * g * a.rule.q.n;
  hipLaunchKernelGGL(kern, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, args);
  return hipGetLastError();
}

}  // namespace f16core
}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_FWD_F16_FEWQ_H_
