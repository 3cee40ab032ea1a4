// fa_kernels.h — launch-argument structs and launcher entry points shared by
// the C-ABI host layer (fa_api.hip) and the kernel translation units.
#ifndef TF_FLASH_ATTENTION_AMD_FA_KERNELS_H_
#define TF_FLASH_ATTENTION_AMD_FA_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_rules.h"

namespace fa {

struct FwdArgs {
  const void* Q;
  const void* K;
  const void* V;
  void* O;
  void* l;
  void* m;
  int64_t b;
  int32_t d, v_d;
  double scale;  // 1/sqrt(d)
  Rule rule;
};

struct BwdArgs {
  const void* Q;
  const void* K;
  const void* V;
  const void* O;
  const void* l;
  const void* m;
  const void* dO;
  void* dQ;
  void* dK;
  void* dV;
  // never read: holds the 8 bytes of the former dQ accumulator pointer, so that every later member keeps its
  // kernarg offset and the backward kernels their instruction streams (profiles/fallback_retire_asm_equal.txt)
  void* reserved;
  void* ws_D;    // b*nq AccT
  void* ws_lse;  // b*nq AccT
  int64_t b;
  int32_t d, v_d;
  double scale;
  Rule rule;
};

// floats of one (slice, chunk) record of the few-query forwards' workspace: v_d channel rows and three
// statistics rows of `stride` floats (the format: fa_fwd_f16_fewq.h)
constexpr int64_t fewq_record_floats(int32_t v_d, int64_t stride) { return (int64_t)(v_d + 3) * stride; }

// split-key fp16 forward (fa_fwd_f16_splitk.hip): the plan of fa_api.hip plus the workspace
struct SplitArgs {
  FwdArgs f;
  float* ws;        // [b][nchunks] records of stride nq
  int32_t nchunks;  // chunks of the key range, >= 2
  int32_t chunk;    // keys per chunk (a multiple of the 64-key tile)
  int32_t k_first;  // first key of chunk 0 (tile-aligned, <= the range's first key)
  int32_t k_end;    // one past the range's last key
};

// grouped-query fp16 forward (fa_fwd_f16_gqa.hip): `g` query slices share one K/V slice and are folded into
// the 128 rows of one workgroup.  s.f.b counts K/V slices; Q, O, l and m hold s.f.b * g slices.
struct GqaArgs {
  SplitArgs s;         // s.ws: [b_kv][nchunks] records of stride g * pitch; nchunks >= 1
  int32_t g;           // query slices per K/V slice, >= 2
  int32_t pitch;       // rows per head: the smallest power of two >= nq; g * pitch <= 128
  int32_t log2_pitch;
};

// ragged few-query fp16 forward (fa_fwd_f16_decode.h): the grouped forward's layout and plan over the
// capacity nk = g.s.f.rule.k.n, with the live keys of each K/V slice read on the device
struct RaggedArgs {
  GqaArgs g;              // g.g >= 1; g.s.k_first = 0 and g.s.k_end = nk (the full rule over the capacity)
  const int32_t* k_lens;  // device: K/V slice bkv of the whole call uses k_lens[bkv / kv_per_len], clamped to [0, nk]
  int64_t len0;           // this launch's first K/V slice is slice len0 * kv_per_len + rem0 of the whole call, so
  int32_t rem0;           //   its slice bkv uses k_lens[len0 + (rem0 + bkv) / kv_per_len]: a 32-bit division
  int32_t kv_per_len;     // K/V slices that share one length, >= 1
  int32_t tail_causal;    // != 0: query i sees keys j <= len - nq + i
};

// paged few-query fp16 forward (fa_fwd_f16_decode.h): the ragged forward over a capacity of max_pages * page
// keys, with K and V held in pools of pages, [num_pages][Hk][channels][page] halfs, and a block table on the
// device.  r.g.s.f.K / V are the POOLS' base pointers (never advanced per launch) and r.kv_per_len is Hk:
// K/V slice bkv of the whole call is head bkv % Hk of sequence bkv / Hk.
struct PagedArgs {
  RaggedArgs r;
  const int32_t* block_table;  // device: [sequences][max_pages]; entry [s][p] holds keys [p*page, (p+1)*page) of s
  int32_t max_pages;           // >= 1; max_pages * page = nk
  int32_t page;                // keys per page, a multiple of 64
  int32_t last_page;           // num_pages - 1: every loaded entry is clamped to [0, last_page]
};

// the ragged and the paged forward over an FP8 K/V cache (fa_fwd_f16_decode.h): K / V (or the pools) are OCP
// e4m3fn bytes in the same layouts, and the scales are device arrays of kv_per_len floats, one per K/V head of a
// sequence, that only the kernels read (null: 1.0)
struct RaggedFp8Args {
  RaggedArgs r;
  const float* k_scale;  // true key = k_scale[head] * K8
  const float* v_scale;  // true value = v_scale[head] * V8
};
struct PagedFp8Args {
  PagedArgs p;
  const float* k_scale;
  const float* v_scale;
};

// the sliding-window forms of the four forwards above (fa_fwd_f16_window.h): `a` with the window's plan in place
// of the capacity's.  a's SplitArgs holds nchunks = the launched chunks per K/V slice (relative to the chunk that
// holds the window's first key, a device value) and the records [b_kv][nchunks]; its tail_causal is not read:
// the tail rule's positions are implied.
template <class Args>
struct WindowOf {
  Args a;
  int32_t window;  // W: query i sees the keys [max(0, pos_i - W + 1), pos_i], pos_i = len - nq + i; 1 <= W < nk
};

// the query-blocked forms of the same four forwards (fa_fwd_f16_prefill.h): `a` for any number of queries.  a's
// GqaArgs holds the BLOCK's pitch P (the largest power of two with g * P <= 128, not bounded below by nq), and its
// SplitArgs the records [b_kv][nqb][nchunks] of stride g * P.
template <class Args>
struct PrefillOf {
  Args a;
  int32_t nqb;  // query blocks: ceil(nq / P), >= 2
};

// the sliding-window forms over query blocks of the same four forwards (fa_fwd_f16_window_prefill.h): `a` as
// PrefillOf takes it, with the window's plan as WindowOf takes it: a's SplitArgs holds nchunks = the launched chunks
// per (K/V slice, query block), relative to the chunk that holds the first key of the block's window, and the
// records [b_kv][nqb][nchunks] of stride g * P; its tail_causal is not read.
template <class Args>
struct WindowPrefillOf {
  Args a;
  int32_t window;  // W, as in WindowOf; 1 <= W < nk
  int32_t nqb;     // query blocks, as in PrefillOf; >= 2
};

// the tree-masked draft forms of the same four forwards (fa_fwd_f16_tree.h): `a` with the capacity's plan, as the
// plain form takes it; a's tail_causal is not read: the draft slots' positions are the tail's.
template <class Args>
struct TreeOf {
  Args a;
  const uint32_t* mask;  // device: [sequences][nq][ceil(nq / 32)] words from this LAUNCH's first sequence on (a.len0)
};

// the write side of the four caches (fa_cache_append.hip): new tokens' K and V stored in place.  Sequence s holds
// L = clamp(k_lens[s], 0, nk) keys AFTER the append, of which the last n = min(clamp(new_lens[s], 0, n_new), L)
// (new_lens null: min(n_new, L)) are new: slot n_new - n + t of K_new / V_new goes to key position L - n + t.
struct AppendArgs {
  const void* K_new;           // [sequences][kv_heads][d][n_new] fp16
  const void* V_new;           // [sequences][kv_heads][v_d][n_new] fp16
  void* K;                     // ragged: [sequences][kv_heads][d][nk]; paged: the pool [num_pages][kv_heads][d][page]
  void* V;                     //   the same over v_d rows; fp16 or e4m3fn bytes
  const float* k_scale;        // FP8 caches: device, kv_heads values, byte = e4m3fn(fp32(x) / scale[h]); null: 1.0
  const float* v_scale;
  const int32_t* block_table;  // paged caches: device [sequences][max_pages], loaded entries clamped to [0, last_page]
  const int32_t* k_lens;       // device [sequences]
  const int32_t* new_lens;     // device [sequences], or null
  int32_t max_pages, page, last_page;
  int32_t kv_heads, d, v_d, n_new, nk;
  int32_t chunks;              // 8-key destination chunks a run of n_new positions can touch: (n_new + 14) / 8
  int32_t slice_blocks;        // 256-thread blocks per (sequence, head): ceil((d + v_d) * chunks / 256)
};

// split-key dQ pass of the fp16 backward (fa_bwd_f16_dq.hip): the plan of fa_api.hip plus the partials
struct BwdSplitArgs {
  BwdArgs b;
  float* ws_part;   // [b][nchunks][d][nq] floats: unscaled fp32 dQ partials
  int32_t nchunks;  // chunks of the key range, >= 2
  int32_t chunk;    // keys per chunk (a multiple of the 64-key tile)
  int32_t k_first;  // first key of chunk 0 (tile-aligned, <= the range's first key)
  int32_t k_end;    // one past the range's last key
};

// split-query dK/dV pass of the fp16 backward (fa_bwd_f16_fast.hip): the plan of fa_api.hip plus the partials
struct BwdQSplitArgs {
  BwdArgs b;
  float* ws_part;   // [b][nchunks][d + v_d][nk] floats: unscaled fp32 dK (d rows), then dV (v_d rows) partials
  int32_t nchunks;  // chunks of the query range, >= 2
  int32_t chunk;    // queries per chunk (a multiple of four 32-query tiles)
  int32_t q_first;  // first query of chunk 0 (tile-aligned, <= the range's first query)
  int32_t q_end;    // one past the range's last query
};

// merge of partial results over several key sets and the part-order sum (fa_merge.hip): the parts'
// pointers travel by value in the kernel arguments (no device pointer table)
constexpr int kMaxParts = 8;  // FA_MAX_PARTS

struct MergeArgs {
  const void* O_parts[kMaxParts];  // [b][v_d][nq] T
  const void* l_parts[kMaxParts];  // [b][nq] L_T, relative to the stored m
  const void* m_parts[kMaxParts];  // [b][nq] T
  void* O;
  void* l;
  void* m;
  int64_t b, nq;
  int32_t v_d;
};

struct AccumulateArgs {
  const void* parts[kMaxParts];  // count elements of T each
  void* out;
  int64_t count;
};

// Slices per launch (the grid's y extent; 0: one slice alone exceeds the 32-bit index of its threads).
int64_t merge_max_batch(int dtype, int64_t nq, int32_t v_d);
hipError_t launch_merge(int dtype, int n_parts, const MergeArgs& a, hipStream_t s);
// Elements per launch, a multiple of every vector width.
int64_t accumulate_max_count();
hipError_t launch_accumulate(int dtype, int n_parts, const AccumulateArgs& a, hipStream_t s);

// generic (any dtype, any channel count) SIMT path, channel-chunked — fa_generic.hip.  The caller refuses
// what the predicates do not take (a channel count past 65536, a grid of 2^31 blocks or more).
bool fwd_generic_supported(int dtype, const FwdArgs& a);
hipError_t launch_fwd_generic(int dtype, const FwdArgs& a, hipStream_t s);
bool bwd_generic_supported(int dtype, const BwdArgs& a);
hipError_t launch_bwd_generic(int dtype, const BwdArgs& a, hipStream_t s);

// The MFMA paths: where a *_supported predicate fails, the caller falls back to the generic path.
// The fp16 MFMA forward's kernels, the choice among them and their launchers: fa_fwd_f16_choice.h.
// The few-query fp16 forwards: a partial kernel per (slice, key chunk), which runs the general kernel's key
// loop (fa_fwd_f16_core.h) over its chunk, and a merge kernel (the pair: fa_fwd_f16_fewq.h).  At most
// fwd_f16_fewq_max_batch() slices per call (grid limits), rows_out the (head, query) rows a slice's merge writes.
int64_t fwd_f16_fewq_max_batch(int32_t nchunks, int32_t v_d, int64_t rows_out);
// split-key: one query block against a long key range — fa_fwd_f16_splitk.hip
hipError_t launch_fwd_f16_splitk(const SplitArgs& sa, hipStream_t s);
// grouped-query: the same over the group's folded query rows, one workgroup per (K/V slice, key chunk), and the
// merge writes each query slice's O, l, m — fa_fwd_f16_gqa.hip
hipError_t launch_fwd_f16_gqa(const GqaArgs& ga, hipStream_t s);
// The decode forwards: a K/V cache times a form (fa_fwd_f16_decode.h).  Args, the cache: RaggedArgs (the grouped
// forward with a per-slice key length), PagedArgs (the same over a page pool and a device block table),
// RaggedFp8Args or PagedFp8Args (the two over an FP8 cache with per-head scales); each launcher is instantiated
// for these four.  The form: plain (a chunk at or past its slice's length returns at once, and the merge folds only
// the chunks below it) — fa_fwd_f16_decode.hip; with a sliding window (work for the window's chunks only) —
// fa_fwd_f16_window.hip; for any number of queries (one workgroup per (K/V slice, query block, key chunk)) —
// fa_fwd_f16_prefill.hip; with a device bit mask over the last nq keys (the plain form's chunks and merge) —
// fa_fwd_f16_tree.hip; with a sliding window over query blocks (the product of the second and the third) —
// fa_fwd_f16_window_prefill.hip.
template <class Args>
hipError_t launch_fwd_f16_decode(const Args& args, hipStream_t s);
template <class Args>
hipError_t launch_fwd_f16_window_prefill(const WindowPrefillOf<Args>& wp, hipStream_t s);
template <class Args>
hipError_t launch_fwd_f16_window(const WindowOf<Args>& wa, hipStream_t s);
template <class Args>
hipError_t launch_fwd_f16_prefill(const PrefillOf<Args>& pf, hipStream_t s);
template <class Args>
hipError_t launch_fwd_f16_tree(const TreeOf<Args>& ta, hipStream_t s);
// The fused K/V append of the same four caches (paged: behind a block table; fp8: e4m3fn bytes with per-head scales):
// one launch of `blocks` = sequences * kv_heads * a.slice_blocks workgroups, which the caller has checked to fit a
// grid — fa_cache_append.hip
hipError_t launch_cache_append(bool paged, bool fp8, const AppendArgs& a, int64_t blocks, hipStream_t s);
// fp32 MFMA forward — fa_fwd_f32.hip
bool fwd_f32_supported(const FwdArgs& a);
hipError_t launch_fwd_f32(const FwdArgs& a, hipStream_t s);
hipError_t launch_fwd_f32_wide(const FwdArgs& a, hipStream_t s);  // fa_fwd_f32_wide.hip (D = 256)
// fp32 MFMA backward (two-pass) — fa_bwd_f32.hip
bool bwd_f32_supported(const BwdArgs& a);
hipError_t launch_bwd_f32(const BwdArgs& a, hipStream_t s);
hipError_t launch_bwd_f32_wide(const BwdArgs& a, hipStream_t s);  // fa_bwd_f32_wide.hip (D = 256, after the prep)
// fp64 MFMA forward and two-pass backward (d, v_d <= 128) — fa_f64.hip
bool fwd_f64_supported(const FwdArgs& a);
hipError_t launch_fwd_f64(const FwdArgs& a, hipStream_t s);
bool bwd_f64_supported(const BwdArgs& a);
hipError_t launch_bwd_f64(const BwdArgs& a, hipStream_t s);
// dK / dV pass at D = 128 with 64 keys a wave (one wave per SIMD, dK / dV in AGPRs) —
// diag/fa_bwd_f16_k64.hip (diagnostic library only: FA_BWD_VARIANT 1700)
bool bwd_dkdv_k64_supported(const BwdArgs& a);
hipError_t launch_dkdv_k64(const BwdArgs& a, hipStream_t s);
// the fp16 MFMA backward, max(d, v_d) <= 256: two passes (dK/dV key-outer + dQ query-outer, no atomics) —
// fa_bwd_f16_fast.hip (prep, dK/dV, dispatch), fa_bwd_f16_dq.hip (dQ), fa_bwd_f16_wide.hip (D = 256); shared
// pieces in fa_bwd_f16_parts.h
bool bwd_f16_fast_supported(const BwdArgs& a);
hipError_t launch_bwd_f16_fast(const BwdArgs& a, hipStream_t s);
// the same backward for one query block (nq <= 128, max(d, v_d) <= 128) against a long key range: the
// prep and the dK/dV pass as above, then the one-wave dQ pass on one workgroup per (slice, key chunk)
// writing fp32 partials, and a reduce kernel that sums them in chunk order — fa_bwd_f16_dq.hip.
// At most bwd_f16_split_max_batch() slices per call (grid limits).
int64_t bwd_f16_split_max_batch(const BwdSplitArgs& sa);
hipError_t launch_bwd_f16_split(const BwdSplitArgs& sa, hipStream_t s);
// the mirrored shape, many queries against one key block (nk <= 128, max(d, v_d) <= 128): the prep, then the
// dK/dV pass on one workgroup per (slice, query chunk) writing fp32 partials and a reduce kernel that sums
// them in chunk order, then the dQ pass as above — fa_bwd_f16_fast.hip.  At most
// bwd_f16_qsplit_max_batch() slices per call (grid limits).
int64_t bwd_f16_qsplit_max_batch(const BwdQSplitArgs& sa);
hipError_t launch_bwd_f16_qsplit(const BwdQSplitArgs& sa, hipStream_t s);

}  // namespace fa

#endif  // TF_FLASH_ATTENTION_AMD_FA_KERNELS_H_
