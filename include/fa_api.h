/*
 * fa_api.h — C ABI of the MI355X (gfx950) fused flash-attention op.
 *
 * This is the drop-in boundary.  It replaces the reference's internal C++
 * launcher boundary
 *     cuda_launch::FlashAttentionLauncher<T, RefShape, OrderMap, Policy>::Forward / ::Backward
 *     (/root/reference/flash_attention/kernel/flash_attention.h:220-260,
 *      instantiated at flash_attention.cu:2450-2487)
 * which the TF op kernels call from
 *     FlashAttentionForwardBase::Compute   (flash_attention_forward.cc:280-386)
 *     FlashAttentionBackwardBase::Compute  (flash_attention_backward.cc:181-344)
 * and the FLOP estimator ops
 *     FlashAttentionForwardFlopsEstimationBase::Compute (flash_attention_forward.cc:420-473).
 *
 * Instead of templates over (dtype, seq dims, policy) the ABI takes them as
 * plain enums, and instead of CuTe order-map types it takes the raw sequence
 * shapes plus the sync-mode name: the sync map (sync_methods.cc:8-117) is
 * computed inside the library.  Plain pointers and sizes only; no torch/TF
 * types; no C++ exceptions cross it.
 *
 * Memory layout (channel-first, row-major, exactly the reference's):
 *   Q  [b][d  ][nq]   K [b][d][nk]   V [b][v_d][nk]
 *   O  [b][v_d][nq]   l [b][nq]      m [b][nq]
 * where b = prod(batch shape), nq = prod(Q sequence shape), nk likewise.
 * T is fp16 / fp32 / fp64; l has type L_T = fp32 for fp16 inputs, T otherwise
 * (flash_attention.h:181-185).  All buffers are device memory owned by the
 * caller.  Every output element is written by the library (no caller memset).
 *
 * Pointers of the dense entry points (fa_forward, fa_forward_ws, fa_backward, fa_backward_split): every
 * tensor need only be aligned to its own element type (2 bytes for fp16 Q / K / V / O / m / dO / dQ / dK /
 * dV, 4 for an fp32 l, and so on), each on its own: the library picks its 16-byte paths per call from the
 * pointers and lengths it is given and takes element-wise ones otherwise, so alignment changes the kernel,
 * never the contract.  Nothing outside [ptr, ptr + bytes) of any tensor influences a result or is written,
 * whatever those bytes hold (NaN included), and no input is written.  A workspace is the library's own
 * layout (regions at multiples of 256 bytes from its base, read and written 16 bytes at a time) and must
 * be 256-byte aligned; the library never reads a workspace byte it has not written in the same call, and
 * writes none past the size its *_workspace_bytes function reports.  tests/test_gpu_guarded.py holds the
 * library to this paragraph.
 *
 * Threading: every entry point is reentrant; all work is enqueued on `stream`
 * (a hipStream_t, NULL = default stream) with no host synchronisation, so the
 * calls are safe inside hipGraph capture.
 */
#ifndef TF_FLASH_ATTENTION_AMD_FA_API_H_
#define TF_FLASH_ATTENTION_AMD_FA_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dtype of Q/K/V/O/m (and l unless fp16) */
enum fa_dtype { FA_F16 = 0, FA_F32 = 1, FA_F64 = 2 };

/* attention policy = masking rule (flash_attention.h:45-149) */
enum fa_policy { FA_FULL = 0, FA_CAUSAL = 1, FA_LOCAL = 2 };

/* sync mode (sync_methods.cc:113-117) */
enum fa_sync_mode { FA_NONE_FRONT = 0, FA_SCALE_FRONT = 1, FA_SCALE_END = 2 };

/* status codes: 0 = success, >0 = hipError_t passed through, <0 = library errors */
enum fa_status {
  FA_OK = 0,
  FA_ERR_INVALID_ARGUMENT = -1,
  FA_ERR_UNSUPPORTED = -2,
  FA_ERR_WORKSPACE_TOO_SMALL = -3,
};

/* Problem description shared by all entry points.
 * q_seq / k_seq hold `seq_dims` extents in the tensors' axis order
 * (e.g. {H, W} for 2d).  window_size >= 1 and 0 <= log2_stride_size < 31 are
 * only read for FA_LOCAL (attrs of the Local ops, flash_attention_forward.cc:173-175). */
typedef struct fa_problem {
  int32_t dtype;            /* enum fa_dtype */
  int32_t policy;           /* enum fa_policy */
  int32_t seq_dims;         /* 1 or 2 */
  int32_t sync_mode;        /* enum fa_sync_mode */
  int64_t b;                /* flattened batch (batch dims incl. heads) */
  int32_t q_seq[2];
  int32_t k_seq[2];
  int32_t d;                /* Q/K channels */
  int32_t v_d;              /* V/O channels */
  int32_t window_size;
  int32_t log2_stride_size;
  int32_t is_causal;
} fa_problem;

/* "none_front" | "scale_front" | "scale_end" -> enum value, or -1
 * (SyncMethods::Lookup, sync_methods.h:91-101). */
int fa_sync_mode_from_string(const char* name);

/* Validates a problem (ranks, extents, local attrs).  Returns FA_OK or
 * FA_ERR_INVALID_ARGUMENT; the message is available via fa_last_error(). */
int fa_validate(const fa_problem* p);

/* Forward: writes O, l, m.  Replaces FlashAttentionLauncher::Forward
 * (flash_attention.h:225-234) + the 4 memsets of flash_attention_forward.cc:352-369. */
int fa_forward(void* stream, const fa_problem* p,
               const void* Q, const void* K, const void* V,
               void* O, void* l, void* m);

/* Split-key forward: fp16 problems with one query block (at most 128 queries), max(d, v_d) <= 128
 * and a rule-bounded key range of at least 2048 keys cut that range into chunks, one workgroup
 * per (slice, chunk), and merge the partial results (fa_forward itself never splits; it keeps one
 * workgroup per slice for such shapes).  The routing is a pure function of the problem WITHOUT b,
 * so a slice's result does not depend on how the batch is sharded.
 *
 * fa_forward_workspace_bytes (host-only): bytes of device scratch fa_forward_ws needs; 0 when
 *   the problem is outside the split envelope.
 * fa_forward_ws: with fa_forward_workspace_bytes(p) == 0 exactly fa_forward (the workspace is
 *   ignored); otherwise the split path, or FA_ERR_WORKSPACE_TOO_SMALL (nothing is written).
 * fa_forward_split_plan (host-only): out[0] = number of chunks (0 outside the envelope),
 *   out[1] = keys per chunk, out[2..3] = key range [kb, ke) of the query block. */
size_t fa_forward_workspace_bytes(const fa_problem* p);
int fa_forward_ws(void* stream, const fa_problem* p,
                  const void* Q, const void* K, const void* V,
                  void* O, void* l, void* m,
                  void* workspace, size_t workspace_bytes);
int fa_forward_split_plan(const fa_problem* p, int32_t out[4]);

/* Grouped-query forward (GQA; MQA when every head shares one K/V head): kv_group = g query slices share one
 * K/V slice.  p->b counts Q slices and must be a multiple of kv_group, else FA_ERR_INVALID_ARGUMENT with text
 * in fa_last_error(); K and V hold b / kv_group slices, Q / O / l / m hold b.  Q slice bi attends K/V slice
 * bi / kv_group (the repeat_interleave convention), and its (O, l, m) is what fa_forward gives for that slice
 * against that K/V slice, to rounding.  fa_problem is unchanged.
 *
 * The fused path folds the g heads of a group into the 128 query rows of one workgroup, at a row pitch P =
 * the smallest power of two >= nq: row rho of the block is query rho % P of head rho / P.  K and V stream once
 * per group instead of once per head.  One workgroup per (K/V slice, key chunk) writes fp32 partials of its
 * live rows, and a merge kernel folds a row's chunks in chunk order (no atomics: deterministic).  The
 * partial-plus-merge pair is the only grouped path, also for a short key range (one chunk).
 *
 * Envelope: fp16, max(d, v_d) <= 128, kv_group >= 2, nq >= 1, nk >= 1, kv_group * P <= 128.
 * Chunks: fa_forward_split_plan's formula — the first chunk starts at the key tile (64 keys) that holds kb,
 *   chunks hold max(min_chunk, ceil(ceil(span / 64) / 64) * 64) keys, span = ke - floor(kb / 64) * 64, at most
 *   64 chunks — with min_chunk = 512 for kv_group * P <= 64 and 1024 above.  There is no 2048-key minimum: a
 *   short range gives one or a few chunks, at least 1.
 *
 * fa_forward_grouped_plan (host-only, a pure function of the problem WITHOUT b, like fa_forward_split_plan):
 *   out[0] = key chunks, 0 outside the envelope; out[1] = keys per chunk; out[2..3] = key range [kb, ke) of
 *   the query block [0, nq-1]; out[4] = row pitch P; out[5] = folded rows kv_group * P.
 * fa_forward_grouped_workspace_bytes (host-only): b / kv_group * chunks * kv_group * P * (v_d + 3) floats,
 *   rounded up to 256 bytes; 0 outside the envelope; with kv_group == 1, fa_forward_workspace_bytes(p).
 * fa_forward_grouped: kv_group == 1 is exactly fa_forward_ws (and the plan reports 0 chunks).  Outside the
 *   envelope it returns FA_ERR_UNSUPPORTED with nothing written: the caller expands K and V and calls
 *   fa_forward_ws (the Python layer does).  A workspace smaller than fa_forward_grouped_workspace_bytes():
 *   FA_ERR_WORKSPACE_TOO_SMALL and nothing written.  No host synchronisation: safe under hipGraph capture,
 *   like the other entry points.
 * A Q slice's bits are NOT those of fa_forward_ws on expanded K/V: the online softmax moves its reference
 * lazily and takes that decision per wave, so a row's arithmetic depends on which rows share its wave.  The
 * result is deterministic, and a group's bits do not depend on b. */
int fa_forward_grouped_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]);
size_t fa_forward_grouped_workspace_bytes(const fa_problem* p, int32_t kv_group);
int fa_forward_grouped(void* stream, const fa_problem* p, int32_t kv_group,
                       const void* Q, const void* K, const void* V,
                       void* O, void* l, void* m,
                       void* workspace, size_t workspace_bytes);

/* Ragged few-query forward (decode over a padded K/V cache): fa_forward_grouped's layout — Q / O / l / m hold
 * p->b slices, K and V hold b / kv_group slices laid out for a CAPACITY nk = p->k_seq[0] — where K/V slice bkv
 * holds only L = k_lens[bkv / kv_per_len] live keys.  k_lens is a DEVICE array of (b / kv_group) / kv_per_len
 * int32 values (kv_per_len = the K/V heads of one sequence); the kernels clamp a value to [0, nk].  The host
 * never reads k_lens: no host synchronisation, and the lengths may change between replays of a captured graph.
 * Whatever K and V hold past L (NaN and Inf included) does not reach a result.
 *
 * For a slice of length L:
 *   tail_causal == 0: the (O, l, m) fa_forward gives under FA_FULL against the first L keys, to rounding;
 *   tail_causal != 0: the nq queries are the last nq positions of the sequence: query i sees keys
 *     j <= L - nq + i (for nq == 1 this is the form above, bit for bit);
 *   rows that see no key (L == 0; i < nq - L under the tail rule): O = 0, l = 0, every byte of m 0xFA.
 *
 * Envelope: fp16, seq_dims == 1, policy == FA_FULL, max(d, v_d) <= 128, kv_group >= 1 (ungrouped decode is
 *   inside, unlike fa_forward_grouped), nq >= 1, nk >= 1, kv_group * P <= 128 with P the smallest power of two
 *   >= nq.  A well-formed problem outside it: FA_ERR_UNSUPPORTED, nothing written.
 * FA_ERR_INVALID_ARGUMENT with text in fa_last_error(): policy != FA_FULL, kv_group < 1, b % kv_group != 0,
 *   kv_per_len < 1, kv_per_len not dividing b / kv_group, a null k_lens with b > 0.
 *
 * fa_forward_ragged_plan (host-only): fa_forward_grouped_plan's formula and out[6] layout over the key range
 *   [0, nk), with kv_group == 1 planned.  A pure function of the problem WITHOUT b and without the lengths
 *   (they are device data): a short sequence in a large cache launches the capacity's chunks, and those at or
 *   past its length return at once.
 * fa_forward_ragged_workspace_bytes (host-only): fa_forward_grouped_workspace_bytes's formula, b / kv_group *
 *   chunks * kv_group * P * (v_d + 3) floats rounded up to 256 bytes; 0 outside the envelope.
 * fa_forward_ragged: a smaller workspace returns FA_ERR_WORKSPACE_TOO_SMALL with nothing written; b == 0
 *   returns FA_OK with nothing launched.  A slice's bits do not depend on b or on the other slices' lengths;
 *   with every length equal to nk and kv_group >= 2 they are fa_forward_grouped's under FA_FULL. */
int fa_forward_ragged_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]);
size_t fa_forward_ragged_workspace_bytes(const fa_problem* p, int32_t kv_group);
int fa_forward_ragged(void* stream, const fa_problem* p, int32_t kv_group,
                      const void* Q, const void* K, const void* V,
                      const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                      void* O, void* l, void* m,
                      void* workspace, size_t workspace_bytes);

/* Paged few-query forward (decode over a PAGED K/V cache): fa_forward_ragged with K and V held in pools of
 * fixed-size pages and a per-sequence block table on the device.
 *   K_pool [num_pages][Hk][d][page], V_pool [num_pages][Hk][v_d][page] fp16, the key axis contiguous: a page
 *     holds `page` consecutive key positions of all Hk = kv_per_len K/V heads of one sequence.
 *   block_table: DEVICE int32 [sequences][max_pages], sequences = (b / kv_group) / kv_per_len.  Entry [s][p] is
 *     the pool page that holds keys [p * page, (p + 1) * page) of sequence s.  Several sequences may name the
 *     same page (a shared prefix): the forward only reads the pools.
 *   k_lens, kv_per_len, tail_causal, the empty rows and Q / O / l / m: as in fa_forward_ragged.  K/V slice bkv
 *     of the call is head bkv % kv_per_len of sequence bkv / kv_per_len.
 *   p->k_seq[0] = nk = max_pages * page is the CAPACITY; the kernels clamp a length to [0, nk].
 * The host reads neither k_lens nor block_table: no host synchronisation, and either may be overwritten in
 * place between replays of a captured graph.  The kernels load only the table entries of pages that hold a live
 * key: entries at or past ceil(len / page) may hold anything.  Every entry that is loaded is clamped to
 * [0, num_pages - 1] before it forms an address, as the lengths are clamped: a corrupt table gives a wrong
 * answer, never an access outside the pools.
 *
 * Envelope: fa_forward_ragged's, plus page % 64 == 0 (a 64-key tile never straddles two pages; page need not be
 *   a power of two).  A well-formed problem outside it, a smaller page included: FA_ERR_UNSUPPORTED, nothing
 *   written; there is no gather fallback.
 * FA_ERR_INVALID_ARGUMENT with text in fa_last_error(): fa_forward_ragged's own argument errors, page < 1,
 *   max_pages < 1, max_pages * page != nk (the plan functions: nk % page != 0), num_pages < 1, and with b > 0 a
 *   null block_table, pool or k_lens.
 *
 * fa_forward_paged_plan / fa_forward_paged_workspace_bytes (host-only): fa_forward_ragged_plan's and
 *   fa_forward_ragged_workspace_bytes's values over the capacity inside the envelope, out[0] == 0 / 0 bytes
 *   outside it (page % 64 != 0).  Pure functions of the problem WITHOUT b, the lengths or the table.
 * fa_forward_paged: a smaller workspace returns FA_ERR_WORKSPACE_TOO_SMALL with nothing written; b == 0 returns
 *   FA_OK with nothing launched.  Same plan, same tiles, same staged values: the (O, l, m) bits are those of
 *   fa_forward_ragged on the cache gathered into [b / kv_group][channels][nk] with the same lengths. */
int fa_forward_paged_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[6]);
size_t fa_forward_paged_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page);
int fa_forward_paged(void* stream, const fa_problem* p, int32_t kv_group,
                     const void* Q, const void* K_pool, const void* V_pool,
                     const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                     const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                     void* O, void* l, void* m,
                     void* workspace, size_t workspace_bytes);

/* The ragged and the paged forward over an FP8 K/V cache: fa_forward_ragged / fa_forward_paged with K and V (or
 * the pools) held as OCP e4m3fn bytes (NOT fnuz), one byte per element, in the same layouts:
 *   ragged: K8 [b / kv_group][d][nk], V8 [b / kv_group][v_d][nk];
 *   paged:  K_pool8 [num_pages][Hk][d][page], V_pool8 [num_pages][Hk][v_d][page], the key axis contiguous.
 * p->dtype stays FA_F16: it is the dtype of Q, O and m; l stays fp32.  Half the cache bytes per decode step and
 * twice the context per byte of cache; the matrix work is fp16 (e4m3fn -> fp16 is exact).
 *   k_scale, v_scale: DEVICE fp32 arrays of kv_per_len values, one per K/V head of a sequence, shared by all
 *     sequences; a null pointer means 1.0.  The true key of head h is k_scale[h] * K8 and the true value
 *     v_scale[h] * V8 (a per-tensor scale is the array with one value repeated).  Only the kernels read them: no
 *     host synchronisation, and they may be overwritten in place between replays of a captured graph, like
 *     k_lens and block_table.  A scale must be finite and positive; any other value gives NaN output, never an
 *     access outside the buffers.
 *   Arithmetic: k_scale = 2^e * r with e = round(log2 k_scale) clamped to [-8, 7].  K8 * 2^e is formed exactly in
 *     the conversion to fp16, r multiplies the fp32 factor 1/sqrt(d) * log2(e) before Q is rounded to fp16, and
 *     v_scale multiplies the fp32 accumulator of each key chunk before the chunks are merged.
 * Everything else is the fp16 twin's: envelope, argument errors, the empty rows, b == 0, FA_ERR_UNSUPPORTED /
 * FA_ERR_WORKSPACE_TOO_SMALL with nothing written, the launches.  The plan and the workspace ARE the twin's: use
 * fa_forward_ragged_plan / fa_forward_ragged_workspace_bytes and fa_forward_paged_plan /
 * fa_forward_paged_workspace_bytes (the chunks do not depend on the element size).
 * Guarantees:
 *   what lies past a length does not reach a result, whatever byte it is, the NaN codes 0x7F / 0xFF included
 *     (staged bytes past the length are cleared as integers before they are converted);
 *   table entries of pages without a live key are never loaded, and a loaded entry is clamped as in
 *     fa_forward_paged;
 *   a slice's bits do not depend on b or on the other slices' lengths;
 *   with both scales null or 1.0 the (O, l, m) bits are the fp16 twin's on the cache converted to fp16. */
int fa_forward_ragged_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                          const void* Q, const void* K8, const void* V8,
                          const float* k_scale, const float* v_scale,
                          const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                          void* O, void* l, void* m,
                          void* workspace, size_t workspace_bytes);
int fa_forward_paged_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                         const void* Q, const void* K_pool8, const void* V_pool8,
                         const float* k_scale, const float* v_scale,
                         const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                         const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                         void* O, void* l, void* m,
                         void* workspace, size_t workspace_bytes);

/* Sliding-window decode: the four forwards above with a window of W = `window` >= 1 keys.  The tail rule's
 * positions are implied (there is no tail_causal argument): with L the clamped length of a slice, query i sits at
 * position pos_i = L - nq + i and sees the keys j with max(0, pos_i - W + 1) <= j <= pos_i: W keys, its own
 * position included (local_1d's |qo - ko| <= W - 1 with is_causal).  A query with pos_i < 0 gets the empty row
 * (O = 0, l = 0, every byte of m 0xFA).  The block as a whole sees [lo, L), lo = max(0, L - nq - W + 1): at most
 * span_w = min(nk, W + nq - 1) keys.
 *
 * Everything else is the un-windowed twin's contract: envelope, argument errors, b == 0, FA_ERR_UNSUPPORTED and
 * FA_ERR_WORKSPACE_TOO_SMALL with nothing written, no host synchronisation, no host read of k_lens, block_table
 * or the scales.  In addition window < 1 returns FA_ERR_INVALID_ARGUMENT with text in fa_last_error().
 *
 * window >= nk can never cut anything (L <= nk), and the host knows it: the call IS the un-windowed twin with
 *   tail_causal = 1, with its plan, workspace bytes and kernels, bit for bit.
 * window < nk: the plan follows the window, not the capacity.  chunk = fa_forward_grouped_plan's formula with
 *   span_w in place of the capacity span, max(min_chunk, ceil(ceil(span_w / 64) / 64) * 64); the chunk boundaries
 *   stay at absolute multiples of chunk from key 0; per K/V slice
 *     n_launch = min(ceil(nk / chunk), floor((span_w + chunk - 2) / chunk) + 1)
 *   workgroups are launched, the most chunks an interval of span_w keys can touch.  Workgroup (slice, c) works
 *   absolute chunk floor(lo / chunk) + c with the lo of the length it loads, over the tiles from
 *   max(chunk start, floor(lo / 64) * 64) to min(chunk end, L), and returns at once where that is empty.  The
 *   workspace is b / kv_group * n_launch records of the twins' layout.
 * The plan functions (host-only; pure functions of the problem WITHOUT b, the lengths or the table) write
 *   out[0] n_launch (0 outside the envelope)     out[4] pitch P
 *   out[1] keys per chunk                        out[5] folded rows kv_group * P
 *   out[2] span_w                                out[6] 1 if delegated to the tail form (window >= nk): out[0],
 *   out[3] ceil(nk / chunk)                             out[1] are then the twin's plan, out[3] = out[0]
 *                                                out[7] reserved, 0
 * The FP8 forms use the fp16 plan and workspace functions, as their twins do.
 *
 * Never read: key tiles wholly below floor(lo / 64) * 64 and keys at or past L; in the paged forms the table
 *   entries of pages wholly below that key and of pages past the last live page: the serving stack may free
 *   and reuse those pages and leave anything in their entries.  Loaded entries and lengths are clamped as in the
 *   twins.
 * Finite keys: the keys of the first staged tile that lie below lo (at most 63, the sequence's own earlier keys
 *   on a page it still owns) are loaded and masked, not zeroed.  They must be finite: a NaN or Inf in V there
 *   would survive a probability of 0.
 * A slice's bits do not depend on b or on the other slices' lengths; the paged bits are the ragged ones on the
 *   gathered cache; the FP8 bits with null or unit scales are the fp16 ones on the converted cache. */
int fa_forward_ragged_window_plan(const fa_problem* p, int32_t kv_group, int32_t window, int32_t out[8]);
int fa_forward_paged_window_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window, int32_t out[8]);
size_t fa_forward_ragged_window_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t window);
size_t fa_forward_paged_window_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window);
int fa_forward_ragged_window(void* stream, const fa_problem* p, int32_t kv_group,
                             const void* Q, const void* K, const void* V,
                             const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                             void* O, void* l, void* m,
                             void* workspace, size_t workspace_bytes);
int fa_forward_paged_window(void* stream, const fa_problem* p, int32_t kv_group,
                            const void* Q, const void* K_pool, const void* V_pool,
                            const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                            const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                            void* O, void* l, void* m,
                            void* workspace, size_t workspace_bytes);
int fa_forward_ragged_window_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                 const void* Q, const void* K8, const void* V8,
                                 const float* k_scale, const float* v_scale,
                                 const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                 void* O, void* l, void* m,
                                 void* workspace, size_t workspace_bytes);
int fa_forward_paged_window_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                const void* Q, const void* K_pool8, const void* V_pool8,
                                const float* k_scale, const float* v_scale,
                                const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                                const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                void* O, void* l, void* m,
                                void* workspace, size_t workspace_bytes);

/* Query-blocked forwards (chunked prefill, long speculative drafts): fa_forward_ragged / fa_forward_paged and their
 * _fp8 forms for ANY nq >= 1, with the same layouts, arguments and semantics.  tail_causal == 0: every query sees
 * the keys [0, L), L the clamped length of its slice.  tail_causal != 0: the nq queries are the last nq positions,
 * query i sees j <= L - nq + i; a query before position 0 gets the empty row (O = 0, l = 0, every byte of m 0xFA).
 * A batch that mixes prefill with decode right-aligns each sequence's real queries in the nq slots; the padding
 * queries in front compute earlier positions' rows, or empty rows.
 *
 * Envelope: the twins' without the row cap: fp16, 1d sequences, FA_FULL, max(d, v_d) <= 128, 1 <= kv_group <= 128,
 * nq >= 1, nk >= 1, and page % 64 == 0 in the paged forms.  Outside it FA_ERR_UNSUPPORTED with nothing written.
 * Argument errors, b == 0 and FA_ERR_WORKSPACE_TOO_SMALL with nothing written are the twins'; so are: no host
 * synchronisation, no host read of k_lens, block_table or the scales, replayable from a captured graph.
 *
 * Block shape (a pure function of the problem WITHOUT b): P_b = the largest power of two with
 * kv_group * P_b <= 128, rows = kv_group * P_b, nqb = ceil(nq / P_b) query blocks; block qb holds the queries
 * [qb * P_b, min(nq, (qb + 1) * P_b)) of all kv_group heads.
 * nqb == 1 (kv_group * next_pow2(nq) <= 128): the call IS the un-blocked twin, with its plan, workspace bytes and
 *   kernels, bit for bit.
 * nqb >= 2: one workgroup per (K/V slice, query block, key chunk) and a merge.  With
 *     kmax = max(1, 64 / nqb), min_chunk = 512 where rows <= 64, else 1024,
 *     chunk = max(min_chunk, ceil(ceil(nk / 64) / kmax) * 64), nchunks = ceil(nk / chunk):
 *   the blocks already fill the GPU, so the more blocks the fewer chunks.  (64 / nqb is a starting rule; DESIGN.md
 *   3.14 says what was and was not measured.)  Under the tail rule block qb sees the keys [0, L_b),
 *   L_b = clamp(L - nq + min(nq, (qb + 1) * P_b), 0, L): its workgroups of chunks at or past L_b return at once, and
 *   tiles at or past L_b are never staged.  The workspace is b / kv_group * nqb * nchunks records of
 *   rows * (v_d + 3) floats, rounded up to 256 bytes.
 * The plan functions (host-only; pure functions of the problem WITHOUT b, the lengths or the table) write
 *   out[0] chunks (0 outside the envelope; then all of out[] is 0)    out[3] rows
 *   out[1] keys per chunk                                            out[4] nqb
 *   out[2] P_b                                                       out[5] 1 if delegated to the twin (nqb == 1):
 *   out[6], out[7] reserved, 0                                              out[0], out[1] are then the twin's plan
 * The FP8 forms use the fp16 plan and workspace functions, as their twins do.
 *
 * Never read: keys at or past L, whatever they hold; in the paged forms the table entries of pages without a key
 *   below L.  Loaded entries and lengths are clamped as in the twins.  No unwritten workspace word reaches a result.
 * A slice's bits do not depend on b or on the other slices' lengths; the paged bits are the ragged ones on the
 *   gathered cache; the FP8 bits with null or unit scales are the fp16 ones on the converted cache.  The kernel
 *   instance is chosen per call, so a block's bits do not depend on how many queries the last block holds. */
int fa_forward_ragged_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t out[8]);
int fa_forward_paged_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[8]);
size_t fa_forward_ragged_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group);
size_t fa_forward_paged_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page);
int fa_forward_ragged_prefill(void* stream, const fa_problem* p, int32_t kv_group,
                              const void* Q, const void* K, const void* V,
                              const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                              void* O, void* l, void* m,
                              void* workspace, size_t workspace_bytes);
int fa_forward_paged_prefill(void* stream, const fa_problem* p, int32_t kv_group,
                             const void* Q, const void* K_pool, const void* V_pool,
                             const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                             const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                             void* O, void* l, void* m,
                             void* workspace, size_t workspace_bytes);
int fa_forward_ragged_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                  const void* Q, const void* K8, const void* V8,
                                  const float* k_scale, const float* v_scale,
                                  const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                                  void* O, void* l, void* m,
                                  void* workspace, size_t workspace_bytes);
int fa_forward_paged_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                 const void* Q, const void* K_pool8, const void* V_pool8,
                                 const float* k_scale, const float* v_scale,
                                 const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                                 const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal,
                                 void* O, void* l, void* m,
                                 void* workspace, size_t workspace_bytes);

/* Tree-masked draft attention (speculative decoding that verifies a TREE of candidates in one step): the four
 * un-windowed, un-blocked forwards above with a DEVICE bit mask in the place of tail_causal.  The nq queries are
 * the draft tokens, held in the last nq positions of each sequence; each sees the committed context and, of the
 * draft tokens, those its mask row names (itself and its ancestors, for a tree).  Layouts, k_lens, kv_per_len,
 * block_table, the scales, the clamping and the empty rows are fa_forward_ragged's / fa_forward_paged's and their
 * _fp8 forms'.
 *   draft_mask: DEVICE uint32 [sequences][nq][W], W = ceil(nq / 32), sequences = (b / kv_group) / kv_per_len; shared
 *     by all K/V heads and query heads of a sequence.  Bit j & 31 of word j >> 5 of row i says whether query i sees
 *     draft slot j.  The array needs 4-byte alignment only.
 *   Rule: with L the clamped length of the slice and base = L - nq, draft slot j is key position base + j, and query
 *     i sees key k iff 0 <= k < L and (k < base or bit(i, k - base)).  There is no other case: slots whose position
 *     is negative (L < nq) name no key, and bits at or past nq in a row's last word are ignored, whatever they hold.
 *     A row that sees no key is the empty row: O = 0, l = 0, every byte of m 0xFA.  The lower-triangular mask (bit j
 *     of row i set iff j <= i) is the twin's tail_causal = 1 call.
 * The host never reads the mask: no host synchronisation, and it may be overwritten in place between replays of a
 * captured graph, like k_lens, block_table and the scales.
 *
 * Envelope: the twins': fp16, 1d sequences, FA_FULL, max(d, v_d) <= 128, kv_group * P <= 128 (so nq <= 128 and
 *   W <= 4), and page % 64 == 0 in the paged forms.  There is no windowed and no query-blocked tree form.  Outside
 *   it FA_ERR_UNSUPPORTED with nothing written.
 * FA_ERR_INVALID_ARGUMENT with text in fa_last_error(): the twins' argument errors, and with b > 0 a null
 *   draft_mask.  b == 0 and FA_ERR_WORKSPACE_TOO_SMALL with nothing written are the twins'.
 * The plan and the workspace do not depend on the mask: fa_forward_ragged_tree_plan /
 *   fa_forward_ragged_tree_workspace_bytes and the paged pair return fa_forward_ragged_plan's / ..._workspace_bytes's
 *   and fa_forward_paged_plan's / ..._workspace_bytes's values; the FP8 forms share them.
 *
 * Never read: keys at or past L, whatever they hold; in the paged forms the table entries of pages without a key
 *   below L.  Loaded entries and lengths are clamped as in the twins.
 * Finite keys: a draft key that is masked for a query is the sequence's own key below L.  It is loaded and masked,
 *   not zeroed, so it must be finite: a NaN or Inf in V there would survive a probability of 0 (the window forms'
 *   clause).
 * Bitwise: a slice's bits do not depend on b, on the other slices' lengths or on the other sequences' masks; the
 *   paged bits are the ragged ones on the gathered cache; the FP8 bits with null or unit scales are the fp16 ones on
 *   the converted cache; with the lower-triangular mask (O, l, m) are the bits of the twin called with
 *   tail_causal = 1 (masking is a select to -inf in front of the same max, exp and sum chains, and a tile the twin
 *   skips adds exact zeros when it is masked instead). */
int fa_forward_ragged_tree_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]);
int fa_forward_paged_tree_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[6]);
size_t fa_forward_ragged_tree_workspace_bytes(const fa_problem* p, int32_t kv_group);
size_t fa_forward_paged_tree_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page);
int fa_forward_ragged_tree(void* stream, const fa_problem* p, int32_t kv_group,
                           const void* Q, const void* K, const void* V,
                           const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask,
                           void* O, void* l, void* m,
                           void* workspace, size_t workspace_bytes);
int fa_forward_paged_tree(void* stream, const fa_problem* p, int32_t kv_group,
                          const void* Q, const void* K_pool, const void* V_pool,
                          const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                          const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask,
                          void* O, void* l, void* m,
                          void* workspace, size_t workspace_bytes);
int fa_forward_ragged_tree_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                               const void* Q, const void* K8, const void* V8,
                               const float* k_scale, const float* v_scale,
                               const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask,
                               void* O, void* l, void* m,
                               void* workspace, size_t workspace_bytes);
int fa_forward_paged_tree_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                              const void* Q, const void* K_pool8, const void* V_pool8,
                              const float* k_scale, const float* v_scale,
                              const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                              const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask,
                              void* O, void* l, void* m,
                              void* workspace, size_t workspace_bytes);

/* Sliding-window forwards over query blocks (chunked prefill of local-attention layers): the sliding-window
 * forwards above for ANY nq >= 1, with the same layouts, arguments and rule.  The nq queries are the last nq
 * positions of a sequence of L = clamp(k_lens, 0, nk) live keys (the tail rule is implied): query i sits at
 * pos = L - nq + i and sees the keys max(0, pos - window + 1) <= j <= pos; a query before position 0 gets the empty
 * row (O = 0, l = 0, every byte of m 0xFA).  A batch that mixes prefill with decode right-aligns each sequence's real
 * queries in the nq slots, as in the query-blocked forwards.
 *
 * Envelope: the query-blocked forwards': fp16, 1d sequences, FA_FULL, max(d, v_d) <= 128, 1 <= kv_group <= 128,
 * nq >= 1, nk >= 1, and page % 64 == 0 in the paged forms.  Outside it FA_ERR_UNSUPPORTED with nothing written.
 * window < 1 is FA_ERR_INVALID_ARGUMENT; the other argument errors, b == 0 and FA_ERR_WORKSPACE_TOO_SMALL with
 * nothing written are the twins'; so are: no host synchronisation, no host read of k_lens, block_table or the
 * scales, replayable from a captured graph.
 *
 * Block shape: the query-blocked forwards' P_b, rows and nqb.  Delegation, each bit for bit the parent with the
 * parent's plan and workspace bytes:
 *   window >= nk: the call IS fa_forward_*_prefill with tail_causal = 1 (delegated = 1);
 *   otherwise nqb == 1 (kv_group * next_pow2(nq) <= 128): the call IS fa_forward_*_window (delegated = 2).
 * Otherwise block qb holds nq_b queries and sees the keys [lo_b, L_b), L_b as in the query-blocked forwards and
 *   lo_b = max(0, L_b - nq_b - window + 1): at most span_w = min(nk, window + P_b - 1) keys.  With
 *     kmax = max(1, 64 / nqb), min_chunk = 512 where rows <= 64, else 1024,
 *     chunk = max(min_chunk, ceil(ceil(span_w / kmax) / 64) * 64), cap_chunks = ceil(nk / chunk),
 *     launched = min(cap_chunks, (span_w + chunk - 2) / chunk + 1)
 *   one workgroup per (K/V slice, query block, launched chunk) and a merge: chunk boundaries are absolute multiples
 *   of `chunk` from key 0, and launched chunk c of a block is absolute chunk lo_b / chunk + c.  The workspace is
 *   b / kv_group * nqb * launched records of rows * (v_d + 3) floats, rounded up to 256 bytes.
 * The plan functions (host-only; pure functions of the problem WITHOUT b, the lengths or the table) write
 *   out[0] launched chunks per block (0 outside the envelope; then all of out[] is 0)
 *   out[1] keys per chunk          out[4] P_b
 *   out[2] span_w                  out[5] rows
 *   out[3] cap_chunks              out[6] nqb
 *   out[7] delegated: 0, 1 or 2 as above; out[0] .. out[3] are then the parent's plan (out[2] = min(nk, window +
 *          P_b - 1) and out[3] = out[0] for 1; the windowed twin's span_w and cap_chunks for 2)
 * The FP8 forms use the fp16 plan and workspace functions, as their twins do.
 *
 * Never read: for each block, key tiles wholly below floor(lo_b / 64) * 64 and keys at or past L_b; so for the call,
 *   key tiles wholly below its lowest window start lo = max(0, L - nq - window + 1) rounded down to 64, and keys at
 *   or past L.  In the paged forms the table entries of pages wholly below that key and of pages past the last live
 *   page are never loaded: the serving stack may free and reuse those pages.  Loaded entries and lengths are clamped
 *   as in the twins.  No unwritten workspace word reaches a result.
 * Finite keys: the keys of a block's first staged tile that lie below lo_b (at most 63) are loaded and masked, not
 *   zeroed.  For every block but the first they are keys that an earlier block sees anyway; for the call, the up to
 *   63 keys below lo must be finite.
 * A slice's bits do not depend on b or on the other slices' lengths; the paged bits are the ragged ones on the
 *   gathered cache; the FP8 bits with null or unit scales are the fp16 ones on the converted cache; a full block's
 *   bits are fa_forward_*_window's on a contiguous copy of its queries with the length L_b, where both plans give the
 *   same chunk. */
int fa_forward_ragged_window_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t window, int32_t out[8]);
int fa_forward_paged_window_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window, int32_t out[8]);
size_t fa_forward_ragged_window_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t window);
size_t fa_forward_paged_window_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window);
int fa_forward_ragged_window_prefill(void* stream, const fa_problem* p, int32_t kv_group,
                                     const void* Q, const void* K, const void* V,
                                     const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                     void* O, void* l, void* m,
                                     void* workspace, size_t workspace_bytes);
int fa_forward_paged_window_prefill(void* stream, const fa_problem* p, int32_t kv_group,
                                    const void* Q, const void* K_pool, const void* V_pool,
                                    const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                                    const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                    void* O, void* l, void* m,
                                    void* workspace, size_t workspace_bytes);
int fa_forward_ragged_window_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                         const void* Q, const void* K8, const void* V8,
                                         const float* k_scale, const float* v_scale,
                                         const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                         void* O, void* l, void* m,
                                         void* workspace, size_t workspace_bytes);
int fa_forward_paged_window_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group,
                                        const void* Q, const void* K_pool8, const void* V_pool8,
                                        const float* k_scale, const float* v_scale,
                                        const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                                        const int32_t* k_lens, int32_t kv_per_len, int32_t window,
                                        void* O, void* l, void* m,
                                        void* workspace, size_t workspace_bytes);

/* Fused K/V append: the write side of the four caches above. New tokens' keys and values are stored IN PLACE into a
 * ragged cache or into page pools, fp16 or FP8, by one kernel launch enqueued on `stream`: a forward enqueued after it
 * on that stream sees the tokens.  Every control value is device data; the host reads nothing and does not
 * synchronise, so the call may be captured in a graph and replayed after any of them was overwritten in place.
 *   K_new [sequences][kv_heads][d][n_new], V_new [sequences][kv_heads][v_d][n_new]: fp16, channel-first.
 *   k_lens: DEVICE int32 [sequences], the length AFTER the append, the array the attention call of this step takes;
 *     L = clamp(k_lens[s], 0, nk).
 *   new_lens: DEVICE int32 [sequences] or null: the real new tokens of sequence s, RIGHT-ALIGNED in the n_new slots
 *     (the query-blocked forwards' mixed-batch convention: the last slot is the sequence's last position);
 *     n = min(clamp(new_lens[s], 0, n_new), L), and n = min(n_new, L) for a null array.
 *   Slot n_new - n + t is stored at key position L - n + t for t in [0, n).  The slots in front are padding: never
 *     loaded, whatever they hold.
 *   ragged: K [sequences][kv_heads][d][nk], V [sequences][kv_heads][v_d][nk]; the position is the last index.
 *   paged:  position pos goes to K_pool[entry][h][c][pos % page], entry = clamp(block_table[s][pos / page], 0,
 *     num_pages - 1), nk = max_pages * page.  pos < L <= nk keeps pos / page inside the table row, so every store lies
 *     inside the pools whatever the table holds.  Only the entries of pages that receive a new position are loaded.
 *   _fp8: the cache holds OCP e4m3fn bytes; the stored byte is the fp32 quotient fp32(x) / scale[h], correctly
 *     rounded, encoded round-to-nearest-even and saturating at +-448.  k_scale / v_scale: DEVICE fp32 [kv_heads], null
 *     means 1.0.  For NaN input, or a scale that is not finite and positive, the byte is unspecified (in bounds).
 *     An fp16 cache stores a bit copy.
 * Guarantees: every stored byte belongs to a new position; no other byte of the cache is written, not even with its
 *   old value (partial 8-key chunks are stored element by element).  A page that is not named at a written position
 *   (a shared prefix) is untouched.  Two sequences that name one page at a written position race: in bounds,
 *   otherwise unspecified.
 * The call does NOT allocate pages, change k_lens, new_lens or the table, compute scales, or copy shared pages on
 *   write.  It takes no workspace and has no plan function.
 * Envelope: page % 64 == 0 in the paged forms (no other pool can be read here); any d, v_d >= 1.  Outside it, or where
 *   sequences * kv_heads * ceil((d + v_d) * ((n_new + 14) / 8) / 256) blocks exceed 2^31 - 1: FA_ERR_UNSUPPORTED,
 *   nothing written.
 * FA_ERR_INVALID_ARGUMENT with text in fa_last_error(), before any device call: sequences < 0, n_new < 0; kv_heads, d,
 *   v_d or nk < 1; page < 1, max_pages < 1, max_pages * page != nk, num_pages < 1; and where there is work a null
 *   K_new, V_new, cache, k_lens or block_table.
 * sequences == 0 or n_new == 0: FA_OK, nothing launched.  Every n == 0: FA_OK, nothing stored. */
int fa_append_ragged(void* stream, int64_t sequences,
                     int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                     const void* K_new, const void* V_new,
                     void* K, void* V,
                     const int32_t* k_lens, const int32_t* new_lens);
int fa_append_paged(void* stream, int64_t sequences,
                    int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                    const void* K_new, const void* V_new,
                    void* K_pool, void* V_pool,
                    const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                    const int32_t* k_lens, const int32_t* new_lens);
int fa_append_ragged_fp8(void* stream, int64_t sequences,
                         int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                         const void* K_new, const void* V_new,
                         void* K8, void* V8,
                         const float* k_scale, const float* v_scale,
                         const int32_t* k_lens, const int32_t* new_lens);
int fa_append_paged_fp8(void* stream, int64_t sequences,
                        int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                        const void* K_new, const void* V_new,
                        void* K_pool8, void* V_pool8,
                        const float* k_scale, const float* v_scale,
                        const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                        const int32_t* k_lens, const int32_t* new_lens);

/* Bytes of device scratch fa_backward needs (replaces the Br_occupancy temp,
 * flash_attention_backward.cc:274-283): the D = rowsum(dO * O) rows and the lse rows,
 * [b][nq] of fp32 (fp64 problems: fp64), each rounded up to 256 bytes.  There is no dQ
 * accumulator: every backward writes dQ once, without atomics.  Pass that many bytes (or more). */
size_t fa_backward_workspace_bytes(const fa_problem* p);

/* Backward: writes dQ, dK, dV from Q, K, V, O, l, m, dO.  Replaces
 * FlashAttentionLauncher::Backward (flash_attention.h:236-246). */
int fa_backward(void* stream, const fa_problem* p,
                const void* Q, const void* K, const void* V,
                const void* O, const void* l, const void* m, const void* dO,
                void* dQ, void* dK, void* dV,
                void* workspace, size_t workspace_bytes);

/* Split-key backward: the few-query shapes of the split-key forward also cut the backward's dQ pass
 * (query-outer: one workgroup per slice for such shapes) into the same key chunks, one workgroup per
 * (slice, chunk) writing fp32 partials, and sum the partials of a query in chunk order (no atomics:
 * deterministic).  The prep and the key-outer dK/dV pass are fa_backward's, so dK and dV are bitwise
 * fa_backward's; dQ differs by fp32 summation order only.  fa_backward itself never splits.  The
 * routing is a pure function of the problem WITHOUT b, so a slice's result does not depend on how
 * the batch is sharded.
 *
 * fa_backward_split_plan (host-only): the layout of fa_forward_split_plan.  The plan is the
 *   forward's where in addition max(d, v_d) * (nk + 8) * 2 < 2^31 (a slice's K / V channel rows stay
 *   inside the dQ kernel's 32-bit buffer offsets); 0 chunks otherwise.
 * fa_backward_split_workspace_bytes (host-only): bytes of device scratch fa_backward_split needs:
 *   fa_backward_workspace_bytes(p) with 0 chunks, otherwise that plus b * chunks * d * nq floats
 *   (rounded up to 256 bytes; the partials follow fa_backward's regions).
 * fa_backward_split: with 0 chunks exactly fa_backward; otherwise the split path, or
 *   FA_ERR_WORKSPACE_TOO_SMALL (nothing is written).
 *
 * Split-query backward, the mirrored shape: fp16 problems with one key block (1 <= nk <= 128),
 * max(d, v_d) <= 128, max(d, v_d) * (nq + 8) * 2 < 2^31 (a slice's Q / dO channel rows stay inside the
 * dK/dV kernels' 32-bit buffer offsets) and a rule-bounded query range [qb, qe) of that key block of at
 * least 2048 queries cut the key-outer dK/dV pass (one workgroup per slice for such shapes) into query
 * chunks, one workgroup per (slice, chunk) writing unscaled fp32 dK / dV partials, and sum the partials of
 * a key in chunk order (no atomics: deterministic).  The prep and the dQ pass are fa_backward's, so dQ is
 * bitwise fa_backward's; dK and dV differ by fp32 summation order only.  Chunks hold
 * max(min_chunk, ceil(ceil(span / 64) / 128) * 128) queries, span = qe - floor(qb / 32) * 32, min_chunk =
 * 512 for nk <= 64 and 1024 above: at most 64 chunks.  The two plans are never both active (the key-chunk
 * plan needs nq <= 128 and a key range of at least 2048 keys).
 *
 * fa_backward_split_q_plan (host-only): out[0] = number of query chunks (0 outside the envelope),
 *   out[1] = queries per chunk, out[2..3] = query range [qb, qe) of the key block.  Validation and errors
 *   as fa_backward_split_plan.
 * fa_backward_split_workspace_bytes: with query chunks, fa_backward_workspace_bytes(p) plus
 *   b * chunks * (d + v_d) * nk floats (rounded up to 256 bytes; the partials follow fa_backward's regions).
 * fa_backward_split: with query chunks the split-query path, or FA_ERR_WORKSPACE_TOO_SMALL (nothing is
 *   written); with 0 chunks in both plans exactly fa_backward. */
int fa_backward_split_plan(const fa_problem* p, int32_t out[4]);
int fa_backward_split_q_plan(const fa_problem* p, int32_t out[4]);
size_t fa_backward_split_workspace_bytes(const fa_problem* p);
int fa_backward_split(void* stream, const fa_problem* p,
                      const void* Q, const void* K, const void* V,
                      const void* O, const void* l, const void* m, const void* dO,
                      void* dQ, void* dK, void* dV,
                      void* workspace, size_t workspace_bytes);

/* Merging partial results: attention over the union of several key sets from attention over each.
 *
 * A partial is what any forward above writes for one key set against the shared Q, in the layouts
 * at the top: O_i [b][v_d][nq] in T, l_i [b][nq] in L_T relative to the STORED m_i, m_i [b][nq] in T
 * (the row max of the scaled scores, scale = 1/sqrt(d) of the shared Q in every part).  A part is
 * empty for a row iff l_i == 0 (its m_i is then the NegInfApprox byte pattern, every byte 0xFA, and
 * stays out of the max).  Per slice and query row, over the non-empty parts:
 *     m = max_i m_i (exact in T)        e_i = l_i * exp(m_i - m)     L = sum_i e_i  (part order)
 *     w_i = e_i / L (correctly rounded) O = T(sum_i w_i * O_i)  (part order)          l = L
 * accumulated in fp32 (fp64 for FA_F64).  A row empty in every part gets O = 0, l = 0, m = NegInfApprox,
 * as the forwards write it.  (O, l, m) is then the forward's output for the concatenated keys; a key that
 * appears in two parts counts twice.  fa_backward called per part with the MERGED (O, l, m) gives that
 * part's exact dK and dV, and the parts' dQ sum to the union's dQ (fa_accumulate_parts).
 * The weights are normalised before they multiply O: one part comes back bit for bit, and a part that is
 * empty in every row leaves the result of the others bit for bit unchanged.  The result is deterministic
 * and a slice's bits do not depend on b.
 *
 * fa_merge_partials: O_parts / l_parts / m_parts are HOST arrays of n_parts device pointers, read during
 *   the call (they travel to the kernel by value: no device pointer table, no host synchronisation, safe
 *   inside hipGraph capture).  1 <= n_parts <= FA_MAX_PARTS.  Vector loads where nq is a multiple of
 *   16 bytes of T and every pointer is 16-byte aligned; any other nq or alignment takes a scalar path.
 * fa_accumulate_parts: out[i] = T(sum_p acc(parts[p][i])) for i < count, summed in part order in fp32
 *   (fp64 for FA_F64): one rounding for dQ = sum_p dQ_p.
 * Both return FA_ERR_INVALID_ARGUMENT (text in fa_last_error()) for an unknown dtype, n_parts outside
 * 1..FA_MAX_PARTS, a negative size, v_d < 1, a null pointer where there is work to do, or an output pointer
 * equal to an input pointer; all checked on the host before any device call.  b * nq == 0 (count == 0)
 * returns FA_OK with nothing launched. */
#define FA_MAX_PARTS 8
int fa_merge_partials(void* stream, int32_t dtype, int64_t b, int64_t nq, int32_t v_d, int32_t n_parts,
                      const void* const* O_parts, const void* const* l_parts, const void* const* m_parts,
                      void* O, void* l, void* m);
int fa_accumulate_parts(void* stream, int32_t dtype, int64_t count, int32_t n_parts,
                        const void* const* parts, void* out);

/* Algorithmic forward FLOPs 2*(d+v_d)*P, P = rule-allowed (q,k) pairs summed
 * over b (host-only; replaces EstimateForwardFlops, flash_attention.cu:2069-2144,
 * which counted issued tiles instead). */
double fa_estimate_forward_flops(const fa_problem* p);

/* Number of rule-allowed (q,k) pairs for one batch slice (host-only). */
int64_t fa_allowed_pairs(const fa_problem* p);

/* Host-side rule inspection (tests / tooling; no device work).
 * fa_rule_mask: writes nq*nk bytes (1 = pair attended) for one batch slice,
 *   evaluated with the same fa_rules.h code the kernels run.
 * fa_rule_probe: for Q rows [q0,q1] and K cols [k0,k1] (inclusive) writes
 *   out[0..1] = K index range [kb,ke) the kernels visit for that Q block,
 *   out[2..3] = Q index range [qb,qe) visited for that K block,
 *   out[4]    = tile class (0 none allowed, 1 mixed, 2 all allowed). */
int fa_rule_mask(const fa_problem* p, uint8_t* mask);
int fa_rule_probe(const fa_problem* p, int32_t q0, int32_t q1, int32_t k0, int32_t k1, int32_t* out);

/* Host-side dispatch inspection (tests / tooling; launches nothing and reads of the pointers only their
 * alignment): the kernel fa_forward would launch for this problem and these operands, from the same function
 * fa_forward launches through.  For fp16 the kernel instance as a kernel trace prints it, e.g.
 * "fwd_f16_fast_kernel<64, 8, 1, 14>"; for the other paths the family, "fwd_f32", "fwd_f64" or "fwd_generic";
 * "none" where fa_forward fails or launches nothing.  The string lives as long as the library.  (The diagnostic
 * library honours FA_FWD_VARIANT here as in the launch.) */
const char* fa_forward_kernel(const fa_problem* p, const void* Q, const void* K, const void* V);

/* Human-readable text for a status code / the calling thread's last error. */
const char* fa_error_string(int status);
const char* fa_last_error(void);

/* Library build identifier (kernel variants compiled in). */
const char* fa_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* TF_FLASH_ATTENTION_AMD_FA_API_H_ */
