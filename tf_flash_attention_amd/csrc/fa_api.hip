// fa_api.hip — C-ABI host layer (include/fa_api.h).
//
// Replaces the reference's host side: the sync-method lookup and order-map
// construction (sync_methods.{h,cc}), the per-op validation/alloc/memset in
// FlashAttention{Forward,Backward}Base::Compute (flash_attention_forward.cc:280-386,
// flash_attention_backward.cc:181-344) and the launcher
// FlashAttentionLauncher::{Forward,Backward} (flash_attention.cu:2147-2447).
// Differences by design: no memsets (kernels write every output element), no
// Br_occupancy lock array, no shared-memory opt-in dance (gfx950 exposes
// 160 KiB LDS per workgroup), and the FLOP estimate is algorithmic.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/fa_api.h"
#include "fa_device.h"
#include "fa_fwd_f16_choice.h"
#include "fa_kernels.h"
#include "fa_rules.h"

namespace fa {

// (kernel, device) pairs whose dynamic-LDS limit is already raised.  Readers take the shared
// lock; the first launch of a kernel on a device takes the exclusive one.  Replaces the
// reference's per-launch cudaFuncSetAttribute (flash_attention.cu:2269, which sits inside an
// assert and vanishes under NDEBUG — SURVEY N7).
hipError_t set_smem_once(const void* kern, int bytes) {
  struct Entry {
    const void* kern;
    int dev, bytes;
  };
  static std::shared_mutex mu;
  static std::vector<Entry> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  {
    std::shared_lock<std::shared_mutex> rd(mu);
    for (const Entry& x : done)
      if (x.kern == kern && x.dev == dev && x.bytes >= bytes) return hipSuccess;
  }
  std::unique_lock<std::shared_mutex> wr(mu);
  for (const Entry& x : done)
    if (x.kern == kern && x.dev == dev && x.bytes >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.push_back({kern, dev, bytes});
  return e;
}

int device_cus() {
  constexpr int kMaxDev = 64;
  static std::atomic<int> cache[kMaxDev];  // 0 = not queried yet (a benign race: same value)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  if (dev >= 0 && dev < kMaxDev) {
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
  }
  int cus = 0;
  if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  if (dev >= 0 && dev < kMaxDev) cache[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// XCDs the block-placement maps assume (blocks dealt round-robin over them, 32 CUs each on gfx950).
// The count is inferred from the CUs, exact only for parts built from 32-CU XCDs; any other CU count
// returns 1, which turns the XCD-aware orders into plain ones (correct for every count: the maps are
// bijections; only their L2-locality assumption needs the true count).
int device_xcds() {
  const int cus = device_cus();
  if (cus % 32 != 0) return 1;
  const int x = cus / 32;
  return x < 1 ? 1 : (x > 8 ? 8 : x);
}

}  // namespace fa

namespace {

thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int32_t next_pow2(int32_t n) {
  int32_t r = 1;
  while (r < n) r <<= 1;
  return r;
}

int32_t ilog2(int32_t n) {
  int32_t l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

int64_t seq_elems(const int32_t* s, int dims) {
  int64_t n = 1;
  for (int i = 0; i < dims; ++i) n *= s[i];
  return n;
}

// Sync methods, sync_methods.cc:8-111: per dim (last axis first) the reference
// extent is the next pow2 >= max(Mq, Mk); scale modes stride by max//M;
// scale_end offsets by stride-1.
void build_rule(const fa_problem* p, fa::Rule* r) {
  memset(r, 0, sizeof(*r));
  const int S = p->seq_dims;
  int32_t R[2] = {1, 1}, sq[2] = {1, 1}, sk[2] = {1, 1}, oq[2] = {0, 0}, ok[2] = {0, 0};
  for (int i = 0; i < S; ++i) {
    const int axis = S - 1 - i;
    const int32_t mq = p->q_seq[axis], mk = p->k_seq[axis];
    const int32_t mx = mq > mk ? mq : mk;
    R[i] = next_pow2(mx < 1 ? 1 : mx);
    if (p->sync_mode != FA_NONE_FRONT) {
      sq[i] = mq > 0 ? mx / mq : 1;
      sk[i] = mk > 0 ? mx / mk : 1;
    }
    if (p->sync_mode == FA_SCALE_END) {
      oq[i] = sq[i] - 1;
      ok[i] = sk[i] - 1;
    }
  }
  r->policy = p->policy;
  r->seq_dims = S;
  r->R0 = R[0];
  r->R1 = R[1];
  r->log2R0 = ilog2(R[0]);
  r->log2R1 = ilog2(R[1]);
  r->q.n = (int32_t)seq_elems(p->q_seq, S);
  r->k.n = (int32_t)seq_elems(p->k_seq, S);
  r->q.w = S == 2 ? p->q_seq[1] : r->q.n;
  r->k.w = S == 2 ? p->k_seq[1] : r->k.n;
  r->q.s0 = sq[0]; r->q.o0 = oq[0]; r->q.s1 = sq[1]; r->q.o1 = oq[1];
  r->k.s0 = sk[0]; r->k.o0 = ok[0]; r->k.s1 = sk[1]; r->k.o1 = ok[1];
  if (p->policy == FA_LOCAL) {
    r->ws = p->window_size;
    r->ls = p->log2_stride_size;
    r->sws = p->window_size << p->log2_stride_size;
    r->look_ahead = p->is_causal ? 1 : r->sws;  // flash_attention.h:91-95
  } else {
    r->ws = 1;
    r->sws = 1;
    r->look_ahead = 1;
  }
}

size_t acc_size(int dtype) { return dtype == FA_F64 ? 8 : 4; }
size_t elem_size(int dtype) { return dtype == FA_F16 ? 2 : (dtype == FA_F32 ? 4 : 8); }

size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

// the backward workspace: the D rows, then the lse rows, [b][nq] of the accumulator type each
struct WsLayout {
  size_t D, lse, total;
};

WsLayout ws_layout(const fa_problem* p) {
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims);
  const size_t rows = align_up(acc_size(p->dtype) * (size_t)p->b * (size_t)nq);
  return {0, rows, 2 * rows};
}

// Split-key routing of the fp16 forward.  A pure function of the problem WITHOUT b,
// so a slice's result does not depend on how the batch is sharded.
constexpr int32_t kSplitMaxQ = 128;        // one query block of the partial kernel
constexpr int32_t kSplitMinRange = 2048;   // shorter key ranges never split
constexpr int32_t kSplitTile = 64;         // the kernels' key tile
constexpr int32_t kSplitMaxChunks = 64;    // bounds the workspace beside K and V

struct SplitPlan {
  int32_t nchunks, chunk, kb, ke, k_first;
};

SplitPlan split_plan(const fa_problem* p) {
  SplitPlan s = {0, 0, 0, 0, 0};
  if (fa_validate(p) != FA_OK || p->dtype != FA_F16 || p->d > 128 || p->v_d > 128) return s;
#ifdef FA_DIAG
  // a pinned forward variant keeps measuring the kernel it names
  if (fa::diag_variant("FA_FWD_VARIANT") >= 0) return s;
#endif
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims);
  if (nq < 1 || nq > kSplitMaxQ) return s;
  fa::Rule r;
  build_rule(p, &r);
  if (r.k.n < 1) return s;
  fa::k_range_for_q_block(r, 0, (int32_t)nq - 1, &s.kb, &s.ke);
  if (s.ke - s.kb < kSplitMinRange) return s;
  s.k_first = s.kb / kSplitTile * kSplitTile;
  const int32_t span = s.ke - s.k_first;
  // a partial is nq*(v_d+3) floats per chunk beside chunk*(d+v_d) halfs of K/V: above 64 queries the
  // chunks are twice as long, so the partials stay near an eighth of the K/V bytes
  const int32_t min_chunk = nq <= 64 ? 512 : 1024;
  const int32_t capped = ((span + kSplitMaxChunks - 1) / kSplitMaxChunks + kSplitTile - 1) / kSplitTile * kSplitTile;
  s.chunk = capped > min_chunk ? capped : min_chunk;
  s.nchunks = (span + s.chunk - 1) / s.chunk;
  return s;
}

size_t split_ws_bytes(const fa_problem* p, const SplitPlan& s) {
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims);
  return align_up((size_t)p->b * (size_t)s.nchunks * (size_t)fa::fewq_record_floats(p->v_d, nq) * sizeof(float));
}

// Grouped-query routing of the fp16 forward: kv_group query slices share a K/V slice and
// are folded into the 128 rows of one workgroup at a row pitch of the next power of two >= nq.  A pure
// function of the problem WITHOUT b.  The chunks follow split_plan's formula, but there is no minimum
// range: the partial + merge pair is the only grouped path, so a short range is one chunk.
constexpr int32_t kGroupMaxRows = 128;     // the folded rows of one workgroup

struct GroupedPlan : SplitPlan {
  int32_t pitch, rows;
};

GroupedPlan grouped_plan(const fa_problem* p, int32_t kv_group, int32_t min_group = 2) {
  GroupedPlan s = {};
  if (fa_validate(p) != FA_OK || kv_group < 1) return s;
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims);
  if (nq >= 1) {  // (validated: nq <= 2^30)
    s.pitch = next_pow2((int32_t)nq);
    s.rows = (int64_t)kv_group * s.pitch <= 0x7fffffff ? kv_group * s.pitch : 0x7fffffff;
  }
  fa::Rule r;
  build_rule(p, &r);
  if (nq >= 1 && r.k.n >= 1) fa::k_range_for_q_block(r, 0, (int32_t)nq - 1, &s.kb, &s.ke);
  if (p->dtype != FA_F16 || p->d > 128 || p->v_d > 128 || kv_group < min_group) return s;
  if (s.pitch == 0 || r.k.n < 1 || (int64_t)kv_group * s.pitch > kGroupMaxRows) return s;
#ifdef FA_DIAG
  // a pinned forward variant keeps measuring the kernel it names
  if (fa::diag_variant("FA_FWD_VARIANT") >= 0) return s;
#endif
  s.k_first = s.kb / kSplitTile * kSplitTile;
  const int32_t span = s.ke - s.k_first;
  const int32_t min_chunk = s.rows <= 64 ? 512 : 1024;
  const int32_t capped = ((span + kSplitMaxChunks - 1) / kSplitMaxChunks + kSplitTile - 1) / kSplitTile * kSplitTile;
  s.chunk = capped > min_chunk ? capped : min_chunk;
  s.nchunks = (span + s.chunk - 1) / s.chunk;
  if (s.nchunks < 1) s.nchunks = 1;  // an empty range: one chunk without tiles, so the merge writes the empty rows
  return s;
}

size_t grouped_ws_bytes(const fa_problem* p, int32_t kv_group, const GroupedPlan& s) {
  return align_up((size_t)(p->b / kv_group) * (size_t)s.nchunks * (size_t)fa::fewq_record_floats(p->v_d, s.rows) * sizeof(float));
}

int check_group(const fa_problem* p, int32_t kv_group) {
  const int st = fa_validate(p);
  if (st != FA_OK) return st;
  if (kv_group < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "kv_group must be >= 1");
  if (p->b % kv_group != 0)
    return set_error(FA_ERR_INVALID_ARGUMENT, "the batch size b = " + std::to_string(p->b) +
                                                  " is not a multiple of kv_group = " + std::to_string(kv_group));
  return FA_OK;
}

// Ragged few-query forward: grouped_plan over the capacity [0, nk) of 1d sequences under the
// full rule, with ungrouped decode (kv_group == 1) inside the envelope.  The lengths are device data, so the
// plan cannot depend on them.
GroupedPlan ragged_plan(const fa_problem* p, int32_t kv_group) {
  GroupedPlan s = grouped_plan(p, kv_group, 1);
  if (p->seq_dims != 1 || p->policy != FA_FULL) s.nchunks = s.chunk = 0;
  return s;
}

int check_ragged(const fa_problem* p, int32_t kv_group) {
  const int st = check_group(p, kv_group);
  if (st != FA_OK) return st;
  if (p->policy != FA_FULL)
    return set_error(FA_ERR_INVALID_ARGUMENT, "ragged forward: the policy must be FA_FULL (the lengths and tail_causal are the mask)");
  return FA_OK;
}

// Paged few-query forward: ragged_plan over the capacity nk = max_pages * page, where a page
// is a multiple of the 64-key tile.  Neither the lengths nor the block table (device data) enter the plan.
GroupedPlan paged_plan(const fa_problem* p, int32_t kv_group, int32_t page) {
  GroupedPlan s = ragged_plan(p, kv_group);
  if (page % kSplitTile != 0) s.nchunks = s.chunk = 0;
  return s;
}

int check_paged(const fa_problem* p, int32_t kv_group, int32_t page) {
  const int st = check_ragged(p, kv_group);
  if (st != FA_OK) return st;
  if (page < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: page must be >= 1");
  if (p->seq_dims == 1 && p->k_seq[0] % page != 0)
    return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: the capacity k_seq[0] = " + std::to_string(p->k_seq[0]) +
                                                  " is not a multiple of page = " + std::to_string(page));
  return FA_OK;
}

// Sliding-window forms of the ragged and the paged forward: `base` is the un-windowed twin's
// plan.  A window that reaches the capacity cuts nothing, and the call is the twin's tail form with its plan
// (delegated).  Below it the block sees at most span_w = min(nk, W + nq - 1) keys somewhere in the capacity (where,
// the device knows): grouped_plan's chunk formula over span_w, chunk boundaries at absolute multiples of the chunk,
// and as many launched chunks as an interval of span_w keys can touch.  A pure function of the problem without b.
struct WindowPlan {
  GroupedPlan g;  // g.nchunks: the launched chunks per K/V slice
  int32_t span_w, cap_chunks, delegated;
};

WindowPlan window_plan(const fa_problem* p, const GroupedPlan& base, int32_t window) {
  WindowPlan w = {base, 0, base.nchunks, 0};
  if (base.nchunks == 0) return w;  // outside the envelope (inside it: 1d, nq >= 1, nk >= 1)
  const int64_t nq = p->q_seq[0], nk = p->k_seq[0];
  w.span_w = (int32_t)(nk < window + nq - 1 ? nk : window + nq - 1);
  w.delegated = window >= nk;
  if (w.delegated) return w;
  const int32_t min_chunk = base.rows <= 64 ? 512 : 1024;
  const int32_t capped = ((w.span_w + kSplitMaxChunks - 1) / kSplitMaxChunks + kSplitTile - 1) / kSplitTile * kSplitTile;
  w.g.chunk = capped > min_chunk ? capped : min_chunk;
  w.cap_chunks = (int32_t)((nk + w.g.chunk - 1) / w.g.chunk);
  const int32_t touched = (w.span_w + w.g.chunk - 2) / w.g.chunk + 1;
  w.g.nchunks = touched < w.cap_chunks ? touched : w.cap_chunks;
  return w;
}

int check_window(int32_t window) {
  if (window < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "windowed forward: window = " + std::to_string(window) + " must be >= 1");
  return FA_OK;
}

void write_window_plan(int32_t out[8], const WindowPlan& w) {
  out[0] = w.g.nchunks;
  out[1] = w.g.chunk;
  out[2] = w.span_w;
  out[3] = w.cap_chunks;
  out[4] = w.g.pitch;
  out[5] = w.g.rows;
  out[6] = w.delegated;
  out[7] = 0;
}

// Query-blocked forms of the ragged and the paged forward: `twin` is the un-blocked twin's plan.
// Inside the twin's envelope (kv_group * next_pow2(nq) <= 128: one block) the call is the twin's with its plan
// (delegated).  Outside it the queries are cut into nqb = ceil(nq / pb) blocks of pb queries, pb the largest power
// of two with kv_group * pb <= 128, one workgroup each per key chunk.  The chunk split exists to fill the GPU where
// the workgroups are few, the blocks already supply them, and every (block, chunk) costs a record of
// rows * (v_d + 3) floats: so at most kmax = max(1, 64 / nqb) chunks, of at least the twins' min_chunk keys.  A
// pure function of the problem without b, the lengths or the table.
struct PrefillPlan {
  GroupedPlan g;  // delegated: the twin's; else pitch = pb, rows = kv_group * pb, the chunks below
  int32_t pb, rows, nqb, delegated;
};

PrefillPlan prefill_plan(const fa_problem* p, int32_t kv_group, const GroupedPlan& twin, int32_t page_keys) {
  PrefillPlan w = {};
  if (fa_validate(p) != FA_OK || p->seq_dims != 1 || kv_group < 1 || kv_group > kGroupMaxRows) return w;
  const int64_t nq = p->q_seq[0], nk = p->k_seq[0];
  if (nq < 1 || nk < 1) return w;
  int32_t pb = 1;
  while (2 * pb * kv_group <= kGroupMaxRows) pb *= 2;
  const int32_t nqb = (int32_t)((nq + pb - 1) / pb);
  if (twin.nchunks != 0) {  // (then nqb == 1)
    w = {twin, pb, kv_group * pb, nqb, 1};
    return w;
  }
  if (nqb < 2 || p->dtype != FA_F16 || p->policy != FA_FULL || p->d > 128 || p->v_d > 128 || page_keys % kSplitTile != 0)
    return w;
#ifdef FA_DIAG
  // a pinned forward variant keeps measuring the kernel it names
  if (fa::diag_variant("FA_FWD_VARIANT") >= 0) return w;
#endif
  w = {twin, pb, kv_group * pb, nqb, 0};
  w.g.pitch = pb;
  w.g.rows = w.rows;
  w.g.kb = w.g.k_first = 0;
  w.g.ke = (int32_t)nk;
  const int32_t kmax = kSplitMaxChunks / nqb > 1 ? kSplitMaxChunks / nqb : 1;
  const int32_t min_chunk = w.rows <= 64 ? 512 : 1024;
  const int64_t tiles = (nk + kSplitTile - 1) / kSplitTile;
  const int64_t capped = (tiles + kmax - 1) / kmax * kSplitTile;
  w.g.chunk = (int32_t)(capped > min_chunk ? capped : min_chunk);
  w.g.nchunks = (int32_t)((nk + w.g.chunk - 1) / w.g.chunk);
  return w;
}

size_t prefill_ws_bytes(const fa_problem* p, int32_t kv_group, const PrefillPlan& w) {
  if (w.delegated) return grouped_ws_bytes(p, kv_group, w.g);
  return align_up((size_t)(p->b / kv_group) * (size_t)w.nqb * (size_t)w.g.nchunks *
                  (size_t)fa::fewq_record_floats(p->v_d, w.rows) * sizeof(float));
}

void write_prefill_plan(int32_t out[8], const PrefillPlan& w) {
  const bool in = w.g.nchunks != 0;
  out[0] = w.g.nchunks;
  out[1] = in ? w.g.chunk : 0;
  out[2] = in ? w.pb : 0;
  out[3] = in ? w.rows : 0;
  out[4] = in ? w.nqb : 0;
  out[5] = in ? w.delegated : 0;
  out[6] = out[7] = 0;
}

// Sliding-window forms over query blocks: the product of the two plans above.  `base` is the
// un-windowed, un-blocked twin's plan.  A window that reaches the capacity cuts nothing: the call is the
// query-blocked form's tail call with its plan (delegated = 1).  Below it, where one block holds the queries, the
// call is the windowed twin's with its plan (delegated = 2).  Otherwise block qb sees at most
// span_w = min(nk, W + pb - 1) keys somewhere in the capacity: prefill_plan's chunk formula over span_w (at most
// kmax = max(1, 64 / nqb) chunks of at least the twins' min_chunk keys), chunk boundaries at absolute multiples of
// the chunk, and as many launched chunks per block as an interval of span_w keys can touch.  A pure function of the
// problem without b, the lengths or the table.
struct WindowPrefillPlan {
  PrefillPlan pp;  // pp.g.nchunks: the launched chunks per (K/V slice, query block); pp.delegated: the parent's own
  int32_t span_w, cap_chunks, delegated;
};

WindowPrefillPlan window_prefill_plan(const fa_problem* p, int32_t kv_group, const GroupedPlan& base, int32_t page_keys,
                                      int32_t window) {
  WindowPrefillPlan w = {prefill_plan(p, kv_group, base, page_keys), 0, 0, 0};
  if (w.pp.g.nchunks == 0) return w;  // outside the envelope (inside it: 1d, nq >= 1, nk >= 1)
  const int64_t nk = p->k_seq[0];
  w.cap_chunks = w.pp.g.nchunks;
  w.span_w = (int32_t)(nk < (int64_t)window + w.pp.pb - 1 ? nk : (int64_t)window + w.pp.pb - 1);
  if (window >= nk) {
    w.delegated = 1;
    return w;
  }
  if (w.pp.delegated) {  // one block: the windowed twin
    const WindowPlan t = window_plan(p, base, window);
    w.pp.g = t.g;
    w.span_w = t.span_w;
    w.cap_chunks = t.cap_chunks;
    w.delegated = 2;
    return w;
  }
  const int32_t kmax = kSplitMaxChunks / w.pp.nqb > 1 ? kSplitMaxChunks / w.pp.nqb : 1;
  const int32_t min_chunk = w.pp.rows <= 64 ? 512 : 1024;
  const int32_t capped = ((w.span_w + kmax - 1) / kmax + kSplitTile - 1) / kSplitTile * kSplitTile;
  w.pp.g.chunk = capped > min_chunk ? capped : min_chunk;
  w.cap_chunks = (int32_t)((nk + w.pp.g.chunk - 1) / w.pp.g.chunk);
  const int32_t touched = (w.span_w + w.pp.g.chunk - 2) / w.pp.g.chunk + 1;
  w.pp.g.nchunks = touched < w.cap_chunks ? touched : w.cap_chunks;
  return w;
}

// (delegated = 2: the windowed twin's records; otherwise the query-blocked form's, its own delegation included)
size_t window_prefill_ws_bytes(const fa_problem* p, int32_t kv_group, const WindowPrefillPlan& w) {
  return w.delegated == 2 ? grouped_ws_bytes(p, kv_group, w.pp.g) : prefill_ws_bytes(p, kv_group, w.pp);
}

void write_window_prefill_plan(int32_t out[8], const WindowPrefillPlan& w) {
  const bool in = w.pp.g.nchunks != 0;
  out[0] = w.pp.g.nchunks;
  out[1] = in ? w.pp.g.chunk : 0;
  out[2] = in ? w.span_w : 0;
  out[3] = in ? w.cap_chunks : 0;
  out[4] = in ? w.pp.pb : 0;
  out[5] = in ? w.pp.rows : 0;
  out[6] = in ? w.pp.nqb : 0;
  out[7] = in ? w.delegated : 0;
}

// Split-key routing of the fp16 backward's dQ pass: the forward's plan, where the
// dQ kernel's 32-bit buffer offsets reach a slice's K / V channel rows (the b-free part of
// bwd_f16_fast_supported).  Also a pure function of the problem WITHOUT b, and a subset of the
// forward's plan (in the diagnostic library too: a pinned forward variant turns both off).
SplitPlan bwd_split_plan(const fa_problem* p) {
  const SplitPlan none = {0, 0, 0, 0, 0};
#ifdef FA_DIAG
  // a pinned backward variant keeps measuring the kernel it names
  if (fa::diag_variant("FA_BWD_VARIANT") >= 0) return none;
#endif
  const SplitPlan s = split_plan(p);
  if (s.nchunks == 0) return none;
  const int64_t nk = seq_elems(p->k_seq, p->seq_dims);
  const int64_t dm = p->d > p->v_d ? p->d : p->v_d;
  if (dm * (nk + 8) * 2 >= (int64_t(1) << 31)) return none;
  return s;
}

// the dQ partials of the split backward: b * nchunks records of d * nq floats, after ws_layout's regions
size_t bwd_split_part_bytes(const fa_problem* p, const SplitPlan& s) {
  const size_t nq = (size_t)seq_elems(p->q_seq, p->seq_dims);
  return align_up((size_t)p->b * (size_t)s.nchunks * (size_t)p->d * nq * sizeof(float));
}

// Split-query routing of the fp16 backward's dK/dV pass, the mirror of the plan above:
// one key block of both dK/dV kernels (nk <= 128) against a rule-bounded query range of at least 2048
// queries, where the kernels' 32-bit buffer offsets reach a slice's Q / dO channel rows (the b-free part
// of bwd_f16_fast_supported).  A pure function of the problem WITHOUT b.  Never active together with
// bwd_split_plan: that one needs nq <= 128 and a key range >= 2048, this one nk <= 128.
constexpr int32_t kQSplitMaxK = 128;       // one key block of the dK/dV kernels
constexpr int32_t kQSplitTile = 32;        // their query tile
constexpr int32_t kQSplitGroup = 128;      // four tiles: the producer / consumer kernel's step group

struct QSplitPlan {
  int32_t nchunks, chunk, qb, qe, q_first;
};

QSplitPlan bwd_qsplit_plan(const fa_problem* p) {
  QSplitPlan s = {0, 0, 0, 0, 0};
  if (fa_validate(p) != FA_OK || p->dtype != FA_F16 || p->d > 128 || p->v_d > 128) return s;
#ifdef FA_DIAG
  // a pinned backward variant keeps measuring the kernel it names
  if (fa::diag_variant("FA_BWD_VARIANT") >= 0) return s;
#endif
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims), nk = seq_elems(p->k_seq, p->seq_dims);
  if (nk < 1 || nk > kQSplitMaxK || nq < 1) return s;
  const int64_t dm = p->d > p->v_d ? p->d : p->v_d;
  if (dm * (nq + 8) * 2 >= (int64_t(1) << 31)) return s;
  fa::Rule r;
  build_rule(p, &r);
  fa::q_range_for_k_block(r, 0, (int32_t)nk - 1, &s.qb, &s.qe);
  if (s.qe - s.qb < kSplitMinRange) return s;
  s.q_first = s.qb / kQSplitTile * kQSplitTile;
  const int32_t span = s.qe - s.q_first;
  // a partial is nk*(d+v_d) floats per chunk beside chunk*(d+v_d) halfs of Q/dO: above 64 keys the chunks
  // are twice as long, so the partials stay within a quarter of the Q/dO bytes
  const int32_t min_chunk = nk <= 64 ? 512 : 1024;
  const int32_t capped = ((span + kSplitMaxChunks - 1) / kSplitMaxChunks + kQSplitGroup - 1) / kQSplitGroup * kQSplitGroup;
  s.chunk = capped > min_chunk ? capped : min_chunk;
  s.nchunks = (span + s.chunk - 1) / s.chunk;
  return s;
}

// the dK/dV partials of the split-query backward: b * nchunks records of (d + v_d) * nk floats, after
// ws_layout's regions
size_t bwd_qsplit_part_bytes(const fa_problem* p, const QSplitPlan& s) {
  const size_t nk = (size_t)seq_elems(p->k_seq, p->seq_dims);
  return align_up((size_t)p->b * (size_t)s.nchunks * (size_t)(p->d + p->v_d) * nk * sizeof(float));
}

// ---- what the entry points below share

// b, d, v_d, the scale and the rule of a problem (FwdArgs or BwdArgs; the pointers are the caller's)
template <class Args>
void fill_problem(const fa_problem* p, Args* a) {
  a->b = p->b; a->d = p->d; a->v_d = p->v_d;
  a->scale = 1.0 / sqrt((double)p->d);
  build_rule(p, &a->rule);
}

// the problem and a plan's chunks as the few-query kernels take them
void fill_split(const fa_problem* p, const SplitPlan& sp, fa::SplitArgs* sa) {
  fill_problem(p, &sa->f);
  sa->nchunks = sp.nchunks; sa->chunk = sp.chunk; sa->k_first = sp.k_first; sa->k_end = sp.ke;
}

void fill_grouped(const fa_problem* p, const GroupedPlan& gp, int32_t kv_group, fa::GqaArgs* ga) {
  fill_split(p, gp, &ga->s);
  ga->g = kv_group; ga->pitch = gp.pitch; ga->log2_pitch = ilog2(gp.pitch);
}

// (the lengths bound the keys: the chunks start at key 0; len0 / rem0 are set per launch)
void fill_ragged(const fa_problem* p, const GroupedPlan& gp, int32_t kv_group, const int32_t* k_lens, int32_t kv_per_len,
                 int32_t tail_causal, fa::RaggedArgs* ra) {
  fill_grouped(p, gp, kv_group, &ra->g);
  ra->g.s.k_first = 0;
  ra->k_lens = k_lens; ra->kv_per_len = kv_per_len; ra->tail_causal = tail_causal != 0;
}

// the four leading fields every plan export has; the grouped plans add the fold
void write_plan(int32_t out[4], int32_t nchunks, int32_t chunk, int32_t first, int32_t end) {
  out[0] = nchunks;
  out[1] = chunk;
  out[2] = first;
  out[3] = end;
}
void write_plan(int32_t out[4], const SplitPlan& s) { write_plan(out, s.nchunks, s.chunk, s.kb, s.ke); }
void write_plan(int32_t out[6], const GroupedPlan& s) {
  write_plan(out, static_cast<const SplitPlan&>(s));
  out[4] = s.pitch;
  out[5] = s.rows;
}

int check_kv_per_len(int64_t bkv, int32_t kv_per_len) {
  if (kv_per_len < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "kv_per_len must be >= 1");
  if (bkv % kv_per_len != 0)
    return set_error(FA_ERR_INVALID_ARGUMENT, "the number of K/V slices b / kv_group = " + std::to_string(bkv) +
                                                  " is not a multiple of kv_per_len = " + std::to_string(kv_per_len));
  return FA_OK;
}

#ifdef FA_DIAG
// Diagnostic library only: FA_SLAB_MAX, read on every call like the variant selectors, lowers the slab limit of
// the four slab loops below (fewq_slabs, bwd_slabs, fa_merge_partials, fa_accumulate_parts) so that a test can
// drive them through several iterations at small batches; the real limits (about 2^31 blocks, 65535 slices)
// are out of a test's reach or costly.  A value that is not positive, or not below the real limit, changes
// nothing.  `unit`: what one count of the variable stands for (slices; for fa_accumulate_parts 8 * kThreads
// elements of fa_merge.hip, so a slab boundary keeps the 16-byte alignment that the real limit guarantees).
// g_diag_slabs counts the slab launches (loop iterations), so the test can prove that the loop iterated.
std::atomic<long long> g_diag_slabs;
int64_t diag_slab_limit(int64_t limit, int64_t unit = 1) {
  const int64_t cap = (int64_t)fa::diag_variant("FA_SLAB_MAX") * unit;
  return cap > 0 && cap < limit ? cap : limit;
}
constexpr int64_t kAccumulateSlabUnit = 8 * 256;
#define FA_SLAB_LIMIT(...) diag_slab_limit(__VA_ARGS__)
#define FA_DIAG_SLAB() g_diag_slabs.fetch_add(1)
#else
#define FA_SLAB_LIMIT(limit, ...) (limit)
#define FA_DIAG_SLAB() ((void)0)
#endif

// A few-query forward call's pointers.  K and V null: not sliced per launch (the paged pools, set by the caller).
// kv_bytes: the size of a K / V element, 2 (fp16) or 1 (an FP8 cache).
struct FewqPtrs {
  const void *Q, *K, *V;
  void *O, *l, *m, *workspace;
  int kv_bytes = 2;
};

// The launches of a few-query forward over the p->b / g K/V slices, g query slices each, in slabs of at most
// fwd_f16_fewq_max_batch slices: one launch pair covers every realistic batch; the loop only keeps the grids
// inside 2^31 blocks.  Sets b, the slab's pointers and the workspace (records of `rows` floats a row) in *sa,
// which lies inside the arguments that launch(b0) sends; b0 is the slab's first K/V slice.  nqb: the query blocks
// of a query-blocked forward, which multiply a slice's partial workgroups and records (its merge threads are
// g * nq a channel either way).
template <class Launch>
int fewq_slabs(const fa_problem* p, const FewqPtrs& t, int32_t g, int64_t rows, fa::SplitArgs* sa, Launch&& launch,
               int32_t nqb = 1) {
  fa::FwdArgs& a = sa->f;
  const int64_t nq = a.rule.q.n, nk = a.rule.k.n, bkv = p->b / g;
  const int64_t bmax = FA_SLAB_LIMIT(fa::fwd_f16_fewq_max_batch(sa->nchunks * nqb, p->v_d, g * nq));
  for (int64_t b0 = 0; b0 < bkv; b0 += bmax) {
    a.b = bkv - b0 < bmax ? bkv - b0 : bmax;
    a.Q = static_cast<const uint16_t*>(t.Q) + b0 * g * p->d * nq;
    if (t.K) a.K = static_cast<const char*>(t.K) + b0 * p->d * nk * t.kv_bytes;
    if (t.V) a.V = static_cast<const char*>(t.V) + b0 * p->v_d * nk * t.kv_bytes;
    a.O = static_cast<uint16_t*>(t.O) + b0 * g * p->v_d * nq;
    a.l = static_cast<float*>(t.l) + b0 * g * nq;
    a.m = static_cast<uint16_t*>(t.m) + b0 * g * nq;
    sa->ws = static_cast<float*>(t.workspace) + b0 * nqb * sa->nchunks * fa::fewq_record_floats(p->v_d, rows);
    FA_DIAG_SLAB();
    const hipError_t e = launch(b0);
    if (e != hipSuccess)
      return set_error((int)e, std::string("Failed to launch the Forward kernel: ") + hipGetErrorString(e));
  }
  return FA_OK;
}

// the problem, a backward call's pointers and the regions of its workspace
void fill_bwd(const fa_problem* p, const WsLayout& w, const void* Q, const void* K, const void* V, const void* O,
              const void* l, const void* m, const void* dO, void* dQ, void* dK, void* dV, void* workspace, fa::BwdArgs* a) {
  a->Q = Q; a->K = K; a->V = V; a->O = O; a->l = l; a->m = m; a->dO = dO;
  a->dQ = dQ; a->dK = dK; a->dV = dV;
  char* ws = static_cast<char*>(workspace);
  a->reserved = nullptr;
  a->ws_D = ws + w.D;
  a->ws_lse = ws + w.lse;
  fill_problem(p, a);
}

// The launches of a split fp16 backward in slabs of at most bmax slices (grid limits, as above): *a receives
// `whole`, the whole call's arguments, advanced to the slab; launch(b0) sets its partials and sends them.
template <class Launch>
int bwd_slabs(const fa_problem* p, const fa::BwdArgs& whole, int64_t bmax, fa::BwdArgs* a, Launch&& launch) {
  const int64_t nq = whole.rule.q.n, nk = whole.rule.k.n;
  for (int64_t b0 = 0; b0 < p->b; b0 += bmax) {
    *a = whole;
    a->b = p->b - b0 < bmax ? p->b - b0 : bmax;
    a->Q = static_cast<const uint16_t*>(whole.Q) + b0 * p->d * nq;
    a->K = static_cast<const uint16_t*>(whole.K) + b0 * p->d * nk;
    a->V = static_cast<const uint16_t*>(whole.V) + b0 * p->v_d * nk;
    a->O = static_cast<const uint16_t*>(whole.O) + b0 * p->v_d * nq;
    a->l = static_cast<const float*>(whole.l) + b0 * nq;
    a->m = static_cast<const uint16_t*>(whole.m) + b0 * nq;
    a->dO = static_cast<const uint16_t*>(whole.dO) + b0 * p->v_d * nq;
    a->dQ = static_cast<uint16_t*>(whole.dQ) + b0 * p->d * nq;
    a->dK = static_cast<uint16_t*>(whole.dK) + b0 * p->d * nk;
    a->dV = static_cast<uint16_t*>(whole.dV) + b0 * p->v_d * nk;
    a->ws_D = static_cast<float*>(whole.ws_D) + b0 * nq;
    a->ws_lse = static_cast<float*>(whole.ws_lse) + b0 * nq;
    FA_DIAG_SLAB();
    const hipError_t e = launch(b0);
    if (e != hipSuccess)
      return set_error((int)e, std::string("Failed to launch the Backward kernel: ") + hipGetErrorString(e));
  }
  return FA_OK;
}

}  // namespace

extern "C" {

int fa_sync_mode_from_string(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "none_front")) return FA_NONE_FRONT;
  if (!strcmp(name, "scale_front")) return FA_SCALE_FRONT;
  if (!strcmp(name, "scale_end")) return FA_SCALE_END;
  return -1;
}

int fa_validate(const fa_problem* p) {
  if (!p) return set_error(FA_ERR_INVALID_ARGUMENT, "null problem descriptor");
  if (p->dtype < FA_F16 || p->dtype > FA_F64) return set_error(FA_ERR_INVALID_ARGUMENT, "unknown dtype");
  if (p->policy < FA_FULL || p->policy > FA_LOCAL) return set_error(FA_ERR_INVALID_ARGUMENT, "unknown attention policy");
  if (p->seq_dims != 1 && p->seq_dims != 2) return set_error(FA_ERR_INVALID_ARGUMENT, "seq_dims must be 1 or 2");
  if (p->sync_mode < FA_NONE_FRONT || p->sync_mode > FA_SCALE_END)
    return set_error(FA_ERR_INVALID_ARGUMENT, "Unsupported sync_mode");
  if (p->b < 0) return set_error(FA_ERR_INVALID_ARGUMENT, "negative batch size");
  for (int i = 0; i < p->seq_dims; ++i)
    if (p->q_seq[i] < 0 || p->k_seq[i] < 0) return set_error(FA_ERR_INVALID_ARGUMENT, "negative sequence extent");
  if (p->d < 1 || p->v_d < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "channel dimensions must be >= 1");
  const int64_t nq = seq_elems(p->q_seq, p->seq_dims), nk = seq_elems(p->k_seq, p->seq_dims);
  if (nq > 0x7fffffff || nk > 0x7fffffff)
    return set_error(FA_ERR_INVALID_ARGUMENT, "sequence sizes are limited to the int32 range (sync_methods.h:12-14)");
  int64_t ref = 1;
  for (int i = 0; i < p->seq_dims; ++i) {
    const int32_t mx = p->q_seq[i] > p->k_seq[i] ? p->q_seq[i] : p->k_seq[i];
    ref *= next_pow2(mx < 1 ? 1 : mx);
  }
  if (ref > (int64_t(1) << 30)) return set_error(FA_ERR_INVALID_ARGUMENT, "reference sequence extent exceeds 2^30");
  if (p->policy == FA_LOCAL) {
    if (p->window_size < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "window_size must be >= 1");
    if (p->log2_stride_size < 0 || p->log2_stride_size >= 31)
      return set_error(FA_ERR_INVALID_ARGUMENT, "log2_stride_size must be in [0, 31)");
    if ((int64_t(p->window_size) << p->log2_stride_size) > 0x7fffffff)
      return set_error(FA_ERR_INVALID_ARGUMENT,
                       "stride size is too big; please make sure the stride size/window size is within the range "
                       "representable by int32_t");
  }
  return FA_OK;
}

#ifdef FA_DIAG
// diagnostic library only: calls that reached a launch, so a test can prove which library ran them
static std::atomic<long long> g_diag_calls[2];
long long fa_diag_call_count(int which) { return (which == 0 || which == 1) ? g_diag_calls[which].load() : -1; }
#define FA_DIAG_COUNT(w) g_diag_calls[w].fetch_add(1)
// slab launches of the four slab loops (fewq_slabs, bwd_slabs, the merge and the accumulate loop)
long long fa_diag_slab_count(void) { return g_diag_slabs.load(); }
// FA_FWD_VARIANT / FA_BWD_VARIANT = 9000 skips the MFMA dispatch of fa_forward / fa_backward, so that a test can
// run the SIMT kernels at the small shapes they otherwise serve only when an MFMA predicate fails
#define FA_DIAG_SIMT(name) (fa::diag_variant(name) == 9000)
#else
#define FA_DIAG_COUNT(w) ((void)0)
#define FA_DIAG_SIMT(name) false
#endif

static const char kGenericUnsupported[] =
    "no kernel takes this shape: more than 65536 channels, or a launch grid of 2^31 workgroups or more";

// the kernel family of a forward call that launches something, and for fp16 the kernel (fa_fwd_f16_choice.h):
// what fa_forward launches and fa_forward_kernel names
enum class FwdFamily { kNone, kF16, kF32, kF64, kGeneric };

static FwdFamily forward_family(const fa_problem* p, const fa::FwdArgs& a, fa::FwdF16Choice* f16) {
  const bool mfma = !FA_DIAG_SIMT("FA_FWD_VARIANT");
  if (mfma && p->dtype == FA_F16 && (*f16 = fa::choose_fwd_f16(a)).kernel != fa::FwdF16::kNone) return FwdFamily::kF16;
  if (mfma && p->dtype == FA_F32 && fa::fwd_f32_supported(a)) return FwdFamily::kF32;
  if (mfma && p->dtype == FA_F64 && fa::fwd_f64_supported(a)) return FwdFamily::kF64;
  return fa::fwd_generic_supported(p->dtype, a) ? FwdFamily::kGeneric : FwdFamily::kNone;
}

int fa_forward(void* stream, const fa_problem* p, const void* Q, const void* K, const void* V, void* O, void* l,
               void* m) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  FA_DIAG_COUNT(0);
  fa::FwdArgs a;
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.l = l; a.m = m;
  fill_problem(p, &a);
  if (a.b == 0 || a.rule.q.n == 0) return FA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  fa::FwdF16Choice f16;
  hipError_t e;
  switch (forward_family(p, a, &f16)) {
    case FwdFamily::kF16: e = fa::launch_fwd_f16(a, f16, s); break;
    case FwdFamily::kF32: e = fa::launch_fwd_f32(a, s); break;
    case FwdFamily::kF64: e = fa::launch_fwd_f64(a, s); break;
    case FwdFamily::kGeneric: e = fa::launch_fwd_generic(p->dtype, a, s); break;
    default: return set_error(FA_ERR_UNSUPPORTED, kGenericUnsupported);
  }
  if (e != hipSuccess)
    return set_error((int)e, std::string("Failed to launch the Forward kernel: ") + hipGetErrorString(e));
  return FA_OK;
}

const char* fa_forward_kernel(const fa_problem* p, const void* Q, const void* K, const void* V) {
  if (fa_validate(p) != FA_OK) return "none";
  fa::FwdArgs a;
  a.Q = Q; a.K = K; a.V = V; a.O = nullptr; a.l = nullptr; a.m = nullptr;
  fill_problem(p, &a);
  if (a.b == 0 || a.rule.q.n == 0) return "none";
  fa::FwdF16Choice f16;
  switch (forward_family(p, a, &f16)) {
    case FwdFamily::kF16: break;
    case FwdFamily::kF32: return "fwd_f32";
    case FwdFamily::kF64: return "fwd_f64";
    case FwdFamily::kGeneric: return "fwd_generic";
    default: return "none";
  }
  // one copy of every name handed out, kept for the life of the library
  static std::mutex mu;
  static std::set<std::string> names;
  std::lock_guard<std::mutex> lock(mu);
  return names.insert(fa::fwd_f16_choice_name(f16)).first->c_str();
}

size_t fa_forward_workspace_bytes(const fa_problem* p) {
  const SplitPlan s = split_plan(p);
  return s.nchunks ? split_ws_bytes(p, s) : 0;
}

int fa_forward_split_plan(const fa_problem* p, int32_t out[4]) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null plan buffer");
  write_plan(out, split_plan(p));
  return FA_OK;
}

int fa_forward_ws(void* stream, const fa_problem* p, const void* Q, const void* K, const void* V, void* O, void* l,
                  void* m, void* workspace, size_t workspace_bytes) {
  const SplitPlan sp = split_plan(p);
  if (sp.nchunks == 0) return fa_forward(stream, p, Q, K, V, O, l, m);
  if (!workspace || workspace_bytes < split_ws_bytes(p, sp))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL, "forward workspace is smaller than fa_forward_workspace_bytes()");
  FA_DIAG_COUNT(0);
  if (p->b == 0) return FA_OK;
  fa::SplitArgs sa;
  fill_split(p, sp, &sa);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return fewq_slabs(p, {Q, K, V, O, l, m, workspace}, 1, sa.f.rule.q.n, &sa,
                    [&](int64_t) { return fa::launch_fwd_f16_splitk(sa, s); });
}

int fa_forward_grouped_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]) {
  const int st = check_group(p, kv_group);
  if (st != FA_OK) return st;
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null plan buffer");
  write_plan(out, grouped_plan(p, kv_group));
  return FA_OK;
}

size_t fa_forward_grouped_workspace_bytes(const fa_problem* p, int32_t kv_group) {
  if (check_group(p, kv_group) != FA_OK) return 0;
  if (kv_group == 1) return fa_forward_workspace_bytes(p);
  const GroupedPlan s = grouped_plan(p, kv_group);
  return s.nchunks ? grouped_ws_bytes(p, kv_group, s) : 0;
}

int fa_forward_grouped(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K, const void* V,
                       void* O, void* l, void* m, void* workspace, size_t workspace_bytes) {
  const int st = check_group(p, kv_group);
  if (st != FA_OK) return st;
  if (kv_group == 1) return fa_forward_ws(stream, p, Q, K, V, O, l, m, workspace, workspace_bytes);
  const GroupedPlan gp = grouped_plan(p, kv_group);
  if (gp.nchunks == 0)
    return set_error(FA_ERR_UNSUPPORTED,
                     "grouped forward: outside the fused envelope (fp16, max(d, v_d) <= 128, kv_group * pitch <= 128, "
                     "nq >= 1, nk >= 1); expand K and V and call fa_forward_ws");
  if (!workspace || workspace_bytes < grouped_ws_bytes(p, kv_group, gp))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL,
                     "forward workspace is smaller than fa_forward_grouped_workspace_bytes()");
  FA_DIAG_COUNT(0);
  if (p->b == 0) return FA_OK;
  fa::GqaArgs ga;
  fill_grouped(p, gp, kv_group, &ga);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return fewq_slabs(p, {Q, K, V, O, l, m, workspace}, kv_group, gp.rows, &ga.s,
                    [&](int64_t) { return fa::launch_fwd_f16_gqa(ga, s); });
}

// ---- the decode forwards (include/fa_api.h): a K/V cache times a form.  The cache
// is ragged or paged, fp16 or FP8; the form plain, sliding-window, query-blocked or tree-masked.  What a call is:
struct PagedPart {  // the block table of a paged cache
  const int32_t* block_table;
  int32_t max_pages, page;
  int64_t num_pages;
};
struct Kv8 {  // the scales of an FP8 cache (either may be null)
  const float *k_scale, *v_scale;
};
struct DecodeKind {
  const PagedPart* paged;  // null: a ragged cache
  const Kv8* kv8;          // null: an fp16 cache
  const int32_t* window;   // null: no window
  bool prefill;            // the query-blocked form
  bool tree;               // the tree-masked draft form, with
  const uint32_t* mask;    //   its device mask [sequences][nq][ceil(nq / 32)] (checked where k_lens is)
};

// the words of one sequence's draft mask: nq rows of ceil(nq / 32)
static int64_t tree_mask_words(int64_t nq) { return nq * ((nq + 31) / 32); }

// the checks and the un-windowed, un-blocked plan of a cache; `page` null: ragged
static int check_cache(const fa_problem* p, int32_t kv_group, const int32_t* page) {
  return page ? check_paged(p, kv_group, *page) : check_ragged(p, kv_group);
}
static GroupedPlan cache_plan(const fa_problem* p, int32_t kv_group, const int32_t* page) {
  return page ? paged_plan(p, kv_group, *page) : ragged_plan(p, kv_group);
}

// the _plan and _workspace_bytes entry points of every cache and form (the FP8 caches share the fp16 ones')
static int decode_plan(const fa_problem* p, int32_t kv_group, const int32_t* page, const int32_t* window, bool prefill,
                       int32_t* out) {
  const int st = check_cache(p, kv_group, page);
  if (st != FA_OK) return st;
  const int wst = window ? check_window(*window) : FA_OK;
  if (wst != FA_OK) return wst;
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null plan buffer");
  const GroupedPlan base = cache_plan(p, kv_group, page);
  if (window && prefill) write_window_prefill_plan(out, window_prefill_plan(p, kv_group, base, page ? *page : 0, *window));
  else if (window) write_window_plan(out, window_plan(p, base, *window));
  else if (prefill) write_prefill_plan(out, prefill_plan(p, kv_group, base, page ? *page : 0));
  else write_plan(out, base);
  return FA_OK;
}

static size_t decode_workspace_bytes(const fa_problem* p, int32_t kv_group, const int32_t* page, const int32_t* window,
                                     bool prefill) {
  if (check_cache(p, kv_group, page) != FA_OK || (window && check_window(*window) != FA_OK)) return 0;
  const GroupedPlan base = cache_plan(p, kv_group, page);
  if (window && prefill) {
    const WindowPrefillPlan w = window_prefill_plan(p, kv_group, base, page ? *page : 0, *window);
    return w.pp.g.nchunks ? window_prefill_ws_bytes(p, kv_group, w) : 0;
  }
  if (prefill) {
    const PrefillPlan w = prefill_plan(p, kv_group, base, page ? *page : 0);
    return w.g.nchunks ? prefill_ws_bytes(p, kv_group, w) : 0;
  }
  const GroupedPlan g = window ? window_plan(p, base, *window).g : base;
  return g.nchunks ? grouped_ws_bytes(p, kv_group, g) : 0;
}

// Every decode forward: the same checks, plan, workspace and launches.  K and V are the cache or the pools.  With
// a window the sliding-window form: the tail form itself where the window reaches the capacity, else the window's
// plan and kernels.  With `prefill` the query-blocked form: the twin itself where one block holds the queries, else
// the blocked plan and kernels.  With both the sliding-window form over query blocks: the query-blocked tail call
// itself where the window reaches the capacity, else the windowed twin itself where one block holds the queries
// (either is the parent's own call: its checks, plan, workspace size and bits), else the product's plan and
// kernels.  With `tree` the tree-masked draft form: the plain plan and workspace, the tree
// kernels, and `tail_causal` unread (the draft slots' positions are the tail's).
static int forward_decode(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K, const void* V,
                          const DecodeKind& c, const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal, void* O,
                          void* l, void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart* pg = c.paged;
  const int32_t* page = pg ? &pg->page : nullptr;
  const std::string name = pg ? "paged" : "ragged";
  const int st = check_cache(p, kv_group, page);
  if (st != FA_OK) return st;
  const int kst = check_kv_per_len(p->b / kv_group, kv_per_len);
  if (kst != FA_OK) return kst;
  const int wst = c.window ? check_window(*c.window) : FA_OK;
  if (wst != FA_OK) return wst;
  if (pg) {
    if (pg->max_pages < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: max_pages must be >= 1");
    if ((int64_t)pg->max_pages * pg->page != p->k_seq[0])
      return set_error(FA_ERR_INVALID_ARGUMENT,
                       "paged forward: max_pages * page = " + std::to_string((int64_t)pg->max_pages * pg->page) +
                           " is not the capacity k_seq[0] = " + std::to_string(p->k_seq[0]));
    if (pg->num_pages < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: num_pages must be >= 1");
  }
  const GroupedPlan base = cache_plan(p, kv_group, page);
  const bool both = c.window && c.prefill;
  const WindowPrefillPlan wpp = both ? window_prefill_plan(p, kv_group, base, pg ? pg->page : 0, *c.window) : WindowPrefillPlan{};
  if (wpp.delegated == 1)
    return forward_decode(stream, p, kv_group, Q, K, V, {c.paged, c.kv8, nullptr, true}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
  if (wpp.delegated == 2)
    return forward_decode(stream, p, kv_group, Q, K, V, {c.paged, c.kv8, c.window}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
  const WindowPlan wp = both ? WindowPlan{} : window_plan(p, base, c.window ? *c.window : 0x7fffffff);
  const PrefillPlan pp = both ? wpp.pp : c.prefill ? prefill_plan(p, kv_group, wp.g, pg ? pg->page : 0) : PrefillPlan{};
  const bool blocked = c.prefill && !pp.delegated;
  const GroupedPlan& gp = blocked || both ? pp.g : wp.g;
  const bool win = c.window && !both && !wp.delegated;
  if (gp.nchunks == 0)
    return set_error(FA_ERR_UNSUPPORTED,
                     name + (both ? " windowed" : "") + (c.prefill ? " prefill forward: outside the envelope (fp16, 1d sequences, max(d, v_d) <= 128, "
                                         "1 <= kv_group <= 128, nq >= 1, nk >= 1"
                                       : " forward: outside the fused envelope (fp16, 1d sequences, max(d, v_d) <= 128, "
                                         "kv_group * pitch <= 128, nq >= 1, nk >= 1") +
                         (pg ? ", page % 64 == 0)" : ")"));
  if (!workspace || workspace_bytes < (blocked ? prefill_ws_bytes(p, kv_group, pp) : grouped_ws_bytes(p, kv_group, gp)))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL, "forward workspace is smaller than fa_forward_" + name +
                                                     (both ? "_window" : "") + (c.prefill ? "_prefill" : "") + "_workspace_bytes()");
  FA_DIAG_COUNT(0);
  if (p->b == 0) return FA_OK;
  if (!k_lens) return set_error(FA_ERR_INVALID_ARGUMENT, "null k_lens");
  if (pg && !pg->block_table) return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: null block_table");
  if (pg && (!K || !V)) return set_error(FA_ERR_INVALID_ARGUMENT, "paged forward: null K_pool or V_pool");
  if (c.tree && !c.mask) return set_error(FA_ERR_INVALID_ARGUMENT, name + " tree forward: null draft_mask");
  fa::PagedFp8Args all = {};  // the widest cache's arguments: a narrower cache sends the part it has
  fa::PagedArgs& pa = all.p;
  fa::RaggedArgs& ra = pa.r;
  fill_ragged(p, gp, kv_group, k_lens, kv_per_len, tail_causal, &ra);
  if (c.kv8) { all.k_scale = c.kv8->k_scale; all.v_scale = c.kv8->v_scale; }
  FewqPtrs ptrs = {Q, K, V, O, l, m, workspace, c.kv8 ? 1 : 2};
  if (pg) {
    pa.block_table = pg->block_table; pa.max_pages = pg->max_pages; pa.page = pg->page;
    pa.last_page = (int32_t)(pg->num_pages - 1 < 0x7fffffff ? pg->num_pages - 1 : 0x7fffffff);  // (an int32 entry reaches no further)
    ra.g.s.f.K = K; ra.g.s.f.V = V;  // the pools are not sliced per launch: the table says where a slice's keys are
    ptrs.K = ptrs.V = nullptr;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the form picks the launcher, the argument struct its instance
  auto launch = [&](const auto& args) {
    using Args = std::decay_t<decltype(args)>;
    if (both) return fa::launch_fwd_f16_window_prefill<Args>({args, *c.window, pp.nqb}, s);
    if (win) return fa::launch_fwd_f16_window<Args>({args, *c.window}, s);
    if (blocked) return fa::launch_fwd_f16_prefill<Args>({args, pp.nqb}, s);
    // (the mask advances by sequences with the slab, as len0 does: the kernel counts from the launch's first)
    if (c.tree) return fa::launch_fwd_f16_tree<Args>({args, c.mask + ra.len0 * tree_mask_words(p->q_seq[0])}, s);
    return fa::launch_fwd_f16_decode(args, s);
  };
  return fewq_slabs(p, ptrs, kv_group, gp.rows, &ra.g.s, [&](int64_t b0) {
    ra.len0 = b0 / kv_per_len; ra.rem0 = (int32_t)(b0 % kv_per_len);
    if (pg && c.kv8) return launch(all);
    if (pg) return launch(pa);
    if (c.kv8) return launch(fa::RaggedFp8Args{ra, all.k_scale, all.v_scale});
    return launch(ra);
  }, blocked ? pp.nqb : 1);
}

// the twelve forwards and their plans: ragged / paged, then the same with a window (the tail rule is implied) and
// over query blocks
int fa_forward_ragged_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]) {
  return decode_plan(p, kv_group, nullptr, nullptr, false, out);
}
size_t fa_forward_ragged_workspace_bytes(const fa_problem* p, int32_t kv_group) {
  return decode_workspace_bytes(p, kv_group, nullptr, nullptr, false);
}
int fa_forward_paged_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[6]) {
  return decode_plan(p, kv_group, &page, nullptr, false, out);
}
size_t fa_forward_paged_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page) {
  return decode_workspace_bytes(p, kv_group, &page, nullptr, false);
}
int fa_forward_ragged_window_plan(const fa_problem* p, int32_t kv_group, int32_t window, int32_t out[8]) {
  return decode_plan(p, kv_group, nullptr, &window, false, out);
}
size_t fa_forward_ragged_window_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t window) {
  return decode_workspace_bytes(p, kv_group, nullptr, &window, false);
}
int fa_forward_paged_window_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window, int32_t out[8]) {
  return decode_plan(p, kv_group, &page, &window, false, out);
}
size_t fa_forward_paged_window_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window) {
  return decode_workspace_bytes(p, kv_group, &page, &window, false);
}
int fa_forward_ragged_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t out[8]) {
  return decode_plan(p, kv_group, nullptr, nullptr, true, out);
}
size_t fa_forward_ragged_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group) {
  return decode_workspace_bytes(p, kv_group, nullptr, nullptr, true);
}
int fa_forward_paged_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[8]) {
  return decode_plan(p, kv_group, &page, nullptr, true, out);
}
size_t fa_forward_paged_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page) {
  return decode_workspace_bytes(p, kv_group, &page, nullptr, true);
}

int fa_forward_ragged(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K, const void* V,
                      const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal, void* O, void* l, void* m,
                      void* workspace, size_t workspace_bytes) {
  return forward_decode(stream, p, kv_group, Q, K, V, {}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K8,
                          const void* V8, const float* k_scale, const float* v_scale, const int32_t* k_lens,
                          int32_t kv_per_len, int32_t tail_causal, void* O, void* l, void* m, void* workspace,
                          size_t workspace_bytes) {
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K8, V8, {nullptr, &kv8}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool,
                     const void* V_pool, const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                     const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal, void* O, void* l, void* m,
                     void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return forward_decode(stream, p, kv_group, Q, K_pool, V_pool, {&pg}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool8,
                         const void* V_pool8, const float* k_scale, const float* v_scale, const int32_t* block_table,
                         int32_t max_pages, int32_t page, int64_t num_pages, const int32_t* k_lens, int32_t kv_per_len,
                         int32_t tail_causal, void* O, void* l, void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K_pool8, V_pool8, {&pg, &kv8}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_window(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K,
                             const void* V, const int32_t* k_lens, int32_t kv_per_len, int32_t window, void* O, void* l,
                             void* m, void* workspace, size_t workspace_bytes) {
  return forward_decode(stream, p, kv_group, Q, K, V, {nullptr, nullptr, &window}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_window_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K8,
                                 const void* V8, const float* k_scale, const float* v_scale, const int32_t* k_lens,
                                 int32_t kv_per_len, int32_t window, void* O, void* l, void* m, void* workspace,
                                 size_t workspace_bytes) {
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K8, V8, {nullptr, &kv8, &window}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_window(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool,
                            const void* V_pool, const int32_t* block_table, int32_t max_pages, int32_t page,
                            int64_t num_pages, const int32_t* k_lens, int32_t kv_per_len, int32_t window, void* O, void* l,
                            void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return forward_decode(stream, p, kv_group, Q, K_pool, V_pool, {&pg, nullptr, &window}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_window_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool8,
                                const void* V_pool8, const float* k_scale, const float* v_scale, const int32_t* block_table,
                                int32_t max_pages, int32_t page, int64_t num_pages, const int32_t* k_lens,
                                int32_t kv_per_len, int32_t window, void* O, void* l, void* m, void* workspace,
                                size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K_pool8, V_pool8, {&pg, &kv8, &window}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_prefill(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K,
                              const void* V, const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal, void* O,
                              void* l, void* m, void* workspace, size_t workspace_bytes) {
  return forward_decode(stream, p, kv_group, Q, K, V, {nullptr, nullptr, nullptr, true}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K8,
                                  const void* V8, const float* k_scale, const float* v_scale, const int32_t* k_lens,
                                  int32_t kv_per_len, int32_t tail_causal, void* O, void* l, void* m, void* workspace,
                                  size_t workspace_bytes) {
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K8, V8, {nullptr, &kv8, nullptr, true}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_prefill(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool,
                             const void* V_pool, const int32_t* block_table, int32_t max_pages, int32_t page,
                             int64_t num_pages, const int32_t* k_lens, int32_t kv_per_len, int32_t tail_causal, void* O,
                             void* l, void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return forward_decode(stream, p, kv_group, Q, K_pool, V_pool, {&pg, nullptr, nullptr, true}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool8,
                                 const void* V_pool8, const float* k_scale, const float* v_scale, const int32_t* block_table,
                                 int32_t max_pages, int32_t page, int64_t num_pages, const int32_t* k_lens,
                                 int32_t kv_per_len, int32_t tail_causal, void* O, void* l, void* m, void* workspace,
                                 size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K_pool8, V_pool8, {&pg, &kv8, nullptr, true}, k_lens, kv_per_len, tail_causal, O, l, m, workspace, workspace_bytes);
}

// the sliding-window forms over query blocks: the `_window` signatures with the prefill forms' envelope
int fa_forward_ragged_window_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t window, int32_t out[8]) {
  return decode_plan(p, kv_group, nullptr, &window, true, out);
}
size_t fa_forward_ragged_window_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t window) {
  return decode_workspace_bytes(p, kv_group, nullptr, &window, true);
}
int fa_forward_paged_window_prefill_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window, int32_t out[8]) {
  return decode_plan(p, kv_group, &page, &window, true, out);
}
size_t fa_forward_paged_window_prefill_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page, int32_t window) {
  return decode_workspace_bytes(p, kv_group, &page, &window, true);
}

int fa_forward_ragged_window_prefill(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K,
                                     const void* V, const int32_t* k_lens, int32_t kv_per_len, int32_t window, void* O,
                                     void* l, void* m, void* workspace, size_t workspace_bytes) {
  return forward_decode(stream, p, kv_group, Q, K, V, {nullptr, nullptr, &window, true}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_window_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K8,
                                         const void* V8, const float* k_scale, const float* v_scale, const int32_t* k_lens,
                                         int32_t kv_per_len, int32_t window, void* O, void* l, void* m, void* workspace,
                                         size_t workspace_bytes) {
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K8, V8, {nullptr, &kv8, &window, true}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_window_prefill(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool,
                                    const void* V_pool, const int32_t* block_table, int32_t max_pages, int32_t page,
                                    int64_t num_pages, const int32_t* k_lens, int32_t kv_per_len, int32_t window, void* O,
                                    void* l, void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return forward_decode(stream, p, kv_group, Q, K_pool, V_pool, {&pg, nullptr, &window, true}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_window_prefill_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q,
                                        const void* K_pool8, const void* V_pool8, const float* k_scale, const float* v_scale,
                                        const int32_t* block_table, int32_t max_pages, int32_t page, int64_t num_pages,
                                        const int32_t* k_lens, int32_t kv_per_len, int32_t window, void* O, void* l, void* m,
                                        void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K_pool8, V_pool8, {&pg, &kv8, &window, true}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

// the tree-masked draft forms: the plain twins' plan and workspace (the mask changes neither), and the twins'
// signatures with the device mask in the place of tail_causal
int fa_forward_ragged_tree_plan(const fa_problem* p, int32_t kv_group, int32_t out[6]) {
  return decode_plan(p, kv_group, nullptr, nullptr, false, out);
}
size_t fa_forward_ragged_tree_workspace_bytes(const fa_problem* p, int32_t kv_group) {
  return decode_workspace_bytes(p, kv_group, nullptr, nullptr, false);
}
int fa_forward_paged_tree_plan(const fa_problem* p, int32_t kv_group, int32_t page, int32_t out[6]) {
  return decode_plan(p, kv_group, &page, nullptr, false, out);
}
size_t fa_forward_paged_tree_workspace_bytes(const fa_problem* p, int32_t kv_group, int32_t page) {
  return decode_workspace_bytes(p, kv_group, &page, nullptr, false);
}

int fa_forward_ragged_tree(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K,
                           const void* V, const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask, void* O,
                           void* l, void* m, void* workspace, size_t workspace_bytes) {
  return forward_decode(stream, p, kv_group, Q, K, V, {nullptr, nullptr, nullptr, false, true, draft_mask}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_ragged_tree_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K8,
                               const void* V8, const float* k_scale, const float* v_scale, const int32_t* k_lens,
                               int32_t kv_per_len, const uint32_t* draft_mask, void* O, void* l, void* m, void* workspace,
                               size_t workspace_bytes) {
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K8, V8, {nullptr, &kv8, nullptr, false, true, draft_mask}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_tree(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool,
                          const void* V_pool, const int32_t* block_table, int32_t max_pages, int32_t page,
                          int64_t num_pages, const int32_t* k_lens, int32_t kv_per_len, const uint32_t* draft_mask, void* O,
                          void* l, void* m, void* workspace, size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return forward_decode(stream, p, kv_group, Q, K_pool, V_pool, {&pg, nullptr, nullptr, false, true, draft_mask}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

int fa_forward_paged_tree_fp8(void* stream, const fa_problem* p, int32_t kv_group, const void* Q, const void* K_pool8,
                              const void* V_pool8, const float* k_scale, const float* v_scale, const int32_t* block_table,
                              int32_t max_pages, int32_t page, int64_t num_pages, const int32_t* k_lens,
                              int32_t kv_per_len, const uint32_t* draft_mask, void* O, void* l, void* m, void* workspace,
                              size_t workspace_bytes) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return forward_decode(stream, p, kv_group, Q, K_pool8, V_pool8, {&pg, &kv8, nullptr, false, true, draft_mask}, k_lens, kv_per_len, 1, O, l, m, workspace, workspace_bytes);
}

// ---- the fused K/V append of the same four caches (include/fa_api.h): every check on the host
// before any device call, then one launch of fa_cache_append.hip's kernel.  No workspace, no plan.
static int cache_append(void* stream, int64_t sequences, int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new,
                        int32_t nk, const void* K_new, const void* V_new, void* K, void* V, const Kv8* kv8,
                        const PagedPart* pg, const int32_t* k_lens, const int32_t* new_lens) {
  const std::string name = pg ? "paged append" : "ragged append";
  if (sequences < 0 || n_new < 0)
    return set_error(FA_ERR_INVALID_ARGUMENT, name + ": sequences = " + std::to_string(sequences) + " and n_new = " +
                                                  std::to_string(n_new) + " must not be negative");
  if (kv_heads < 1 || d < 1 || v_d < 1 || nk < 1)
    return set_error(FA_ERR_INVALID_ARGUMENT, name + ": kv_heads = " + std::to_string(kv_heads) + ", d = " + std::to_string(d) +
                                                  ", v_d = " + std::to_string(v_d) + " and nk = " + std::to_string(nk) +
                                                  " must be >= 1");
  if (pg) {
    if (pg->page < 1) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": page must be >= 1");
    if (pg->max_pages < 1) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": max_pages must be >= 1");
    if ((int64_t)pg->max_pages * pg->page != nk)
      return set_error(FA_ERR_INVALID_ARGUMENT,
                       name + ": max_pages * page = " + std::to_string((int64_t)pg->max_pages * pg->page) +
                           " is not the capacity nk = " + std::to_string(nk));
    if (pg->num_pages < 1) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": num_pages must be >= 1");
    if (pg->page % kSplitTile != 0)
      return set_error(FA_ERR_UNSUPPORTED, name + ": outside the envelope (page % 64 == 0), got page = " + std::to_string(pg->page));
  }
  if (sequences == 0 || n_new == 0) return FA_OK;
  if (!K_new || !V_new) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": null K_new or V_new");
  if (!K || !V) return set_error(FA_ERR_INVALID_ARGUMENT, name + (pg ? ": null K_pool or V_pool" : ": null K or V"));
  if (!k_lens) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": null k_lens");
  if (pg && !pg->block_table) return set_error(FA_ERR_INVALID_ARGUMENT, name + ": null block_table");
  // one thread per (channel row, 8-key chunk), 256 to a block, the blocks of a (sequence, head) together: a grid
  // that holds fewer blocks than that would have to read more of K_new than a device holds, so there is no slab loop
  const int64_t kMaxBlocks = 0x7fffffff;
  const int64_t chunks = ((int64_t)n_new + 14) / 8, slice_threads = ((int64_t)d + v_d) * chunks;
  const int64_t slice_blocks = (slice_threads + 255) / 256;
  if (slice_threads > kMaxBlocks || sequences > kMaxBlocks || sequences * kv_heads > kMaxBlocks / slice_blocks)
    return set_error(FA_ERR_UNSUPPORTED, name + ": sequences * kv_heads * ceil((d + v_d) * ((n_new + 14) / 8) / 256) "
                                                "blocks do not fit one launch of 2^31 - 1 blocks");
  fa::AppendArgs a = {};
  a.K_new = K_new; a.V_new = V_new; a.K = K; a.V = V;
  if (kv8) { a.k_scale = kv8->k_scale; a.v_scale = kv8->v_scale; }
  if (pg) {
    a.block_table = pg->block_table; a.max_pages = pg->max_pages; a.page = pg->page;
    a.last_page = (int32_t)(pg->num_pages - 1 < 0x7fffffff ? pg->num_pages - 1 : 0x7fffffff);  // (an int32 entry reaches no further)
  }
  a.k_lens = k_lens; a.new_lens = new_lens;
  a.kv_heads = kv_heads; a.d = d; a.v_d = v_d; a.n_new = n_new; a.nk = nk;
  a.chunks = (int32_t)chunks; a.slice_blocks = (int32_t)slice_blocks;
  const hipError_t e = fa::launch_cache_append(pg != nullptr, kv8 != nullptr, a, sequences * kv_heads * slice_blocks,
                                               static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return set_error((int)e, std::string("Failed to launch the append kernel: ") + hipGetErrorString(e));
  return FA_OK;
}

int fa_append_ragged(void* stream, int64_t sequences, int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                     const void* K_new, const void* V_new, void* K, void* V, const int32_t* k_lens,
                     const int32_t* new_lens) {
  return cache_append(stream, sequences, kv_heads, d, v_d, n_new, nk, K_new, V_new, K, V, nullptr, nullptr, k_lens, new_lens);
}

int fa_append_paged(void* stream, int64_t sequences, int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new, int32_t nk,
                    const void* K_new, const void* V_new, void* K_pool, void* V_pool, const int32_t* block_table,
                    int32_t max_pages, int32_t page, int64_t num_pages, const int32_t* k_lens, const int32_t* new_lens) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  return cache_append(stream, sequences, kv_heads, d, v_d, n_new, nk, K_new, V_new, K_pool, V_pool, nullptr, &pg, k_lens, new_lens);
}

int fa_append_ragged_fp8(void* stream, int64_t sequences, int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new,
                         int32_t nk, const void* K_new, const void* V_new, void* K8, void* V8, const float* k_scale,
                         const float* v_scale, const int32_t* k_lens, const int32_t* new_lens) {
  const Kv8 kv8 = {k_scale, v_scale};
  return cache_append(stream, sequences, kv_heads, d, v_d, n_new, nk, K_new, V_new, K8, V8, &kv8, nullptr, k_lens, new_lens);
}

int fa_append_paged_fp8(void* stream, int64_t sequences, int32_t kv_heads, int32_t d, int32_t v_d, int32_t n_new,
                        int32_t nk, const void* K_new, const void* V_new, void* K_pool8, void* V_pool8,
                        const float* k_scale, const float* v_scale, const int32_t* block_table, int32_t max_pages,
                        int32_t page, int64_t num_pages, const int32_t* k_lens, const int32_t* new_lens) {
  const PagedPart pg = {block_table, max_pages, page, num_pages};
  const Kv8 kv8 = {k_scale, v_scale};
  return cache_append(stream, sequences, kv_heads, d, v_d, n_new, nk, K_new, V_new, K_pool8, V_pool8, &kv8, &pg, k_lens, new_lens);
}

size_t fa_backward_workspace_bytes(const fa_problem* p) {
  if (fa_validate(p) != FA_OK) return 0;
  return ws_layout(p).total;
}

int fa_backward(void* stream, const fa_problem* p, const void* Q, const void* K, const void* V, const void* O,
                const void* l, const void* m, const void* dO, void* dQ, void* dK, void* dV, void* workspace,
                size_t workspace_bytes) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  const WsLayout w = ws_layout(p);
  if (workspace_bytes < w.total || (!workspace && w.total > 0))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL, "backward workspace is smaller than fa_backward_workspace_bytes()");
  FA_DIAG_COUNT(1);
  fa::BwdArgs a;
  fill_bwd(p, w, Q, K, V, O, l, m, dO, dQ, dK, dV, workspace, &a);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.b == 0) return FA_OK;
  const bool mfma = !FA_DIAG_SIMT("FA_BWD_VARIANT");
  hipError_t e = hipSuccess;
  if (a.rule.q.n == 0 || a.rule.k.n == 0) {
    // nothing attends: every gradient is zero
    const size_t es = elem_size(p->dtype);
    if (a.rule.q.n) e = hipMemsetAsync(dQ, 0, es * (size_t)a.b * a.d * a.rule.q.n, s);
    if (e == hipSuccess && a.rule.k.n) e = hipMemsetAsync(dK, 0, es * (size_t)a.b * a.d * a.rule.k.n, s);
    if (e == hipSuccess && a.rule.k.n) e = hipMemsetAsync(dV, 0, es * (size_t)a.b * a.v_d * a.rule.k.n, s);
  } else if (mfma && p->dtype == FA_F16 && fa::bwd_f16_fast_supported(a)) {
    e = fa::launch_bwd_f16_fast(a, s);
  } else if (mfma && p->dtype == FA_F32 && fa::bwd_f32_supported(a)) {
    e = fa::launch_bwd_f32(a, s);
  } else if (mfma && p->dtype == FA_F64 && fa::bwd_f64_supported(a)) {
    e = fa::launch_bwd_f64(a, s);
  } else if (fa::bwd_generic_supported(p->dtype, a)) {
    e = fa::launch_bwd_generic(p->dtype, a, s);
  } else {
    return set_error(FA_ERR_UNSUPPORTED, kGenericUnsupported);
  }
  if (e != hipSuccess)
    return set_error((int)e, std::string("Failed to launch the Backward kernel: ") + hipGetErrorString(e));
  return FA_OK;
}

int fa_backward_split_plan(const fa_problem* p, int32_t out[4]) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null plan buffer");
  write_plan(out, bwd_split_plan(p));
  return FA_OK;
}

int fa_backward_split_q_plan(const fa_problem* p, int32_t out[4]) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null plan buffer");
  const QSplitPlan s = bwd_qsplit_plan(p);
  write_plan(out, s.nchunks, s.chunk, s.qb, s.qe);
  return FA_OK;
}

size_t fa_backward_split_workspace_bytes(const fa_problem* p) {
  if (fa_validate(p) != FA_OK) return 0;
  const SplitPlan s = bwd_split_plan(p);
  const QSplitPlan qs = bwd_qsplit_plan(p);  // (never both: see bwd_qsplit_plan)
  return ws_layout(p).total + (s.nchunks ? bwd_split_part_bytes(p, s) : 0) + (qs.nchunks ? bwd_qsplit_part_bytes(p, qs) : 0);
}

namespace {

// fa_backward_split for a problem with query chunks: the dK/dV pass split over them
int backward_split_q(void* stream, const fa_problem* p, const QSplitPlan& qp, const void* Q, const void* K, const void* V,
                     const void* O, const void* l, const void* m, const void* dO, void* dQ, void* dK, void* dV,
                     void* workspace, size_t workspace_bytes) {
  const WsLayout w = ws_layout(p);
  if (!workspace || workspace_bytes < w.total + bwd_qsplit_part_bytes(p, qp))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL,
                     "backward workspace is smaller than fa_backward_split_workspace_bytes()");
  FA_DIAG_COUNT(1);
  if (p->b == 0) return FA_OK;
  fa::BwdQSplitArgs sa;
  fa::BwdArgs whole;
  fill_bwd(p, w, Q, K, V, O, l, m, dO, dQ, dK, dV, workspace, &whole);
  sa.b = whole;  // (the batch limit below reads the problem)
  sa.nchunks = qp.nchunks; sa.chunk = qp.chunk; sa.q_first = qp.q_first; sa.q_end = qp.qe;
  float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return bwd_slabs(p, whole, FA_SLAB_LIMIT(fa::bwd_f16_qsplit_max_batch(sa)), &sa.b, [&](int64_t b0) {
    sa.ws_part = part + b0 * qp.nchunks * (p->d + p->v_d) * whole.rule.k.n;
    return fa::launch_bwd_f16_qsplit(sa, s);
  });
}

}  // namespace

int fa_backward_split(void* stream, const fa_problem* p, const void* Q, const void* K, const void* V, const void* O,
                      const void* l, const void* m, const void* dO, void* dQ, void* dK, void* dV, void* workspace,
                      size_t workspace_bytes) {
  const SplitPlan sp = bwd_split_plan(p);
  if (sp.nchunks == 0) {
    const QSplitPlan qp = bwd_qsplit_plan(p);
    if (qp.nchunks) return backward_split_q(stream, p, qp, Q, K, V, O, l, m, dO, dQ, dK, dV, workspace, workspace_bytes);
    return fa_backward(stream, p, Q, K, V, O, l, m, dO, dQ, dK, dV, workspace, workspace_bytes);
  }
  const WsLayout w = ws_layout(p);
  if (!workspace || workspace_bytes < w.total + bwd_split_part_bytes(p, sp))
    return set_error(FA_ERR_WORKSPACE_TOO_SMALL,
                     "backward workspace is smaller than fa_backward_split_workspace_bytes()");
  FA_DIAG_COUNT(1);
  if (p->b == 0) return FA_OK;
  fa::BwdSplitArgs sa;
  fa::BwdArgs whole;
  fill_bwd(p, w, Q, K, V, O, l, m, dO, dQ, dK, dV, workspace, &whole);
  sa.b = whole;  // (the batch limit below reads the problem)
  sa.nchunks = sp.nchunks; sa.chunk = sp.chunk; sa.k_first = sp.k_first; sa.k_end = sp.ke;
  float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return bwd_slabs(p, whole, FA_SLAB_LIMIT(fa::bwd_f16_split_max_batch(sa)), &sa.b, [&](int64_t b0) {
    sa.ws_part = part + b0 * sp.nchunks * p->d * whole.rule.q.n;
    return fa::launch_bwd_f16_split(sa, s);
  });
}

int fa_merge_partials(void* stream, int32_t dtype, int64_t b, int64_t nq, int32_t v_d, int32_t n_parts,
                      const void* const* O_parts, const void* const* l_parts, const void* const* m_parts, void* O,
                      void* l, void* m) {
  if (dtype < FA_F16 || dtype > FA_F64) return set_error(FA_ERR_INVALID_ARGUMENT, "unknown dtype");
  if (n_parts < 1 || n_parts > FA_MAX_PARTS)
    return set_error(FA_ERR_INVALID_ARGUMENT, "n_parts must be in [1, " + std::to_string(FA_MAX_PARTS) + "]");
  if (b < 0) return set_error(FA_ERR_INVALID_ARGUMENT, "negative batch size");
  if (nq < 0) return set_error(FA_ERR_INVALID_ARGUMENT, "negative sequence extent");
  if (nq > 0x7fffffff)
    return set_error(FA_ERR_INVALID_ARGUMENT, "sequence sizes are limited to the int32 range (sync_methods.h:12-14)");
  if (v_d < 1) return set_error(FA_ERR_INVALID_ARGUMENT, "channel dimensions must be >= 1");
  if (b == 0 || nq == 0) return FA_OK;
  if (!O_parts || !l_parts || !m_parts) return set_error(FA_ERR_INVALID_ARGUMENT, "null array of part pointers");
  if (!O || !l || !m) return set_error(FA_ERR_INVALID_ARGUMENT, "null output pointer");
  fa::MergeArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_parts; ++i) {
    if (!O_parts[i] || !l_parts[i] || !m_parts[i])
      return set_error(FA_ERR_INVALID_ARGUMENT, "null pointer in part " + std::to_string(i));
    for (const void* in : {O_parts[i], l_parts[i], m_parts[i]})
      if (in == O || in == l || in == m)
        return set_error(FA_ERR_INVALID_ARGUMENT, "an output aliases an input of part " + std::to_string(i));
    a.O_parts[i] = O_parts[i]; a.l_parts[i] = l_parts[i]; a.m_parts[i] = m_parts[i];
  }
  const int64_t bmax = FA_SLAB_LIMIT(fa::merge_max_batch(dtype, nq, v_d));
  if (bmax < 1) return set_error(FA_ERR_UNSUPPORTED, "one slice exceeds the merge kernel's grid");
  const size_t es = elem_size(dtype), ls = dtype == FA_F16 ? sizeof(float) : es;
  a.nq = nq; a.v_d = v_d;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // slabs of at most bmax slices: the grid's y extent
  for (int64_t b0 = 0; b0 < b; b0 += bmax) {
    a.b = b - b0 < bmax ? b - b0 : bmax;
    const size_t o_off = es * (size_t)b0 * (size_t)v_d * (size_t)nq, l_off = ls * (size_t)b0 * (size_t)nq,
                 m_off = es * (size_t)b0 * (size_t)nq;
    for (int i = 0; i < n_parts; ++i) {
      a.O_parts[i] = static_cast<const char*>(O_parts[i]) + o_off;
      a.l_parts[i] = static_cast<const char*>(l_parts[i]) + l_off;
      a.m_parts[i] = static_cast<const char*>(m_parts[i]) + m_off;
    }
    a.O = static_cast<char*>(O) + o_off;
    a.l = static_cast<char*>(l) + l_off;
    a.m = static_cast<char*>(m) + m_off;
    FA_DIAG_SLAB();
    const hipError_t e = fa::launch_merge(dtype, n_parts, a, s);
    if (e != hipSuccess)
      return set_error((int)e, std::string("Failed to launch the merge kernel: ") + hipGetErrorString(e));
  }
  return FA_OK;
}

int fa_accumulate_parts(void* stream, int32_t dtype, int64_t count, int32_t n_parts, const void* const* parts,
                        void* out) {
  if (dtype < FA_F16 || dtype > FA_F64) return set_error(FA_ERR_INVALID_ARGUMENT, "unknown dtype");
  if (n_parts < 1 || n_parts > FA_MAX_PARTS)
    return set_error(FA_ERR_INVALID_ARGUMENT, "n_parts must be in [1, " + std::to_string(FA_MAX_PARTS) + "]");
  if (count < 0) return set_error(FA_ERR_INVALID_ARGUMENT, "negative element count");
  if (count == 0) return FA_OK;
  if (!parts) return set_error(FA_ERR_INVALID_ARGUMENT, "null array of part pointers");
  if (!out) return set_error(FA_ERR_INVALID_ARGUMENT, "null output pointer");
  for (int i = 0; i < n_parts; ++i) {
    if (!parts[i]) return set_error(FA_ERR_INVALID_ARGUMENT, "null pointer in part " + std::to_string(i));
    if (parts[i] == out)
      return set_error(FA_ERR_INVALID_ARGUMENT, "the output aliases the input of part " + std::to_string(i));
  }
  fa::AccumulateArgs a;
  memset(&a, 0, sizeof(a));
  const size_t es = elem_size(dtype);
  const int64_t cmax = FA_SLAB_LIMIT(fa::accumulate_max_count(), kAccumulateSlabUnit);
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int64_t c0 = 0; c0 < count; c0 += cmax) {
    a.count = count - c0 < cmax ? count - c0 : cmax;
    for (int i = 0; i < n_parts; ++i) a.parts[i] = static_cast<const char*>(parts[i]) + es * (size_t)c0;
    a.out = static_cast<char*>(out) + es * (size_t)c0;
    FA_DIAG_SLAB();
    const hipError_t e = fa::launch_accumulate(dtype, n_parts, a, s);
    if (e != hipSuccess)
      return set_error((int)e, std::string("Failed to launch the accumulate kernel: ") + hipGetErrorString(e));
  }
  return FA_OK;
}

int64_t fa_allowed_pairs(const fa_problem* p) {
  if (fa_validate(p) != FA_OK) return -1;
  fa::Rule r;
  build_rule(p, &r);
  const int64_t nq = r.q.n, nk = r.k.n;
  if (r.policy == FA_FULL) return nq * nk;
  int64_t total = 0;
  for (int32_t q = 0; q < nq; ++q) {
    int32_t kb, ke;
    fa::k_range_for_q_block(r, q, q, &kb, &ke);
    if (r.policy == FA_CAUSAL) {  // the causal range is exact
      total += ke - kb;
      continue;
    }
    const int32_t qo = fa::seq_order(r.q, r, q);
    for (int32_t k = kb; k < ke; ++k) total += fa::check_orders(r, qo, fa::seq_order(r.k, r, k)) ? 1 : 0;
  }
  return total;
}

int fa_rule_mask(const fa_problem* p, uint8_t* mask) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  if (!mask) return set_error(FA_ERR_INVALID_ARGUMENT, "null mask buffer");
  fa::Rule r;
  build_rule(p, &r);
  for (int32_t q = 0; q < r.q.n; ++q) {
    const int32_t qo = fa::seq_order(r.q, r, q);
    for (int32_t k = 0; k < r.k.n; ++k)
      mask[(int64_t)q * r.k.n + k] = fa::check_orders(r, qo, fa::seq_order(r.k, r, k)) ? 1 : 0;
  }
  return FA_OK;
}

int fa_rule_probe(const fa_problem* p, int32_t q0, int32_t q1, int32_t k0, int32_t k1, int32_t* out) {
  int st = fa_validate(p);
  if (st != FA_OK) return st;
  fa::Rule r;
  build_rule(p, &r);
  if (!out || q0 < 0 || q1 < q0 || q1 >= r.q.n || k0 < 0 || k1 < k0 || k1 >= r.k.n)
    return set_error(FA_ERR_INVALID_ARGUMENT, "probe block out of range");
  fa::k_range_for_q_block(r, q0, q1, &out[0], &out[1]);
  fa::q_range_for_k_block(r, k0, k1, &out[2], &out[3]);
  out[4] = fa::tile_class(r, q0, q1, k0, k1);
  return FA_OK;
}

double fa_estimate_forward_flops(const fa_problem* p) {
  const int64_t pairs = fa_allowed_pairs(p);
  if (pairs < 0) return -1.0;
  return 2.0 * (double)(p->d + p->v_d) * (double)pairs * (double)p->b;
}

const char* fa_error_string(int status) {
  switch (status) {
    case FA_OK: return "success";
    case FA_ERR_INVALID_ARGUMENT: return "invalid argument";
    case FA_ERR_UNSUPPORTED: return "unsupported problem";
    case FA_ERR_WORKSPACE_TOO_SMALL: return "workspace too small";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown error";
  }
}

const char* fa_last_error(void) { return g_last_error.c_str(); }

#ifndef FA_SRC_HASH
#define FA_SRC_HASH "unknown"
#endif
#ifdef FA_DIAG
#define FA_LIB_KIND "diagnostic (FA_DIAG: environment-selected variants)"
#else
#define FA_LIB_KIND "product"
#endif

const char* fa_build_info(void) {
  return "tf_flash_attention_amd: src=" FA_SRC_HASH "; lib=" FA_LIB_KIND "; gfx950; fwd={mfma_f16 (+ split-key, grouped-query fold, ragged key lengths, paged K/V, fp8 e4m3 K/V cache, sliding-window decode, query-blocked prefill, tree-masked draft decode, sliding-window prefill), mfma_f32, mfma_f64, generic(f16,f32,f64)}; bwd={mfma_f16 (two-pass (+ split-key dQ, split-query dK/dV)), mfma_f32 (two-pass), mfma_f64 (two-pass, d<=256), generic(f16,f32,f64)}; merge={f16,f32,f64, 1..8 parts}; append={fused K/V append: ragged, paged x f16, fp8 e4m3}";
}

}  // extern "C"
