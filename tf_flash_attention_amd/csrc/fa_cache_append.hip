// fa_cache_append.hip — the write side of the four K/V caches of fa_fwd_f16_decode.h: new tokens' keys and values
// stored in place, ragged or paged, fp16 or FP8 (gfx950).
//
// Sequence s holds L = clamp(k_lens[s], 0, nk) keys AFTER the append, the same array the attention call of the step
// takes.  Its last n = min(clamp(new_lens[s], 0, n_new), L) positions are new (new_lens null: min(n_new, L)), taken
// from the LAST n of the n_new slots of K_new / V_new: slot n_new - n + t goes to position L - n + t, that is slot
// j + n_new - L to position j.  The slots in front are padding and are never loaded.
//
// ONE kernel template over a write-side cache description, which is a place times an encoding:
//   place     where key position k of channel row r of head h of sequence s lies, in elements
//             (AtRagged: row (slice, r) of a [..][C][nk] tensor; AtPaged: the pool page that the table names)
//   encoding  the element size and the conversion of 8 fp16 values into 8 packed elements
//             (AsF16: a bit copy; AsFp8: e4m3fn(fp32(x) / scale[h]), round to nearest even, saturating)
// Work is cut by DESTINATION: a thread owns one (channel row, 8-key chunk) of the cache, chunk c of the
// (n_new + 14) / 8 that a run of n_new positions can touch counted from the chunk of position L - n.  A chunk lies
// inside one page (page % 64 == 0), so a thread loads one table entry.  Lanes run along the key axis first, then over
// the d rows of K and the v_d rows of V of one (sequence, head): a prefill chunk's loads and stores are contiguous
// across a wave; a single token's stores are a row apart, which is what a cache with the key axis innermost costs.
// The source run is misaligned against the destination by (n_new - L) mod 8 elements, so a thread gathers its up to
// 8 source halfs with element loads (a wave's loads sweep one contiguous span).  It stores one 16-byte (fp16) or
// 8-byte (FP8) vector where all 8 positions are new and the address is aligned (always, in a pool whose base is),
// and single elements otherwise: nothing outside [L - n, L) is written, not even with its old value.
#include <hip/hip_fp16.h>

#include "fa_kernels.h"

namespace fa {
namespace {

constexpr int kAppendThreads = 256;
constexpr int kAppendChunk = 8;  // keys per thread
constexpr float kFp8Max = 448.0f;

struct AtRagged {
  static __device__ __forceinline__ int64_t element(const AppendArgs& a, uint32_t, uint32_t, int64_t slice_row, int32_t, int,
                                                    int k) {
    return slice_row * a.nk + k;
  }
};

struct AtPaged {
  // (k < L <= max_pages * page keeps the entry inside the table row; the clamp keeps the page inside the pool)
  static __device__ __forceinline__ int64_t element(const AppendArgs& a, uint32_t s, uint32_t h, int64_t, int32_t C, int r,
                                                    int k) {
    const int pg = k / a.page;
    const int entry = min(max(a.block_table[(int64_t)s * a.max_pages + pg], 0), a.last_page);
    return (((int64_t)entry * a.kv_heads + h) * C + r) * a.page + (k - pg * a.page);
  }
};

struct AsF16 {
  using Elem = uint16_t;
  static constexpr int kWords = 4;
  static __device__ __forceinline__ float scale(const float*, uint32_t) { return 1.0f; }
  static __device__ __forceinline__ void pack(const uint16_t (&x)[kAppendChunk], float, uint32_t (&w)[kWords]) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = (uint32_t)x[2 * i] | ((uint32_t)x[2 * i + 1] << 16);
  }
};

struct AsFp8 {
  using Elem = uint8_t;
  static constexpr int kWords = 2;
  static __device__ __forceinline__ float scale(const float* sc, uint32_t h) { return sc ? sc[h] : 1.0f; }
  // the fp32 quotient, correctly rounded, clamped to the format's range (the conversion alone would turn what lies
  // beyond it into NaN), then the hardware's round-to-nearest-even e4m3fn conversion, two values an instruction
  static __device__ __forceinline__ float quotient(uint16_t bits, float sc) {
    const float q = __half2float(__ushort_as_half(bits)) / sc;
    return fminf(fmaxf(q, -kFp8Max), kFp8Max);
  }
  static __device__ __forceinline__ void pack(const uint16_t (&x)[kAppendChunk], float sc, uint32_t (&w)[kWords]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
      int v = __builtin_amdgcn_cvt_pk_fp8_f32(quotient(x[4 * i], sc), quotient(x[4 * i + 1], sc), 0, false);
      v = __builtin_amdgcn_cvt_pk_fp8_f32(quotient(x[4 * i + 2], sc), quotient(x[4 * i + 3], sc), v, true);
      w[i] = (uint32_t)v;
    }
#else
    (void)x; (void)sc; (void)w;
#endif
  }
};

template <class Place, class Encoding>
struct AppendCache {
  using At = Place;
  using As = Encoding;
};
using RaggedAppend = AppendCache<AtRagged, AsF16>;
using PagedAppend = AppendCache<AtPaged, AsF16>;
using RaggedAppend8 = AppendCache<AtRagged, AsFp8>;
using PagedAppend8 = AppendCache<AtPaged, AsFp8>;

template <int WORDS>
struct VecOf;
template <>
struct VecOf<4> { using type = uint4; };
template <>
struct VecOf<2> { using type = uint2; };

template <class Cache>
__global__ __launch_bounds__(kAppendThreads) void cache_append_kernel(AppendArgs a) {
  using As = typename Cache::As;
  using Elem = typename As::Elem;
  using Vec = typename VecOf<As::kWords>::type;
  constexpr int kBits = 8 * (int)sizeof(Elem);
  static_assert(sizeof(Vec) == kAppendChunk * sizeof(Elem), "a chunk is one vector");
  const uint32_t slice = blockIdx.x / (uint32_t)a.slice_blocks;  // (sequence, head)
  const uint32_t within = (blockIdx.x - slice * (uint32_t)a.slice_blocks) * kAppendThreads + threadIdx.x;
  const uint32_t rows = (uint32_t)a.d + (uint32_t)a.v_d;
  if (within >= rows * (uint32_t)a.chunks) return;
  const int row = (int)(within / (uint32_t)a.chunks), c = (int)(within - (uint32_t)row * (uint32_t)a.chunks);
  const uint32_t s = slice / (uint32_t)a.kv_heads, h = slice - s * (uint32_t)a.kv_heads;
  const int L = min(max(a.k_lens[s], 0), a.nk);
  const int n = min(a.new_lens ? min(max(a.new_lens[s], 0), a.n_new) : a.n_new, L);
  const int p0 = L - n;  // the first new position
  const int64_t k64 = ((int64_t)(p0 / kAppendChunk) + c) * kAppendChunk;
  if (k64 >= L) return;
  const int k = (int)k64;  // the chunk's first position; k + 8 <= nk + 7
  const bool is_v = row >= a.d;
  const int r = is_v ? row - a.d : row, C = is_v ? a.v_d : a.d;
  const int64_t slice_row = (int64_t)slice * C + r;
  // position j comes from slot j + n_new - L; (k - L) + n_new + e >= n_new - n >= 0 for every loaded e
  const uint16_t* src = static_cast<const uint16_t*>(is_v ? a.V_new : a.K_new) + slice_row * a.n_new + ((k - L) + a.n_new);
  const int e0 = max(p0 - k, 0), e1 = min(L - k, kAppendChunk);  // the chunk's new positions: k + [e0, e1)
  const bool whole = e0 == 0 && e1 == kAppendChunk;
  uint16_t x[kAppendChunk];
  if (whole) {  // (apart from the partial chunks' guarded loads: 8 loads in flight, not 8 round trips)
#pragma unroll
    for (int e = 0; e < kAppendChunk; ++e) x[e] = src[e];
  } else {
#pragma unroll
    for (int e = 0; e < kAppendChunk; ++e) x[e] = (e >= e0 && e < e1) ? src[e] : (uint16_t)0;
  }
  uint32_t w[As::kWords];
  As::pack(x, As::scale(is_v ? a.v_scale : a.k_scale, h), w);
  Elem* dst = static_cast<Elem*>(is_v ? a.V : a.K) + Cache::At::element(a, s, h, slice_row, C, r, k);
  if (whole && (reinterpret_cast<uintptr_t>(dst) & (sizeof(Vec) - 1)) == 0) {
    Vec v;
    if constexpr (As::kWords == 4) v = make_uint4(w[0], w[1], w[2], w[3]);
    else v = make_uint2(w[0], w[1]);
    *reinterpret_cast<Vec*>(dst) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < kAppendChunk; ++e)
    if (e >= e0 && e < e1) dst[e] = (Elem)(w[e * kBits / 32] >> (e * kBits % 32));
}

template <class Cache>
hipError_t launch(const AppendArgs& a, int64_t blocks, hipStream_t s) {
  hipLaunchKernelGGL(cache_append_kernel<Cache>, dim3((uint32_t)blocks), dim3(kAppendThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cache_append(bool paged, bool fp8, const AppendArgs& a, int64_t blocks, hipStream_t s) {
  if (paged) return fp8 ? launch<PagedAppend8>(a, blocks, s) : launch<PagedAppend>(a, blocks, s);
  return fp8 ? launch<RaggedAppend8>(a, blocks, s) : launch<RaggedAppend>(a, blocks, s);
}

}  // namespace fa
