// fa_merge.hip — merge of attention partials over several key sets, and the part-order sum (gfx950).
//
// merge_kernel<T, N>: N partial results (O_i, l_i, m_i) of one Q against N key sets, in the forwards'
// own output format, become the forward's output for the concatenated keys (include/fa_api.h, "Merging
// partial results").  accumulate_kernel<T, N>: out = T(sum_i in_i), summed in part order in the
// accumulator type; dQ of a combined attention is that sum of the parts' dQ.
//
// Both are memory-bound, so they are shaped for the vector memory path: a thread owns 16 bytes of
// consecutive queries (8 halfs, 4 floats, 2 doubles); the merge computes the N weights of each of its
// queries once, in registers, and sweeps kRows channel rows with one 16-byte load per part and one
// 16-byte store per row.  Rows are 16-byte aligned only when nq is a multiple of the vector width and
// every base pointer is aligned: that is the VEC instantiation; every other case takes the same code
// with guarded element loads and stores.  No atomics, no cross-thread traffic: the result is
// deterministic, and an element's bits depend on its own inputs only (not on b or on the grid).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "fa_kernels.h"

namespace fa {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 8;  // channel rows a merge thread sweeps with one set of weights

// element types on the device: T, its accumulator A and the type L of l (fp32 for fp16 inputs)
template <typename T> struct Types { using A = float; using L = float; };
template <> struct Types<double> { using A = double; using L = double; };

// NegInfApprox: every byte 0xFA, the m of a row that attends nothing
template <typename T> __device__ __forceinline__ T neg_inf_approx_bits() {
  T v;
  memset(&v, 0xFA, sizeof(T));
  return v;
}

__device__ __forceinline__ float exp_acc(float x) { return expf(x); }
__device__ __forceinline__ double exp_acc(double x) { return exp(x); }

// V consecutive elements from p[i0 ...]: 16-byte loads (VEC: p + i0 is 16-byte aligned and all V are
// in range), else element loads guarded by i0 + j < n, `fill` past the end.
template <bool VEC, typename E, int V>
__device__ __forceinline__ void load_run(const E* __restrict__ p, int64_t i0, int64_t n, E fill, E (&out)[V]) {
  if constexpr (VEC) {
    constexpr int kBytes = V * (int)sizeof(E);
    static_assert(kBytes % 16 == 0, "a run is whole 16-byte vectors");
    uint4 raw[kBytes / 16];
#pragma unroll
    for (int k = 0; k < kBytes / 16; ++k) raw[k] = reinterpret_cast<const uint4*>(p + i0)[k];
    memcpy(out, raw, kBytes);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = i0 + j < n ? p[i0 + j] : fill;
  }
}

template <bool VEC, typename E, int V>
__device__ __forceinline__ void store_run(E* __restrict__ p, int64_t i0, int64_t n, const E (&in)[V]) {
  if constexpr (VEC) {
    constexpr int kBytes = V * (int)sizeof(E);
    uint4 raw[kBytes / 16];
    memcpy(raw, in, kBytes);
#pragma unroll
    for (int k = 0; k < kBytes / 16; ++k) reinterpret_cast<uint4*>(p + i0)[k] = raw[k];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < n) p[i0 + j] = in[j];
  }
}

// One thread = (slice, chunk of kRows channel rows, run of V queries), runs fastest.  The threads of
// chunk 0 also write l and m.  a.b is not read: the grid's y extent is the slice count.
template <typename T, int N, bool VEC>
__global__ __launch_bounds__(kThreads) void merge_kernel(MergeArgs a) {
  using A = typename Types<T>::A;
  using L = typename Types<T>::L;
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t nq = a.nq;
  const int vd = a.v_d;
  // grid: x over the (chunk, run) pairs of one slice (fewer than 2^31: 32-bit index arithmetic), y = slice
  const uint32_t runs = (uint32_t)((nq + V - 1) / V);
  const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= runs * (uint32_t)((vd + kRows - 1) / kRows)) return;
  const int64_t bi = blockIdx.y;
  const int chunk = (int)(idx / runs);
  const int64_t q0 = (int64_t)(idx - (uint32_t)chunk * runs) * V;

  // ---- the weights of this thread's V queries: w[i][j] = e_i / L, e_i = l_i * exp(m_i - m)
  A w[N][V];
  bool live[N][V];  // part i is not empty for query j
  L l_out[V];
  T m_out[V];
  {
    L li[N][V];
    T mi[N][V];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      load_run<VEC>(static_cast<const L*>(a.l_parts[i]) + bi * nq, q0, nq, (L)0, li[i]);
      load_run<VEC>(static_cast<const T*>(a.m_parts[i]) + bi * nq, q0, nq, (T)0, mi[i]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      // (an empty part's m never enters the arithmetic, so no infinity or NaN arises anywhere)
      bool any = false;
      A mx = (A)0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        live[i][j] = li[i][j] != (L)0;
        const A mv = (A)mi[i][j];
        if (live[i][j]) mx = any ? (mv > mx ? mv : mx) : mv;
        any = any || live[i][j];
      }
      A sum = (A)0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const A dm = live[i][j] ? (A)mi[i][j] - mx : (A)0;  // <= 0
        w[i][j] = (A)li[i][j] * exp_acc(dm);                // 0 for an empty part
        sum += w[i][j];
      }
      // any: the part that holds the max has e = l > 0, so sum > 0
      const A den = any ? sum : (A)1;
#pragma unroll
      for (int i = 0; i < N; ++i) w[i][j] = w[i][j] / den;  // IEEE division: correctly rounded
      l_out[j] = any ? (L)sum : (L)0;
      m_out[j] = any ? (T)mx : neg_inf_approx_bits<T>();  // mx is one of the parts' m: exact in T
    }
  }
  if (chunk == 0) {
    store_run<VEC>(static_cast<L*>(a.l) + bi * nq, q0, nq, l_out);
    store_run<VEC>(static_cast<T*>(a.m) + bi * nq, q0, nq, m_out);
  }

  // ---- O rows [v0, v1) of the run.  The sum starts from -0 and an empty part adds -0, which leave every
  // other term's bits alone (x + -0 == x, also for x == -0): one part comes back bit for bit, and an empty
  // part changes nothing; a row empty everywhere gets +0.
  // Rows go in groups of G with all of a group's loads issued before its first use: about 8 loads of 16 bytes
  // in flight per thread whatever N is.
  constexpr int G = N >= 8 ? 1 : 8 / N;
  const int v0 = chunk * kRows, v1 = v0 + kRows < vd ? v0 + kRows : vd;
  const int64_t slice = bi * (int64_t)vd * nq;
  for (int vg = v0; vg < v1; vg += G) {
    T oi[G][N][V];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      // (past the chunk's last row the load repeats that row, unconditionally: no branch between the loads)
      const int vr = vg + g < v1 ? vg + g : v1 - 1;
#pragma unroll
      for (int i = 0; i < N; ++i)
        load_run<VEC>(static_cast<const T*>(a.O_parts[i]) + slice + (int64_t)vr * nq, q0, nq, (T)0, oi[g][i]);
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (vg + g < v1) {
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          A acc = -(A)0;
          bool any = false;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            acc += live[i][j] ? w[i][j] * (A)oi[g][i][j] : -(A)0;
            any = any || live[i][j];
          }
          // fp16: keep the product and its rounding to T apart.  Fused, a lone product becomes a mixed-precision
          // fma with a +0 addend, which turns a -0 result into +0 (the one-part case would not come back bitwise)
          if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(acc));
          o[j] = any ? (T)acc : (T)0;
        }
        store_run<VEC>(static_cast<T*>(a.O) + slice + (int64_t)(vg + g) * nq, q0, nq, o);
      }
  }
}

// One thread = a run of V elements.  The last run of an unaligned count, and every run of unaligned
// pointers, goes element by element.
template <typename T, int N, bool VEC>
__global__ __launch_bounds__(kThreads) void accumulate_kernel(AccumulateArgs a) {
  using A = typename Types<T>::A;
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V;
  if (i0 >= a.count) return;
  const bool whole = i0 + V <= a.count;
  A acc[V];
  T in[V];
  auto add = [&](int i, auto vec) {
    load_run<decltype(vec)::value>(static_cast<const T*>(a.parts[i]), i0, a.count, (T)0, in);
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = i == 0 ? (A)in[j] : acc[j] + (A)in[j];
  };
  T out[V];
  if (VEC && whole) {
#pragma unroll
    for (int i = 0; i < N; ++i) add(i, std::true_type{});
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = (T)acc[j];
    store_run<true>(static_cast<T*>(a.out), i0, a.count, out);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) add(i, std::false_type{});
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = (T)acc[j];
    store_run<false>(static_cast<T*>(a.out), i0, a.count, out);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

size_t elem_bytes(int dtype) { return dtype == 0 ? 2 : (dtype == 1 ? 4 : 8); }

int64_t merge_items_per_slice(int dtype, int64_t nq, int32_t v_d) {
  const int64_t V = 16 / (int64_t)elem_bytes(dtype);
  return ((nq + V - 1) / V) * ((v_d + kRows - 1) / kRows);
}

template <typename T, int N>
hipError_t launch_merge_tn(const MergeArgs& a, bool vec, hipStream_t s) {
  const int64_t per = merge_items_per_slice(sizeof(T) == 2 ? 0 : (sizeof(T) == 4 ? 1 : 2), a.nq, a.v_d);
  const dim3 grid((unsigned)((per + kThreads - 1) / kThreads), (unsigned)a.b);
  if (vec)
    hipLaunchKernelGGL((merge_kernel<T, N, true>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((merge_kernel<T, N, false>), grid, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

template <typename T, int N>
hipError_t launch_accumulate_tn(const AccumulateArgs& a, bool vec, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t threads = (a.count + V - 1) / V;
  const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads));
  if (vec)
    hipLaunchKernelGGL((accumulate_kernel<T, N, true>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((accumulate_kernel<T, N, false>), grid, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// calls f(integral_constant<int, n>) for the runtime n in 1..kMaxParts
template <typename F>
hipError_t with_parts(int n, F&& f) {
  switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

int64_t merge_max_batch(int dtype, int64_t nq, int32_t v_d) {
  // the grid's y extent holds the slices; a slice's (chunk, run) pairs are indexed in 32 bits
  return merge_items_per_slice(dtype, nq, v_d) < (int64_t(1) << 31) ? 65535 : 0;
}

hipError_t launch_merge(int dtype, int n_parts, const MergeArgs& a, hipStream_t s) {
  const int64_t V = 16 / (int64_t)elem_bytes(dtype);
  bool vec = a.nq % V == 0 && aligned16(a.O) && aligned16(a.l) && aligned16(a.m);
  for (int i = 0; i < n_parts; ++i)
    vec = vec && aligned16(a.O_parts[i]) && aligned16(a.l_parts[i]) && aligned16(a.m_parts[i]);
  return with_parts(n_parts, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return dtype == 0   ? launch_merge_tn<_Float16, N>(a, vec, s)
           : dtype == 1 ? launch_merge_tn<float, N>(a, vec, s)
                        : launch_merge_tn<double, N>(a, vec, s);
  });
}

int64_t accumulate_max_count() { return ((int64_t(1) << 31) - 1) / 8 * 8 * kThreads; }

hipError_t launch_accumulate(int dtype, int n_parts, const AccumulateArgs& a, hipStream_t s) {
  bool vec = aligned16(a.out);
  for (int i = 0; i < n_parts; ++i) vec = vec && aligned16(a.parts[i]);
  return with_parts(n_parts, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return dtype == 0   ? launch_accumulate_tn<_Float16, N>(a, vec, s)
           : dtype == 1 ? launch_accumulate_tn<float, N>(a, vec, s)
                        : launch_accumulate_tn<double, N>(a, vec, s);
  });
}

}  // namespace fa
