// Device primitives shared by the evaluation kernels (roc.hip, coinc.hip, detect.hip, glitch_scan.hip, logmel.hip,
// logmel_any.hip, and through device_compact.h score.hip and trigger_stats.hip): the order-preserving integer image of a
// float, an inclusive block scan, and a stable LSD radix sort of (key, index) pairs.
#pragma once

// ---- order-preserving integer images --------------------------------------------------------------------------------------
// a < b as floats <=> ordered(a) < ordered(b) as unsigned integers, with -0.0 just below +0.0.  No NaN rule and no folding of
// the zeros: a caller that needs either writes it at the call site.  Plain C++ outside hipcc, so a host test can compile them.
#ifdef __HIPCC__
#include "common.h"
#define GWW_KEY_FN __host__ __device__ __forceinline__
#else
#define GWW_KEY_FN inline
#endif

namespace gww {

GWW_KEY_FN unsigned ordered_u32(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GWW_KEY_FN float from_ordered_u32(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
GWW_KEY_FN unsigned long long ordered_u64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

}  // namespace gww

#ifdef __HIPCC__
namespace gww {

// ---- block scan -------------------------------------------------------------------------------------------------------------
// inclusive scan of v over the workgroup's 64 * WAVES threads in thread order; part: WAVES values of LDS.  Returns the
// thread's inclusive prefix; *total = the sum over the workgroup.  Ends on a barrier: part may be reused at once.  The
// additions of one call always happen in the same order (the shuffle tree, then the waves in index order): fp64 sums keep
// their bits from call to call.
template <typename T, int WAVES>
__device__ __forceinline__ T block_scan(T v, T* part, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v = v + u;
  }
  if (lane == 63) part[wave] = v;
  __syncthreads();
  T before = T(0), all = T(0);
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T t = part[w];
    if (w < wave) before = before + t;
    all = all + t;
  }
  __syncthreads();
  *total = all;
  return before + v;
}

// ---- radix sort -------------------------------------------------------------------------------------------------------------
// Stable LSD radix sort of (key, index) pairs, 8-bit digits, K = unsigned or unsigned long long.  Per pass: radix_hist (one
// workgroup per chunk), radix_scan (one workgroup), radix_scatter (one workgroup per chunk).  The element count may live
// on the device (n_dev): the grid covers the capacity, the kernels read the count.
constexpr int RADIX_CHUNK = 4096;           // elements of one workgroup of the sort (16 sub-tiles of 256)

// the element count: the capacity, or the device's count clamped into 0..capacity
__device__ __forceinline__ int device_count(const int* __restrict__ n_dev, int cap) {
  if (!n_dev) return cap;
  const int n = n_dev[0];
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// hist[block][d] = the number of the block's keys with digit d (a block behind the count writes zeros)
template <typename K>
__global__ __launch_bounds__(256) void radix_hist(const K* __restrict__ key, const int* __restrict__ n_dev, int cap, int shift,
                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  const int n = device_count(n_dev, cap);
  h[threadIdx.x] = 0u;
  __syncthreads();
  const long lo = (long)blockIdx.x * RADIX_CHUNK;
  const long hi = lo + RADIX_CHUNK < n ? lo + RADIX_CHUNK : n;
  for (long i = lo + threadIdx.x; i < hi; i += 256) atomicAdd(&h[(unsigned)(key[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(size_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// one workgroup, thread d: hist[b][d] becomes the first output position of block b's keys with digit d (digit-major order)
static __global__ __launch_bounds__(256) void radix_scan(unsigned* __restrict__ hist, int blocks) {
  __shared__ unsigned tot[256];
  const int d = threadIdx.x;
  unsigned s = 0u;
  for (int b = 0; b < blocks; ++b) s += hist[(size_t)b * 256 + d];
  tot[d] = s;
  __syncthreads();
  unsigned off = 0u;
  for (int j = 0; j < d; ++j) off += tot[j];
  for (int b = 0; b < blocks; ++b) {
    const unsigned c = hist[(size_t)b * 256 + d];
    hist[(size_t)b * 256 + d] = off;
    off += c;
  }
}

// the block's keys in order, 256 at a time: a key goes behind every earlier key of the same digit (stable)
template <typename K>
__global__ __launch_bounds__(256) void radix_scatter(const K* __restrict__ key, const int* __restrict__ idx,
                                                     const int* __restrict__ n_dev, int cap, int shift,
                                                     const unsigned* __restrict__ hist, K* __restrict__ key_out,
                                                     int* __restrict__ idx_out) {
  __shared__ unsigned base[256];            // next output position of digit d
  __shared__ unsigned wcnt[4][256];         // per wave: the count, then the first position, of digit d in this sub-tile
  const int n = device_count(n_dev, cap);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  base[tid] = hist[(size_t)blockIdx.x * 256 + tid];
  const long lo = (long)blockIdx.x * RADIX_CHUNK;
  const long hi = lo + RADIX_CHUNK < n ? lo + RADIX_CHUNK : n;
  for (long t0 = lo; t0 < hi; t0 += 256) {   // lo, hi are the workgroup's: every thread takes the same trips
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    const long i = t0 + tid;
    const bool active = i < hi;
    K k = 0;
    int ix = 0;
    if (active) {
      k = key[i];
      ix = idx[i];
    }
    const unsigned d = (unsigned)(k >> shift) & 255u;
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long vote = __ballot(active && bit);
      peers &= bit ? vote : ~vote;
    }
    const unsigned before = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    if (active && before == 0u) wcnt[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    {
      unsigned off = base[tid];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const unsigned c = wcnt[w][tid];
        wcnt[w][tid] = off;
        off += c;
      }
      base[tid] = off;
    }
    __syncthreads();
    if (active) {
      const unsigned dst = wcnt[wave][d] + before;
      if (dst < (unsigned)n) {               // always true for a consistent histogram; never store outside the buffers
        key_out[dst] = k;
        idx_out[dst] = ix;
      }
    }
    __syncthreads();
  }
}

// workspace of one sort of up to n pairs
template <typename K>
struct RadixWs {
  K *key_a, *key_b;
  int *idx_a, *idx_b;
  unsigned* hist;           // [blocks][256]
  size_t bytes;
};
template <typename K>
RadixWs<K> radix_carve(void* ws, long n) {
  Arena a;
  char* base = reinterpret_cast<char*>(ws);
  const size_t nb = (size_t)cdiv(n, RADIX_CHUNK);
  RadixWs<K> w;
  w.key_a = reinterpret_cast<K*>(base + a.take((size_t)n * sizeof(K)));
  w.key_b = reinterpret_cast<K*>(base + a.take((size_t)n * sizeof(K)));
  w.idx_a = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.idx_b = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.hist = reinterpret_cast<unsigned*>(base + a.take(nb * 256 * 4));
  w.bytes = a.total();
  return w;
}

// sorts the pairs in key_a / idx_a (the first n_dev[0] of them; a null n_dev: cap) by sizeof(K) passes that ping-pong
// between the a and the b buffers; *key, *idx = where the sorted pairs ended up
template <typename K>
int radix_sort_pairs(const RadixWs<K>& w, const int* n_dev, long cap, hipStream_t s, const K** key, const int** idx) {
  const unsigned blocks = (unsigned)cdiv(cap, RADIX_CHUNK);
  K *ka = w.key_a, *kb = w.key_b;
  int *ia = w.idx_a, *ib = w.idx_b;
  for (int pass = 0; pass < (int)sizeof(K); ++pass) {
    hipLaunchKernelGGL(radix_hist<K>, dim3(blocks), dim3(256), 0, s, (const K*)ka, n_dev, (int)cap, 8 * pass, w.hist);
    GWW_LAUNCH_CHECK();
    hipLaunchKernelGGL(radix_scan, dim3(1), dim3(256), 0, s, w.hist, (int)blocks);
    GWW_LAUNCH_CHECK();
    hipLaunchKernelGGL(radix_scatter<K>, dim3(blocks), dim3(256), 0, s, (const K*)ka, (const int*)ia, n_dev, (int)cap, 8 * pass,
                       (const unsigned*)w.hist, kb, ib);
    GWW_LAUNCH_CHECK();
    K* tk = ka; ka = kb; kb = tk;
    int* ti = ia; ia = ib; ib = ti;
  }
  *key = ka;
  *idx = ia;
  return GWW_OK;
}

}  // namespace gww
#endif  // __HIPCC__
