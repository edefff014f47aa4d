// Ordered compaction into one or two lists for the evaluation kernels (score.hip, trigger_stats.hip): a count pass (one
// packed count pair per workgroup), a one-workgroup exclusive scan of the pairs, and a put pass that scans again behind
// the workgroup's offset and stores.  Both passes classify through the same P::side, so the offsets match the stores.
#pragma once
#include "device_sort.h"

namespace gww {

// ---- the packed count pair ----------------------------------------------------------------------------------------------
// two counts travel as one 64-bit word, (first << 32) | second, and add as words.  Each half stays at most 2^27 (the
// entry points' largest n), so no carry crosses bit 32.  Plain C++ outside hipcc, as ordered_u32 is.
GWW_KEY_FN unsigned long long pair_word(bool first, bool second) { return first ? 1ull << 32 : (second ? 1ull : 0ull); }
GWW_KEY_FN unsigned pair_first(unsigned long long w) { return (unsigned)(w >> 32); }
GWW_KEY_FN unsigned pair_second(unsigned long long w) { return (unsigned)(w & 0xFFFFFFFFull); }

}  // namespace gww

#ifdef __HIPCC__
namespace gww {

constexpr int COMPACT_THREADS = 1024;
constexpr int COMPACT_WAVES = COMPACT_THREADS / 64;

static __global__ __launch_bounds__(64) void k_zero_i32(int* __restrict__ v, int n) {
  if ((int)threadIdx.x < n) v[threadIdx.x] = 0;
}

// one workgroup: blk[b] becomes the pair of counts in front of block b; *first, *second (either may be NULL) = the totals
static __global__ __launch_bounds__(COMPACT_THREADS) void k_pair_offsets(unsigned long long* __restrict__ blk, int nb,
                                                                         int* __restrict__ first, int* __restrict__ second) {
  __shared__ unsigned long long part[COMPACT_WAVES];
  unsigned long long carry = 0ull;
  for (int b0 = 0; b0 < nb; b0 += COMPACT_THREADS) {   // nb is the workgroup's: every thread takes the same trips
    const int b = b0 + threadIdx.x;
    const unsigned long long v = b < nb ? blk[b] : 0ull;
    unsigned long long tot;
    const unsigned long long incl = block_scan<unsigned long long, COMPACT_WAVES>(v, part, &tot);
    if (b < nb) blk[b] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    if (first) first[0] = (int)pair_first(carry);
    if (second) second[0] = (int)pair_second(carry);
  }
}

// ---- the block-level step (a workgroup of COMPACT_THREADS; part: COMPACT_WAVES words of LDS) -----------------------------
// the workgroup's packed total of the threads' pairs (thread 0 writes it to blk[blockIdx.x])
__device__ __forceinline__ unsigned long long block_pair_total(unsigned long long mine, unsigned long long* part) {
  unsigned long long tot;
  block_scan<unsigned long long, COMPACT_WAVES>(mine, part, &tot);
  return tot;
}
// the packed pair of output positions of this thread's first survivors: what lies in front of the workgroup plus the
// pairs of the threads in front of it
__device__ __forceinline__ unsigned long long block_pair_before(unsigned long long blk_offset, unsigned long long mine,
                                                                unsigned long long* part) {
  unsigned long long tot;
  return blk_offset + block_scan<unsigned long long, COMPACT_WAVES>(mine, part, &tot) - mine;
}

// ---- the generic kernel pair --------------------------------------------------------------------------------------------
// For compactions whose passes do nothing but classify and store, one element per thread.  A compaction is a struct P
// passed by value (pointers and scalars) with
//   int count() const                            the number of elements (device_count where it lives on the device)
//   unsigned capacity() const                    entries of each output list: a position at or past it is counted, not stored
//   int side(long i) const                       0 dropped, 1 first list, 2 second list: THE predicate, for both passes
//   void put(long i, int side, unsigned pos) const   the store, pos < capacity()
// Thread t of block b owns element b * COMPACT_THREADS + t: the lists keep the input's order.
template <typename P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_count(P p, unsigned long long* __restrict__ blk) {
  __shared__ unsigned long long part[COMPACT_WAVES];
  const long i = (long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  const int s = i < p.count() ? p.side(i) : 0;
  const unsigned long long tot = block_pair_total(pair_word(s == 1, s == 2), part);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

template <typename P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_put(P p, const unsigned long long* __restrict__ blk) {
  __shared__ unsigned long long part[COMPACT_WAVES];
  const long i = (long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  const int s = i < p.count() ? p.side(i) : 0;
  const unsigned long long at = block_pair_before(blk[blockIdx.x], pair_word(s == 1, s == 2), part);
  if (!s) return;
  const unsigned pos = s == 1 ? pair_first(at) : pair_second(at);
  if (pos < p.capacity()) p.put(i, s, pos);
}

// count, offsets, put over nb workgroups; blk: nb words of workspace; *first, *second (either may be NULL) = the totals
template <typename P>
int compact_launch(const P& p, unsigned nb, unsigned long long* blk, int* first, int* second, hipStream_t s) {
  hipLaunchKernelGGL(k_compact_count<P>, dim3(nb), dim3(COMPACT_THREADS), 0, s, p, blk);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(COMPACT_THREADS), 0, s, blk, (int)nb, first, second);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_compact_put<P>, dim3(nb), dim3(COMPACT_THREADS), 0, s, p, (const unsigned long long*)blk);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww
#endif  // __HIPCC__
