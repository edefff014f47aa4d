// The one-wave trigger clustering shared by search.hip (one trigger list per launch) and timeslide.hip (one wave per time
// slide).  Reference: MLGWSC-1/inference.py:140-166 (`get_clusters`) fed by :484-487: time-ordered triggers closer than
// `cluster_threshold` seconds to their predecessor join its cluster; a cluster is reported as the time and value of its
// FIRST maximum.  The wave walks the score array 64 windows at a time, the trigger mask of a step is a ballot, and the
// (rare) set bits are folded into a wave-uniform running cluster -- a sequential algorithm whose state is four scalars.
// Times are the reference's float64 stamps, compared in float64.
#pragma once
#include "common.h"

namespace gww {

__device__ __forceinline__ double readlane_f64(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffu), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// All 64 lanes of ONE wave call this with the same arguments.  out_t / out_v hold max_clusters entries; *out_count counts
// on past them.
__device__ __forceinline__ void cluster_wave(const double* __restrict__ times, const float* __restrict__ scores, long n,
                                             float trigger_threshold, double cluster_threshold, double* __restrict__ out_t,
                                             float* __restrict__ out_v, int* __restrict__ out_count, int max_clusters) {
  const int lane = threadIdx.x & 63;
  bool have = false;
  double last_t = 0.0, best_t = 0.0;
  float best_v = 0.f;
  int count = 0;
  auto emit = [&]() {
    if (lane == 0 && count < max_clusters) { out_t[count] = best_t; out_v[count] = best_v; }
    ++count;
  };
  for (long base = 0; base < n; base += 64) {
    const long i = base + lane;
    const float s = i < n ? scores[i] : -INFINITY;
    const double t = i < n ? times[i] : 0.0;
    unsigned long long mask = __builtin_amdgcn_ballot_w64(s > trigger_threshold);
    while (mask) {
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const double tl = readlane_f64(t, l);
      const float vl = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), l));
      if (have && (tl - last_t) > cluster_threshold) {
        emit();
        have = false;
      }
      if (!have) { best_t = tl; best_v = vl; have = true; }
      else if (vl > best_v) { best_t = tl; best_v = vl; }     // strictly greater: np.argmax keeps the first maximum
      last_t = tl;
    }
  }
  if (have) emit();
  if (lane == 0) *out_count = count;
}

}  // namespace gww
