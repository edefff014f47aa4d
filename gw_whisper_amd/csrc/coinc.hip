// Coincidences of two detectors' event lists at zero lag and under S time slides.  Every detector's
// events are final before any pairing happens, so a slide is a shift o of detector 1's event times: events i (detector 0)
// and j (detector 1) are coincident iff fabs(d) <= window with d = (t1[j] + o) - t0[i], one fp64 addition and then one
// fp64 subtraction, in this order everywhere.  t1[j] + o is non-decreasing in j and fp64 subtraction is monotone, so
// `d >= -window` is a monotone predicate of j: the first candidate is found by bisection on the predicate itself and the
// result equals a double loop over all (i, j) bit for bit.  Partner rule: of the coincident j the largest v1[j], then the
// smallest fabs(d), then the smallest j; a detector-1 event is not consumed by being chosen.
//   k_coinc_count    grid (ceil(cap0 / 256), S), one thread per detector-0 event of one slide: bisection, the walk over
//                    the candidates, partner[s][i] (-1: none) and the workgroup's number of coincidences
//   k_coinc_offsets  one workgroup: the exclusive scan of those counts in (slide, workgroup) order, carried over chunks
//                    of 256 entries; offsets[s] = where slide s starts in the ragged result, offsets[S] = the total
//   k_coinc_emit     the same grid: a block scan behind the workgroup's offset puts the coincidences of a slide in
//                    ascending i; nothing is written at or beyond cap_total
// Comparing, counting and three fp64 operations: no atomics, no cross-workgroup flags, nothing here synchronises, identical
// calls give identical bits.  The counts may live on the device (device_sort.h: device_count): the grids cover the
// capacity, the kernels read the clamped count.
#include "device_sort.h"

namespace gww {

constexpr int CO_THREADS = 256;
constexpr int CO_WAVES = CO_THREADS / 64;
constexpr long CO_NMAX = 1L << 27;

__device__ __forceinline__ double coinc_dt(double t1j, double o, double t0i) {
  const double shifted = t1j + o;
  return shifted - t0i;
}

__global__ __launch_bounds__(CO_THREADS) void k_coinc_count(const double* __restrict__ t0, const int* __restrict__ n0_dev, int cap0,
                                                            const double* __restrict__ t1, const float* __restrict__ v1,
                                                            const int* __restrict__ n1_dev, int cap1,
                                                            const double* __restrict__ shifts, double window,
                                                            int* __restrict__ partner, long long* __restrict__ blk) {
  __shared__ int part[CO_WAVES];
  const int n0 = device_count(n0_dev, cap0), n1 = device_count(n1_dev, cap1);
  const int i = blockIdx.x * CO_THREADS + threadIdx.x;
  const int s = blockIdx.y;
  int best = -1;
  if (i < n0) {
    const double a = t0[i], o = shifts[s];
    int lo = 0, hi = n1;                       // the first j with d(i, j) >= -window
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (coinc_dt(t1[mid], o, a) >= -window) hi = mid; else lo = mid + 1;
    }
    float bv = 0.f;
    double bd = 0.0;
    for (int j = lo; j < n1; ++j) {
      const double ad = fabs(coinc_dt(t1[j], o, a));
      if (!(ad <= window)) break;              // d only grows from here on
      const float v = v1[j];
      if (best < 0 || v > bv || (v == bv && ad < bd)) {
        best = j;
        bv = v;
        bd = ad;
      }
    }
  }
  if (i < cap0) partner[(size_t)s * cap0 + i] = best;
  int total;
  block_scan<int, CO_WAVES>(best >= 0 ? 1 : 0, part, &total);
  if (threadIdx.x == 0) blk[(size_t)s * gridDim.x + blockIdx.x] = total;
}

// one workgroup: blk[e] becomes the number of coincidences in front of entry e = s * nb + b; offsets[s] = blk[s * nb]
__global__ __launch_bounds__(CO_THREADS) void k_coinc_offsets(long long* __restrict__ blk, int nb, int S,
                                                              long long* __restrict__ offsets) {
  __shared__ long long part[CO_WAVES];
  const long n = (long)S * nb;
  long long carry = 0;
  for (long e0 = 0; e0 < n; e0 += CO_THREADS) {       // n is the launch's: every thread takes the same trips
    const long e = e0 + threadIdx.x;
    const long long v = e < n ? blk[e] : 0;
    long long total;
    const long long incl = block_scan<long long, CO_WAVES>(v, part, &total);
    if (e < n) {
      const long long excl = carry + incl - v;
      blk[e] = excl;
      if (e % nb == 0) offsets[e / nb] = excl;
    }
    carry += total;
  }
  if (threadIdx.x == 0) offsets[S] = carry;
}

__global__ __launch_bounds__(CO_THREADS) void k_coinc_emit(const double* __restrict__ t0, const float* __restrict__ v0,
                                                           const int* __restrict__ n0_dev, int cap0,
                                                           const double* __restrict__ t1, const float* __restrict__ v1,
                                                           const int* __restrict__ n1_dev, int cap1,
                                                           const double* __restrict__ shifts, const int* __restrict__ partner,
                                                           const long long* __restrict__ blk, long long cap_total,
                                                           double* __restrict__ time, double* __restrict__ stat,
                                                           double* __restrict__ dt, int* __restrict__ idx0, int* __restrict__ idx1) {
  __shared__ int part[CO_WAVES];
  const int n0 = device_count(n0_dev, cap0), n1 = device_count(n1_dev, cap1);
  const int i = blockIdx.x * CO_THREADS + threadIdx.x;
  const int s = blockIdx.y;
  int j = i < n0 ? partner[(size_t)s * cap0 + i] : -1;
  if (j >= n1) j = -1;                         // a table this launch's count kernel wrote never holds one; no read outside t1
  int total;
  const int incl = block_scan<int, CO_WAVES>(j >= 0 ? 1 : 0, part, &total);
  if (j < 0) return;
  const long long pos = blk[(size_t)s * gridDim.x + blockIdx.x] + (long long)(incl - 1);
  if (pos < 0 || pos >= cap_total) return;
  const double a = t0[i];
  time[pos] = a;                               // detector 0 is never moved
  stat[pos] = (double)v0[i] + (double)v1[j];   // two fp32 values: exact in fp64
  dt[pos] = coinc_dt(t1[j], shifts[s], a);
  idx0[pos] = i;
  idx1[pos] = j;
}

static int coinc_blocks(long cap0) { return (int)(cap0 > 0 ? cdiv(cap0, CO_THREADS) : 1); }

}  // namespace gww

using namespace gww;

#define COINC_COUNTS(who)                                                                                              \
  GWW_REQUIRE(cap0 >= 0 && cap0 <= CO_NMAX, who ": n0=%ld must be 0..2^27", cap0);                                       \
  GWW_REQUIRE(cap1 >= 0 && cap1 <= CO_NMAX, who ": n1=%ld must be 0..2^27", cap1);                                       \
  GWW_REQUIRE(S >= 1 && S <= 65535, who ": S=%d slides, must be 1..65535", S)

extern "C" size_t gww_coinc_blocks(long n0) {
  if (n0 < 0 || n0 > CO_NMAX) return 0;
  return (size_t)coinc_blocks(n0);
}

extern "C" int gww_coinc_count_f64(const double* t0, const int* n0_dev, long cap0, const double* t1, const float* v1,
                                   const int* n1_dev, long cap1, const double* shifts, int S, double window, int* partner,
                                   long long* blocks, void* stream) {
  COINC_COUNTS("gww_coinc_count_f64");
  GWW_REQUIRE(shifts && blocks && (cap0 == 0 || (t0 && partner)) && (cap1 == 0 || (t1 && v1)),
              "gww_coinc_count_f64: NULL argument");
  GWW_REQUIRE(window >= 0.0, "gww_coinc_count_f64: window=%g must not be negative", window);
  GWW_REQUIRE(aligned(t0, 8) && aligned(t1, 8) && aligned(shifts, 8) && aligned(blocks, 8) && aligned(v1, 4) &&
              aligned(partner, 4) && aligned(n0_dev, 4) && aligned(n1_dev, 4),
              "gww_coinc_count_f64: operands must be aligned to their element size");
  const dim3 grid((unsigned)coinc_blocks(cap0), (unsigned)S);
  hipLaunchKernelGGL(k_coinc_count, grid, dim3(CO_THREADS), 0, (hipStream_t)stream, t0, n0_dev, (int)cap0, t1, v1, n1_dev,
                     (int)cap1, shifts, window, partner, blocks);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_coinc_offsets(long long* blocks, long cap0, int S, long long* offsets, void* stream) {
  GWW_REQUIRE(blocks && offsets, "gww_coinc_offsets: NULL argument");
  GWW_REQUIRE(cap0 >= 0 && cap0 <= CO_NMAX, "gww_coinc_offsets: n0=%ld must be 0..2^27", cap0);
  GWW_REQUIRE(S >= 1 && S <= 65535, "gww_coinc_offsets: S=%d slides, must be 1..65535", S);
  GWW_REQUIRE(aligned(blocks, 8) && aligned(offsets, 8), "gww_coinc_offsets: operands must be 8-byte aligned");
  hipLaunchKernelGGL(k_coinc_offsets, dim3(1), dim3(CO_THREADS), 0, (hipStream_t)stream, blocks, coinc_blocks(cap0), S, offsets);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_coinc_emit_f64(const double* t0, const float* v0, const int* n0_dev, long cap0, const double* t1,
                                  const float* v1, const int* n1_dev, long cap1, const double* shifts, int S,
                                  const int* partner, const long long* blocks, long cap_total, double* time, double* stat,
                                  double* dt, int* idx0, int* idx1, void* stream) {
  COINC_COUNTS("gww_coinc_emit_f64");
  GWW_REQUIRE(cap_total >= 0, "gww_coinc_emit_f64: cap_total=%ld is negative", cap_total);
  GWW_REQUIRE(shifts && blocks && (cap0 == 0 || (t0 && v0 && partner)) && (cap1 == 0 || (t1 && v1)) &&
              (cap_total == 0 || (time && stat && dt && idx0 && idx1)), "gww_coinc_emit_f64: NULL argument");
  GWW_REQUIRE(aligned(t0, 8) && aligned(t1, 8) && aligned(shifts, 8) && aligned(blocks, 8) && aligned(time, 8) &&
              aligned(stat, 8) && aligned(dt, 8) && aligned(v0, 4) && aligned(v1, 4) && aligned(partner, 4) &&
              aligned(idx0, 4) && aligned(idx1, 4) && aligned(n0_dev, 4) && aligned(n1_dev, 4),
              "gww_coinc_emit_f64: operands must be aligned to their element size");
  if (cap0 == 0 || cap1 == 0 || cap_total == 0) return GWW_OK;          // nothing can be written
  const dim3 grid((unsigned)coinc_blocks(cap0), (unsigned)S);
  hipLaunchKernelGGL(k_coinc_emit, grid, dim3(CO_THREADS), 0, (hipStream_t)stream, t0, v0, n0_dev, (int)cap0, t1, v1, n1_dev,
                     (int)cap1, shifts, partner, blocks, (long long)cap_total, time, stat, dt, idx0, idx1);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
