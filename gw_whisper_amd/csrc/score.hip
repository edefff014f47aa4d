// Scoring a search on the device (MLGWSC-1/evaluate.py: get_stats): clustered events against the injections -> true and
// false positives, the found and missed injections, the false-alarm rates and the sensitive volume at every background
// statistic.  Everything here is sorting, searching and integer counting plus a few fp64 operations in the reference's
// order, so identical calls give identical bits and the results equal numpy's operation for operation; the only sums of
// many fp64 terms, the chirp-mass-weighted suffix sums, are taken in one fixed order.  No float
// atomics, no cross-workgroup flags, nothing here synchronises.
//   k_sc_keys / k_sc_finish   key = the order-preserving 64-bit image of the double, ascending; between the two the shared
//                    stable radix sort of (key, index) pairs, eight 8-bit digits (device_sort.h: radix_hist / radix_scan /
//                    radix_scatter on 64-bit keys).  The element count may live on the device (n_dev): the grid covers
//                    the capacity, the kernels read the count
//   k_sc_closest     find_closest_index for plain values
//   k_sc_match       per time-sorted event: the gathered event, the closest injection, |dt|, the per-block (TP, FP) counts:
//                    the count pass of the events' ordered compaction (device_compact.h: k_pair_offsets scans the counts)
//   k_sc_compact_ev  its put pass: a block scan behind the block's offset
//   k_sc_best        one wave per injection: its run of events by two binary searches, the best true-positive statistic
//   ScInjections     ordered compaction of the found and the missed injections (compact_launch)
// An event is a true positive iff sc_true_positive(|dt|, var): the one place that rule is written.
//   k_sc_far         (n - k - 1) / duration
//   k_sc_suffix      one workgroup: suffix sums of the found injections' chirp-mass weights in found-statistic order
//   k_sc_volume      per background statistic: nfound by a binary search, the fraction, the volume and its error
// This file is compiled with -ffp-contract=off (Makefile): a fused multiply-add in p - p * p would lose the bit match
// with numpy.
#include "common.h"
#include "device_compact.h"

namespace gww {

constexpr long SC_NMAX = 1L << 27;
constexpr int SC_THREADS = COMPACT_THREADS;
constexpr int SC_WAVES = SC_THREADS / 64;

// ascending key = ascending value; -0.0 and +0.0 are one value; every NaN gets the last key (counted by the caller)
__device__ __forceinline__ unsigned long long sc_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.0) v = 0.0;
  return ordered_u64(v);
}

__global__ __launch_bounds__(256) void k_sc_keys(const double* __restrict__ keys, const int* __restrict__ n_dev, int cap,
                                                 unsigned long long* __restrict__ key, int* __restrict__ idx,
                                                 int* __restrict__ n_nan) {
  const int n = device_count(n_dev, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = keys[i];
  key[i] = sc_key(v);
  idx[i] = i;
  if (v != v) atomicAdd(n_nan, 1);            // an integer count: the order of the adds does not matter
}

__global__ __launch_bounds__(256) void k_sc_finish(const int* __restrict__ idx, const double* __restrict__ keys,
                                                   const int* __restrict__ n_dev, int cap, int* __restrict__ order,
                                                   double* __restrict__ sorted) {
  const int n = device_count(n_dev, cap);
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int i = idx[p];
  if ((unsigned)i >= (unsigned)n) i = 0;     // a permutation by construction
  order[p] = i;
  sorted[p] = keys[i];
}

// ---- closest injection --------------------------------------------------------------------------------------------------
// find_closest_index (evaluate.py:91-97) for one value: r = searchsorted(tc, t, 'right'), l = max(r - 1, 0); l wins when
// r == N or |tc[l] - t| < |tc[min(r, N - 1)] - t| (strict: an exact midpoint goes right)
__device__ __forceinline__ int sc_closest(const double* __restrict__ tc, int N, double t, double* diff) {
  int lo = 0, hi = N;                         // the first j with tc[j] > t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tc[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const int r = lo, l = r > 0 ? r - 1 : 0, rc = r < N ? r : N - 1;
  const double dl = fabs(tc[l] - t), dr = fabs(tc[rc] - t);
  const bool left = r == N || dl < dr;
  *diff = left ? dl : dr;
  return left ? l : r;
}

__global__ __launch_bounds__(256) void k_sc_closest(const double* __restrict__ tc, int N, const double* __restrict__ t, int n,
                                                    int* __restrict__ idx, double* __restrict__ diff) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  double d;
  idx[p] = sc_closest(tc, N, t[p], &d);
  diff[p] = d;
}

// ---- events -----------------------------------------------------------------------------------------------------------
// a true positive lies within its own var of the closest injection; equality counts (evaluate.py:161)
__device__ __forceinline__ bool sc_true_positive(double diff, double var) { return diff <= var; }

__global__ __launch_bounds__(SC_THREADS) void k_sc_match(const double* __restrict__ time, const double* __restrict__ stat,
                                                         const double* __restrict__ var, const int* __restrict__ order, int E,
                                                         const double* __restrict__ tc, int N, double* __restrict__ fgs,
                                                         int* __restrict__ found_idx, double* __restrict__ diff,
                                                         unsigned long long* __restrict__ blk, int* __restrict__ n_nan) {
  __shared__ unsigned long long part[SC_WAVES];
  const long p = (long)blockIdx.x * SC_THREADS + threadIdx.x;
  bool tp = false;
  if (p < E) {
    int i = order[p];
    if ((unsigned)i >= (unsigned)E) i = 0;   // a permutation by construction
    const double t = time[i], s = stat[i], v = var[i];
    fgs[p] = t;
    fgs[(size_t)E + p] = s;
    fgs[2 * (size_t)E + p] = v;
    double d;
    found_idx[p] = sc_closest(tc, N, t, &d);
    diff[p] = d;
    tp = sc_true_positive(d, v);
    if (t != t || s != s || v != v) atomicAdd(n_nan, 1);
  }
  const unsigned long long tot = block_pair_total(pair_word(p < E && tp, p < E), part);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// the put pass behind k_sc_match: the true positives (first list) and the false positives of the time-sorted events
__global__ __launch_bounds__(SC_THREADS) void k_sc_compact_ev(const double* __restrict__ fgs, const double* __restrict__ diff,
                                                              int E, const unsigned long long* __restrict__ blk,
                                                              int* __restrict__ tp_idx, int* __restrict__ fp_idx,
                                                              double* __restrict__ tp_diff, double* __restrict__ fp_diff,
                                                              double* __restrict__ tp_ev, double* __restrict__ fp_ev) {
  __shared__ unsigned long long part[SC_WAVES];
  const long p = (long)blockIdx.x * SC_THREADS + threadIdx.x;
  const bool active = p < E;
  double t = 0.0, s = 0.0, v = 0.0, d = 0.0;
  if (active) {
    t = fgs[p];
    s = fgs[(size_t)E + p];
    v = fgs[2 * (size_t)E + p];
    d = diff[p];
  }
  const bool tp = active && sc_true_positive(d, v);
  const unsigned long long excl = block_pair_before(blk[blockIdx.x], pair_word(tp, active), part);
  if (!active) return;
  const unsigned j = tp ? pair_first(excl) : pair_second(excl);
  if (j >= (unsigned)E) return;              // always false for consistent counts; never store outside the buffers
  double* oe = tp ? tp_ev : fp_ev;
  (tp ? tp_idx : fp_idx)[j] = (int)p;
  (tp ? tp_diff : fp_diff)[j] = d;
  oe[j] = t;
  oe[(size_t)E + j] = s;
  oe[2 * (size_t)E + j] = v;
}

// ---- injections ---------------------------------------------------------------------------------------------------------
// One wave per injection i.  The events are time-sorted and tc ascends, so found_idx is non-decreasing: the events of i
// are the run [L, R) two binary searches find (evaluate.py:205-208).  flag: 1 = found (the run holds a true positive; best =
// the largest statistic among them), 2 = missed (an empty run: the reference's setdiff1d), 0 = a run of false positives only.
__global__ __launch_bounds__(SC_THREADS) void k_sc_best(const int* __restrict__ found_idx, const double* __restrict__ fgs,
                                                        const double* __restrict__ diff, int E, int N, double* __restrict__ best,
                                                        unsigned char* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;                         // the whole wave; no barrier in this kernel
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (found_idx[mid] < (int)i) lo = mid + 1; else hi = mid;
  }
  const int L = lo;
  hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (found_idx[mid] <= (int)i) lo = mid + 1; else hi = mid;
  }
  const int R = lo;
  double m = 0.0;
  int has = 0;
  for (int p = L + lane; p < R; p += 64) {
    if (sc_true_positive(diff[p], fgs[2 * (size_t)E + p])) {
      const double s = fgs[(size_t)E + p];
      if (!has || s > m) m = s;
      has = 1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(m, o, 64);
    const int oh = __shfl_xor(has, o, 64);
    if (oh && (!has || om > m)) m = om;
    has |= oh;
  }
  if (lane == 0) {
    best[i] = m;
    flag[i] = L == R ? 2 : (has ? 1 : 0);
  }
}

// the found injections with their best statistic (first list) and the missed ones
struct ScInjections {
  const unsigned char* flag;
  const double* best;
  int N;
  int* found_inj;
  double* found_stat;
  int* missed;
  __device__ int count() const { return N; }
  __device__ unsigned capacity() const { return (unsigned)N; }
  __device__ int side(long i) const {
    const int f = flag[i];
    return f == 1 || f == 2 ? f : 0;
  }
  __device__ void put(long i, int side, unsigned j) const {
    (side == 1 ? found_inj : missed)[j] = (int)i;
    if (side == 1) found_stat[j] = best[i];
  }
};

// ---- rates and volumes ----------------------------------------------------------------------------------------------------
// far[k] = (n - k - 1) / duration over n ascending noise statistics (evaluate.py:185-186): an exact integer, one division
__global__ __launch_bounds__(256) void k_sc_far(const int* __restrict__ n_dev, int cap, double duration, double* __restrict__ far) {
  const int n = device_count(n_dev, cap);
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  far[k] = (double)((long)n - k - 1) / duration;
}

// one workgroup walks the found injections from the largest best statistic down, SC_THREADS at a time: cs1[p] = the sum of
// w1 over the sorted positions p .. F - 1 (cs2: of w2), cs[F] = 0 (evaluate.py:256-262)
__global__ __launch_bounds__(SC_THREADS) void k_sc_suffix(const double* __restrict__ w1, const double* __restrict__ w2, int N,
                                                          const int* __restrict__ found_inj, const int* __restrict__ order,
                                                          const int* __restrict__ F_dev, double* __restrict__ cs1,
                                                          double* __restrict__ cs2) {
  __shared__ double part[SC_WAVES];
  const int F = device_count(F_dev, N);
  double c1 = 0.0, c2 = 0.0;
  if (threadIdx.x == 0) {
    cs1[F] = 0.0;
    cs2[F] = 0.0;
  }
  for (int r0 = 0; r0 < F; r0 += SC_THREADS) {   // F is the workgroup's: every thread takes the same trips
    const int p = F - 1 - (r0 + (int)threadIdx.x);
    double a = 0.0, b = 0.0;
    if (p >= 0) {
      int o = order[p];
      if ((unsigned)o >= (unsigned)F) o = 0;
      int i = found_inj[o];
      if ((unsigned)i >= (unsigned)N) i = 0;
      a = w1[i];
      b = w2[i];
    }
    double t1, t2;
    const double s1 = block_scan<double, SC_WAVES>(a, part, &t1);
    const double s2 = block_scan<double, SC_WAVES>(b, part, &t2);
    if (p >= 0) {
      cs1[p] = c1 + s1;
      cs2[p] = c2 + s2;
    }
    c1 = c1 + t1;
    c2 = c2 + t2;
  }
}

// thread k: fidx = searchsorted(found, noise[k], 'right'), nfound = F - fidx, then evaluate.py:263-276 in its order
__global__ __launch_bounds__(256) void k_sc_volume(const double* __restrict__ found, const int* __restrict__ F_dev, int cap,
                                                   const double* __restrict__ noise, int B, double Ninj, double prefactor,
                                                   const double* __restrict__ cs1, const double* __restrict__ cs2,
                                                   long long* __restrict__ nfound, double* __restrict__ frac,
                                                   double* __restrict__ vol, double* __restrict__ vol_err) {
  const int F = device_count(F_dev, cap);
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= B) return;
  const double x = noise[k];
  int lo = 0, hi = F;                         // the first j with found[j] > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (found[mid] <= x) lo = mid + 1; else hi = mid;
  }
  const long long nf = (long long)F - lo;
  const double f = (double)nf / Ninj;
  double mc, sv;
  if (cs1) {
    mc = cs1[lo];
    const double a = cs2[lo] / Ninj, q = mc / Ninj;
    const double qq = q * q;
    sv = a - qq;
  } else {
    mc = (double)nf;
    const double ff = f * f;
    sv = f - ff;
  }
  nfound[k] = nf;
  frac[k] = f;
  vol[k] = prefactor * mc;
  vol_err[k] = prefactor * __dsqrt_rn(Ninj * sv);
}

struct ScMatchWs {
  double* diff;             // [E]
  double* best;             // [N]
  unsigned long long *blk_e, *blk_n;
  unsigned char* flag;      // [N]
  size_t bytes;
};
static ScMatchWs sc_match_carve(void* ws, long E, long N) {
  Arena a;
  char* base = reinterpret_cast<char*>(ws);
  ScMatchWs w;
  w.diff = reinterpret_cast<double*>(base + a.take((size_t)E * 8));
  w.best = reinterpret_cast<double*>(base + a.take((size_t)N * 8));
  w.blk_e = reinterpret_cast<unsigned long long*>(base + a.take((size_t)cdiv(E, SC_THREADS) * 8));
  w.blk_n = reinterpret_cast<unsigned long long*>(base + a.take((size_t)cdiv(N, SC_THREADS) * 8));
  w.flag = reinterpret_cast<unsigned char*>(base + a.take((size_t)N));
  w.bytes = a.total();
  return w;
}

}  // namespace gww

using namespace gww;

extern "C" size_t gww_score_sort_workspace_bytes(long n) {
  if (n < 1 || n > SC_NMAX) return 0;
  return radix_carve<unsigned long long>(nullptr, n).bytes;
}

extern "C" int gww_score_sort_f64(const double* keys, long n, const int* n_dev, double* sorted, int* order, int* n_nan, void* ws,
                                  size_t ws_bytes, void* stream) {
  GWW_REQUIRE(keys && sorted && order && n_nan && ws, "gww_score_sort_f64: NULL argument");
  GWW_REQUIRE(n >= 1 && n <= SC_NMAX, "gww_score_sort_f64: n=%ld must be 1..2^27", n);
  GWW_REQUIRE(ws_bytes >= gww_score_sort_workspace_bytes(n), "gww_score_sort_f64: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_score_sort_workspace_bytes(n));
  GWW_REQUIRE(aligned(ws, 16), "gww_score_sort_f64: workspace must be 16-byte aligned");
  const RadixWs<unsigned long long> w = radix_carve<unsigned long long>(ws, n);
  hipStream_t s = (hipStream_t)stream;
  const int cap = (int)n;
  const unsigned b256 = (unsigned)cdiv(n, 256);
  hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, n_nan, 1);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sc_keys, dim3(b256), dim3(256), 0, s, keys, n_dev, cap, w.key_a, w.idx_a, n_nan);
  GWW_LAUNCH_CHECK();
  const unsigned long long* key;
  const int* idx;
  GWW_TRY(radix_sort_pairs(w, n_dev, n, s, &key, &idx));
  hipLaunchKernelGGL(k_sc_finish, dim3(b256), dim3(256), 0, s, idx, keys, n_dev, cap, order, sorted);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_score_closest_f64(const double* tc, long N, const double* t, long n, int* idx, double* diff, void* stream) {
  GWW_REQUIRE(tc && t && idx && diff, "gww_score_closest_f64: NULL argument");
  GWW_REQUIRE(N >= 1 && N <= SC_NMAX, "gww_score_closest_f64: N=%ld must be 1..2^27", N);
  GWW_REQUIRE(n >= 1 && n <= SC_NMAX, "gww_score_closest_f64: n=%ld must be 1..2^27", n);
  hipLaunchKernelGGL(k_sc_closest, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, tc, (int)N, t, (int)n, idx,
                     diff);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_score_match_workspace_bytes(long E, long N) {
  if (E < 1 || E > SC_NMAX || N < 1 || N > SC_NMAX) return 0;
  return sc_match_carve(nullptr, E, N).bytes;
}

extern "C" int gww_score_match_f64(const double* events, const int* order, long E, const double* tc, long N, double* fg_sorted,
                                   int* found_idx, int* tp_idx, int* fp_idx, double* tp_diff, double* fp_diff, double* tp_events,
                                   double* fp_events, int* found_inj, double* found_stat, int* missed, int* counts, void* ws,
                                   size_t ws_bytes, void* stream) {
  GWW_REQUIRE(events && order && tc && fg_sorted && found_idx && tp_idx && fp_idx && tp_diff && fp_diff && tp_events &&
              fp_events && found_inj && found_stat && missed && counts && ws, "gww_score_match_f64: NULL argument");
  GWW_REQUIRE(E >= 1 && E <= SC_NMAX, "gww_score_match_f64: E=%ld must be 1..2^27", E);
  GWW_REQUIRE(N >= 1 && N <= SC_NMAX, "gww_score_match_f64: N=%ld must be 1..2^27", N);
  GWW_REQUIRE(ws_bytes >= gww_score_match_workspace_bytes(E, N), "gww_score_match_f64: workspace of %zu bytes, %zu needed",
              ws_bytes, gww_score_match_workspace_bytes(E, N));
  GWW_REQUIRE(aligned(ws, 16), "gww_score_match_f64: workspace must be 16-byte aligned");
  const ScMatchWs w = sc_match_carve(ws, E, N);
  hipStream_t s = (hipStream_t)stream;
  const int e = (int)E, n = (int)N;
  const unsigned be = (unsigned)cdiv(E, SC_THREADS), bn = (unsigned)cdiv(N, SC_THREADS);
  hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, counts, 5);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sc_match, dim3(be), dim3(SC_THREADS), 0, s, events, events + E, events + 2 * E, order, e, tc, n, fg_sorted,
                     found_idx, w.diff, w.blk_e, counts + 4);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(SC_THREADS), 0, s, w.blk_e, (int)be, counts, counts + 1);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sc_compact_ev, dim3(be), dim3(SC_THREADS), 0, s, (const double*)fg_sorted, (const double*)w.diff, e,
                     (const unsigned long long*)w.blk_e, tp_idx, fp_idx, tp_diff, fp_diff, tp_events, fp_events);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sc_best, dim3((unsigned)cdiv(N, SC_WAVES)), dim3(SC_THREADS), 0, s, (const int*)found_idx,
                     (const double*)fg_sorted, (const double*)w.diff, e, n, w.best, w.flag);
  GWW_LAUNCH_CHECK();
  return compact_launch(ScInjections{w.flag, w.best, n, found_inj, found_stat, missed}, bn, w.blk_n, counts + 2, counts + 3, s);
}

extern "C" int gww_score_far_f64(const int* n_dev, long n, double duration, double* far, void* stream) {
  GWW_REQUIRE(far, "gww_score_far_f64: NULL argument");
  GWW_REQUIRE(n >= 1 && n <= SC_NMAX, "gww_score_far_f64: n=%ld must be 1..2^27", n);
  hipLaunchKernelGGL(k_sc_far, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, n_dev, (int)n, duration, far);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_score_suffix_f64(const double* w1, const double* w2, long N, const int* found_inj, const int* order,
                                    const int* F, double* cs1, double* cs2, void* stream) {
  GWW_REQUIRE(w1 && w2 && found_inj && order && F && cs1 && cs2, "gww_score_suffix_f64: NULL argument");
  GWW_REQUIRE(N >= 1 && N <= SC_NMAX, "gww_score_suffix_f64: N=%ld must be 1..2^27", N);
  hipLaunchKernelGGL(k_sc_suffix, dim3(1), dim3(SC_THREADS), 0, (hipStream_t)stream, w1, w2, (int)N, found_inj, order, F, cs1, cs2);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_score_volume_f64(const double* found_sorted, const int* F, long N, const double* noise_sorted, long B,
                                    double Ninj, double prefactor, const double* cs1, const double* cs2, long long* nfound,
                                    double* fraction, double* volume, double* volume_err, void* stream) {
  GWW_REQUIRE(found_sorted && F && noise_sorted && nfound && fraction && volume && volume_err,
              "gww_score_volume_f64: NULL argument");
  GWW_REQUIRE((cs1 == nullptr) == (cs2 == nullptr), "gww_score_volume_f64: cs1 and cs2 come together");
  GWW_REQUIRE(N >= 1 && N <= SC_NMAX, "gww_score_volume_f64: N=%ld must be 1..2^27", N);
  GWW_REQUIRE(B >= 1 && B <= SC_NMAX, "gww_score_volume_f64: B=%ld must be 1..2^27", B);
  hipLaunchKernelGGL(k_sc_volume, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, found_sorted, F, (int)N,
                     noise_sorted, (int)B, Ninj, prefactor, cs1, cs2, nfound, fraction, volume, volume_err);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
