// The test stage of the efficiency study on the device (Signal_vs_Noise/Efficiency_test/src/evaluate_test_data.py): a long
// series of ranking statistics -> triggers -> clustered events -> true and false positives -> the ranking steps with their
// false-alarm rate and sensitive volume.  Everything here is comparing, counting, searching and a few fp64 operations in
// the reference's order: identical calls give identical bits, no result depends on the launch geometry, and every output
// equals numpy's operation for operation.  No atomics on data (two integer NaN counters only), no
// cross-workgroup flags, nothing here synchronises.  Every count lives on the device (device_sort.h: device_count): the
// grids cover the capacity, the kernels read the clamped count.
// The three ordered compactions share device_compact.h: per-block count pairs, k_pair_offsets (a one-workgroup exclusive
// scan of them), a block scan behind the block's offset; each predicate is one function, used by both passes.
//   k_ts_trig_count / k_ts_trig_compact   (time, value) of the samples above the threshold (ts_is_trigger).  TS_ITEMS
//                    consecutive samples per thread.  time = double(i) * delta_t + epoch, rounded twice
//   k_ts_ev_partial / k_ts_ev_carry / k_ts_ev_emit   clusters and events: trigger j opens a cluster iff j == 0 or
//                    t[j] - t[j-1] >= tolerance; a segmented inclusive scan with the (value, first index) maximum as
//                    operator -- in the block, then over the blocks' aggregates by one workgroup, then again in the block
//                    behind the carry -- leaves at the last trigger of every cluster np.argmax of its run; the cluster's
//                    number is the scan of the opening flags
//   k_ts_split_count / k_ts_split_compact   true positive iff the distance to the nearest injection <= tolerance
//                    (ts_true_positive): the two groups' values
//   TsStepStarts / k_ts_step_stats   one ranking step per run of equal ascending false-positive values: the starts are
//                    compacted by the generic kernel pair (compact_launch), then one thread per step
// This file is compiled with -ffp-contract=off (Makefile): a fused multiply-add in double(i) * delta_t + epoch or in
// q - q * q would lose the bit match with numpy, and the first decides on which side of the cluster tolerance a gap falls.
#include "common.h"
#include "device_compact.h"

namespace gww {

constexpr long TS_NMAX = 1L << 27;
constexpr int TS_THREADS = COMPACT_THREADS;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_ITEMS = 4;                       // consecutive samples of one thread of the trigger kernels
constexpr int TS_CARRY = 256;                     // threads of the one-workgroup carry scan of the event kernels
constexpr int TS_TILE = TS_THREADS * TS_ITEMS;    // samples of one workgroup of the trigger kernels
constexpr double TS_SEC_PER_MONTH = 2592000.0;    // 30 * 24 * 60 * 60 (evaluate_test_data.py:18)

// ---- triggers -----------------------------------------------------------------------------------------------------------
// get_triggers (bnslib.py:216-240): the samples with series[i] > threshold, compared in fp64 (an fp32 sample widens
// exactly); equality is no trigger and a NaN never is (counted: the caller refuses the series)
__device__ __forceinline__ bool ts_is_trigger(double v, double thr) { return v > thr; }

template <typename T>
__global__ __launch_bounds__(TS_THREADS) void k_ts_trig_count(const T* __restrict__ series, int n, double thr,
                                                              unsigned long long* __restrict__ blk, int* __restrict__ n_nan) {
  __shared__ unsigned long long part[TS_WAVES];
  const long i0 = (long)blockIdx.x * TS_TILE + (long)threadIdx.x * TS_ITEMS;
  unsigned long long c = 0ull;
  int bad = 0;
#pragma unroll
  for (int k = 0; k < TS_ITEMS; ++k) {
    if (i0 + k < n) {
      const double v = (double)series[i0 + k];
      c += ts_is_trigger(v, thr) ? 1ull : 0ull;
      bad += v != v ? 1 : 0;
    }
  }
  if (bad) atomicAdd(n_nan, bad);               // an integer count: the order of the adds does not matter
  const unsigned long long tot = block_pair_total(c << 32, part);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

template <typename T>
__global__ __launch_bounds__(TS_THREADS) void k_ts_trig_compact(const T* __restrict__ series, int n, double thr, double delta_t,
                                                                double epoch, const unsigned long long* __restrict__ blk, int cap,
                                                                double* __restrict__ times, double* __restrict__ values) {
  __shared__ unsigned long long part[TS_WAVES];
  const long i0 = (long)blockIdx.x * TS_TILE + (long)threadIdx.x * TS_ITEMS;
  double v[TS_ITEMS];
  unsigned long long c = 0ull;
#pragma unroll
  for (int k = 0; k < TS_ITEMS; ++k) {
    v[k] = i0 + k < n ? (double)series[i0 + k] : 0.0;
    c += (i0 + k < n && ts_is_trigger(v[k], thr)) ? 1ull : 0ull;
  }
  unsigned j = pair_first(block_pair_before(blk[blockIdx.x], c << 32, part));
#pragma unroll
  for (int k = 0; k < TS_ITEMS; ++k) {
    if (i0 + k < n && ts_is_trigger(v[k], thr)) {
      if (j < (unsigned)cap) {                    // more triggers than the capacity: counted, not stored (the caller refuses)
        const double prod = (double)(i0 + k) * delta_t;   // sample_times = arange(n) * delta_t + epoch: two roundings
        times[j] = prod + epoch;
        values[j] = v[k];
      }
      ++j;
    }
  }
}

// ---- clusters and events --------------------------------------------------------------------------------------------------
// the running maximum of a cluster: v = the largest value since the cluster opened, i = the FIRST trigger that has it
// (np.argmax), f = a cluster opens inside the range this covers; i < 0: an empty range
struct TsSeg {
  double v;
  int i, f;
};
__device__ __forceinline__ TsSeg ts_seg_none() { return TsSeg{0.0, -1, 0}; }
// a: the earlier triggers, b: the later ones (by value, member by member: the triple stays in registers)
__device__ __forceinline__ TsSeg ts_seg_join(TsSeg a, TsSeg b) {
  const bool later = b.f || a.i < 0 || (b.i >= 0 && b.v > a.v);
  TsSeg r;
  r.v = later ? b.v : a.v;
  r.i = later ? b.i : a.i;
  r.f = a.f | b.f;
  return r;
}

// the LDS of one segmented block scan: one triple per wave
template <int WAVES>
struct TsSegPart {
  double v[WAVES];
  int i[WAVES], f[WAVES];
};

// inclusive segmented scan over the workgroup in thread order.  Ends on a barrier: part may be reused at once.
template <int WAVES>
__device__ __forceinline__ TsSeg ts_block_seg_scan(TsSeg s, TsSegPart<WAVES>& part, TsSeg* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    TsSeg u;
    u.v = __shfl_up(s.v, o, 64);
    u.i = __shfl_up(s.i, o, 64);
    u.f = __shfl_up(s.f, o, 64);
    if (lane >= o) s = ts_seg_join(u, s);
  }
  if (lane == 63) {
    part.v[wave] = s.v;
    part.i[wave] = s.i;
    part.f[wave] = s.f;
  }
  __syncthreads();
  TsSeg before = ts_seg_none(), all = ts_seg_none();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    TsSeg t;
    t.v = part.v[w];
    t.i = part.i[w];
    t.f = part.f[w];
    if (w < wave) before = ts_seg_join(before, t);
    all = ts_seg_join(all, t);
  }
  __syncthreads();
  *total = all;
  return ts_seg_join(before, s);
}

// trigger j of n opens a cluster (evaluate_test_data.py:261-319: the loop compares against the last trigger taken into the
// cluster, which is always the previous trigger)
__device__ __forceinline__ bool ts_opens(const double* __restrict__ t, int j, double tol) {
  return j == 0 || t[j] - t[j - 1] >= tol;
}

struct TsBlocks {
  unsigned long long* cnt;   // [nb] the block's number of opened clusters (high word), then the number in front of it
  double* v;                 // [nb] the block's aggregate, then the carry into it
  int *i, *f;
};

__global__ __launch_bounds__(TS_THREADS) void k_ts_ev_partial(const double* __restrict__ times, const double* __restrict__ values,
                                                              const int* __restrict__ n_dev, int cap, double tol, TsBlocks B,
                                                              int* __restrict__ n_nan) {
  __shared__ unsigned long long part[TS_WAVES];
  __shared__ TsSegPart<TS_WAVES> spart;
  const int n = device_count(n_dev, cap);
  const long j = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  TsSeg s = ts_seg_none();
  if (j < n) {
    s = TsSeg{values[j], (int)j, ts_opens(times, (int)j, tol) ? 1 : 0};
    if (s.v != s.v) atomicAdd(n_nan, 1);
  }
  unsigned long long tot;
  block_scan<unsigned long long, TS_WAVES>(pair_word(s.f != 0, false), part, &tot);
  TsSeg all;
  ts_block_seg_scan(s, spart, &all);
  if (threadIdx.x == 0) {
    B.cnt[blockIdx.x] = tot;
    B.v[blockIdx.x] = all.v;
    B.i[blockIdx.x] = all.i;
    B.f[blockIdx.x] = all.f;
  }
}

// one workgroup: the exclusive scans of the blocks' counts and aggregates, TS_CARRY blocks at a time behind a carry (256
// threads: the two scans and the carry fit the registers of a smaller workgroup; 1024 threads spilled)
__global__ __launch_bounds__(TS_CARRY) void k_ts_ev_carry(TsBlocks B, int nb, int* __restrict__ n_events) {
  __shared__ unsigned long long part[TS_CARRY / 64];
  __shared__ TsSegPart<TS_CARRY / 64> spart;
  __shared__ double sv[TS_CARRY];
  __shared__ int si[TS_CARRY], sf[TS_CARRY];
  unsigned long long carry = 0ull;
  TsSeg scarry = ts_seg_none();
  for (int b0 = 0; b0 < nb; b0 += TS_CARRY) {   // nb is the workgroup's: every thread takes the same trips
    const int b = b0 + threadIdx.x;
    const unsigned long long c = b < nb ? B.cnt[b] : 0ull;
    const TsSeg s = b < nb ? TsSeg{B.v[b], B.i[b], B.f[b]} : ts_seg_none();
    unsigned long long tot;
    const unsigned long long incl = block_scan<unsigned long long, TS_CARRY / 64>(c, part, &tot);
    TsSeg all;
    const TsSeg sincl = ts_block_seg_scan(s, spart, &all);
    sv[threadIdx.x] = sincl.v;
    si[threadIdx.x] = sincl.i;
    sf[threadIdx.x] = sincl.f;
    __syncthreads();
    if (b < nb) {
      // what enters block b: the carry joined with the blocks of this trip in front of it (the previous thread's
      // inclusive value; its f says whether a cluster opened among them).  The flag itself is not needed again.
      TsSeg in = scarry;
      if (threadIdx.x > 0) in = ts_seg_join(scarry, TsSeg{sv[threadIdx.x - 1], si[threadIdx.x - 1], sf[threadIdx.x - 1]});
      B.cnt[b] = carry + incl - c;
      B.v[b] = in.v;
      B.i[b] = in.i;
    }
    __syncthreads();
    carry += tot;
    scarry = ts_seg_join(scarry, all);
  }
  if (threadIdx.x == 0) n_events[0] = (int)pair_first(carry);
}

__global__ __launch_bounds__(TS_THREADS) void k_ts_ev_emit(const double* __restrict__ times, const double* __restrict__ values,
                                                           const int* __restrict__ n_dev, int cap, double tol, TsBlocks B,
                                                           double* __restrict__ ev_times, double* __restrict__ ev_values) {
  __shared__ unsigned long long part[TS_WAVES];
  __shared__ TsSegPart<TS_WAVES> spart;
  const int n = device_count(n_dev, cap);
  const long j = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  TsSeg s = ts_seg_none();
  if (j < n) s = TsSeg{values[j], (int)j, ts_opens(times, (int)j, tol) ? 1 : 0};
  unsigned long long tot;
  const unsigned long long incl = B.cnt[blockIdx.x] + block_scan<unsigned long long, TS_WAVES>(pair_word(s.f != 0, false), part, &tot);
  TsSeg all;
  const TsSeg in{B.v[blockIdx.x], B.i[blockIdx.x], 0};
  const TsSeg best = ts_seg_join(in, ts_block_seg_scan(s, spart, &all));
  if (j >= n) return;
  const bool last = j == n - 1 || times[j + 1] - times[j] >= tol;
  if (!last) return;
  const unsigned c = pair_first(incl) - 1u;   // the cluster's number: the clusters opened up to j, less one
  if (c >= (unsigned)cap || (unsigned)best.i >= (unsigned)n) return;   // never true; never store or load outside the buffers
  ev_times[c] = times[best.i];
  ev_values[c] = best.v;
}

// ---- true and false positives ---------------------------------------------------------------------------------------------
// split_true_and_false_positives (evaluate_test_data.py:28-87): diff = the distance to the nearest injection; a true positive
// iff diff <= tolerance (equality counts)
__device__ __forceinline__ bool ts_true_positive(double diff, double tol) { return diff <= tol; }

__global__ __launch_bounds__(TS_THREADS) void k_ts_split_count(const double* __restrict__ values, const double* __restrict__ diff,
                                                               const int* __restrict__ n_dev, int cap, double tol,
                                                               unsigned long long* __restrict__ blk, int* __restrict__ n_nan) {
  __shared__ unsigned long long part[TS_WAVES];
  const int n = device_count(n_dev, cap);
  const long j = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  bool tp = false;
  if (j < n) {
    tp = ts_true_positive(diff[j], tol);
    const double v = values[j];
    if (v != v) atomicAdd(n_nan, 1);
  }
  const unsigned long long tot = block_pair_total(pair_word(j < n && tp, j < n), part);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(TS_THREADS) void k_ts_split_compact(const double* __restrict__ values, const double* __restrict__ diff,
                                                                 const int* __restrict__ n_dev, int cap, double tol,
                                                                 const unsigned long long* __restrict__ blk,
                                                                 double* __restrict__ tp_values, double* __restrict__ fp_values) {
  __shared__ unsigned long long part[TS_WAVES];
  const int n = device_count(n_dev, cap);
  const long j = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  const bool active = j < n;
  const bool tp = active && ts_true_positive(diff[j], tol);
  const unsigned long long excl = block_pair_before(blk[blockIdx.x], pair_word(tp, active), part);
  if (!active) return;
  const unsigned p = tp ? pair_first(excl) : pair_second(excl);
  if (p >= (unsigned)cap) return;                 // always false for consistent counts; never store outside the buffers
  (tp ? tp_values : fp_values)[p] = values[j];
}

// ---- ranking steps --------------------------------------------------------------------------------------------------------
// evaluate_test_data.py:555-583 over the ascending false-positive values v[0 .. n): one step per run of equal values,
// starts[s] = the position where run s begins
struct TsStepStarts {
  const double* v;
  const int* n_dev;
  int cap;
  int* starts;
  __device__ int count() const { return device_count(n_dev, cap); }
  __device__ unsigned capacity() const { return (unsigned)cap; }
  __device__ int side(long a) const { return a == 0 || v[a] != v[a - 1] ? 1 : 0; }
  __device__ void put(long a, int, unsigned s) const { starts[s] = (int)a; }
};

struct TsStats {
  double *ranking, *far, *frac, *vol, *vol_err;
};

// thread s: the run [a, b] of step s.  ranking = v[a]; count = n - b - 1, except that a first run of length one counts n
// (the reference's first far entry is (n - 0) and only a later equal value overwrites it); far = count / duration *
// SEC_PER_MONTH in that order; tidx = searchsorted(tp, ranking, 'right'); then :589-612 in their order
__global__ __launch_bounds__(256) void k_ts_step_stats(const double* __restrict__ v, const int* __restrict__ n_fp_dev, int cap,
                                                       const int* __restrict__ starts, const int* __restrict__ n_steps_dev,
                                                       const double* __restrict__ tp, const int* __restrict__ n_tp_dev, int cap_tp,
                                                       double duration, double prefactor, double Ninj, TsStats O) {
  const int n = device_count(n_fp_dev, cap), S = device_count(n_steps_dev, cap), T = device_count(n_tp_dev, cap_tp);
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  int a = starts[s];
  int b = (s + 1 < S ? starts[s + 1] : n) - 1;
  if ((unsigned)a >= (unsigned)n) a = 0;          // positions of v by construction
  if (b < a || b >= n) b = a;
  const double x = v[a];
  const long count = (s == 0 && b == a) ? (long)n : (long)n - b - 1;
  const double per_s = (double)count / duration;
  int lo = 0, hi = T;                             // the first j with tp[j] > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tp[mid] <= x) lo = mid + 1; else hi = mid;
  }
  const double part = (double)lo / (double)T;
  const long sum = (long)T - lo;
  const double q = (double)sum / Ninj;
  const double qq = q * q;
  const double var = q - qq;
  O.ranking[s] = x;
  O.far[s] = per_s * TS_SEC_PER_MONTH;
  O.frac[s] = 1.0 - part;
  O.vol[s] = prefactor * (double)sum;
  O.vol_err[s] = prefactor * __dsqrt_rn(Ninj * var);
}

static size_t ts_blocks(long n, int per) { return (size_t)cdiv(n, per); }

struct TsEvWs {
  TsBlocks B;
  size_t bytes;
};
static TsEvWs ts_ev_carve(void* ws, long n) {
  Arena a;
  char* base = reinterpret_cast<char*>(ws);
  const size_t nb = ts_blocks(n, TS_THREADS);
  TsEvWs w;
  w.B.cnt = reinterpret_cast<unsigned long long*>(base + a.take(nb * 8));
  w.B.v = reinterpret_cast<double*>(base + a.take(nb * 8));
  w.B.i = reinterpret_cast<int*>(base + a.take(nb * 4));
  w.B.f = reinterpret_cast<int*>(base + a.take(nb * 4));
  w.bytes = a.total();
  return w;
}

struct TsStepWs {
  unsigned long long* blk;
  int* starts;
  size_t bytes;
};
static TsStepWs ts_step_carve(void* ws, long n) {
  Arena a;
  char* base = reinterpret_cast<char*>(ws);
  TsStepWs w;
  w.blk = reinterpret_cast<unsigned long long*>(base + a.take(ts_blocks(n, TS_THREADS) * 8));
  w.starts = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.bytes = a.total();
  return w;
}

template <typename T>
static int ts_triggers(const T* series, long n, long cap, double delta_t, double epoch, double threshold, double* times,
                       double* values, int* counts, unsigned long long* blk, hipStream_t s) {
  hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, counts, 2);
  GWW_LAUNCH_CHECK();
  const unsigned nb = (unsigned)ts_blocks(n, TS_TILE);
  hipLaunchKernelGGL(k_ts_trig_count<T>, dim3(nb), dim3(TS_THREADS), 0, s, series, (int)n, threshold, blk, counts + 1);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(TS_THREADS), 0, s, blk, (int)nb, counts, (int*)nullptr);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ts_trig_compact<T>, dim3(nb), dim3(TS_THREADS), 0, s, series, (int)n, threshold, delta_t, epoch,
                     (const unsigned long long*)blk, (int)cap, times, values);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" size_t gww_trig_triggers_workspace_bytes(long n) {
  if (n < 1 || n > TS_NMAX) return 0;
  Arena a;
  a.take(ts_blocks(n, TS_TILE) * 8);
  return a.total();
}

extern "C" int gww_trig_triggers_f64(const void* series, int is_f64, long n, long cap, double delta_t, double epoch,
                                     double threshold, double* times, double* values, int* counts, void* ws, size_t ws_bytes,
                                     void* stream) {
  GWW_REQUIRE(series && times && values && counts && ws, "gww_trig_triggers_f64: NULL argument");
  GWW_REQUIRE(n >= 1 && n <= TS_NMAX, "gww_trig_triggers_f64: n=%ld must be 1..2^27", n);
  GWW_REQUIRE(cap >= 1 && cap <= n, "gww_trig_triggers_f64: cap=%ld must be 1..n", cap);
  GWW_REQUIRE(is_f64 == 0 || is_f64 == 1, "gww_trig_triggers_f64: is_f64=%d must be 0 (fp32 series) or 1", is_f64);
  GWW_REQUIRE(ws_bytes >= gww_trig_triggers_workspace_bytes(n), "gww_trig_triggers_f64: workspace of %zu bytes, %zu needed",
              ws_bytes, gww_trig_triggers_workspace_bytes(n));
  GWW_REQUIRE(aligned(ws, 16), "gww_trig_triggers_f64: workspace must be 16-byte aligned");
  unsigned long long* blk = reinterpret_cast<unsigned long long*>(ws);
  if (is_f64)
    return ts_triggers(reinterpret_cast<const double*>(series), n, cap, delta_t, epoch, threshold, times, values, counts, blk,
                       (hipStream_t)stream);
  return ts_triggers(reinterpret_cast<const float*>(series), n, cap, delta_t, epoch, threshold, times, values, counts, blk,
                     (hipStream_t)stream);
}

extern "C" size_t gww_trig_events_workspace_bytes(long n) {
  if (n < 1 || n > TS_NMAX) return 0;
  return ts_ev_carve(nullptr, n).bytes;
}

extern "C" int gww_trig_events_f64(const double* times, const double* values, const int* n_dev, long cap, double tolerance,
                                   double* ev_times, double* ev_values, int* counts, void* ws, size_t ws_bytes, void* stream) {
  GWW_REQUIRE(times && values && ev_times && ev_values && counts && ws, "gww_trig_events_f64: NULL argument");
  GWW_REQUIRE(cap >= 1 && cap <= TS_NMAX, "gww_trig_events_f64: cap=%ld must be 1..2^27", cap);
  GWW_REQUIRE(ws_bytes >= gww_trig_events_workspace_bytes(cap), "gww_trig_events_f64: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_trig_events_workspace_bytes(cap));
  GWW_REQUIRE(aligned(ws, 16), "gww_trig_events_f64: workspace must be 16-byte aligned");
  const TsEvWs w = ts_ev_carve(ws, cap);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)ts_blocks(cap, TS_THREADS);
  hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, counts, 2);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ts_ev_partial, dim3(nb), dim3(TS_THREADS), 0, s, times, values, n_dev, (int)cap, tolerance, w.B, counts + 1);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ts_ev_carry, dim3(1), dim3(TS_CARRY), 0, s, w.B, (int)nb, counts);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ts_ev_emit, dim3(nb), dim3(TS_THREADS), 0, s, times, values, n_dev, (int)cap, tolerance, w.B, ev_times,
                     ev_values);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_trig_split_workspace_bytes(long n) {
  if (n < 1 || n > TS_NMAX) return 0;
  Arena a;
  a.take(ts_blocks(n, TS_THREADS) * 8);
  return a.total();
}

extern "C" int gww_trig_split_f64(const double* values, const double* diff, const int* n_dev, long cap, double tolerance,
                                  double* tp_values, double* fp_values, int* counts, void* ws, size_t ws_bytes, void* stream) {
  GWW_REQUIRE(values && diff && tp_values && fp_values && counts && ws, "gww_trig_split_f64: NULL argument");
  GWW_REQUIRE(cap >= 1 && cap <= TS_NMAX, "gww_trig_split_f64: cap=%ld must be 1..2^27", cap);
  GWW_REQUIRE(ws_bytes >= gww_trig_split_workspace_bytes(cap), "gww_trig_split_f64: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_trig_split_workspace_bytes(cap));
  GWW_REQUIRE(aligned(ws, 16), "gww_trig_split_f64: workspace must be 16-byte aligned");
  unsigned long long* blk = reinterpret_cast<unsigned long long*>(ws);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, counts, 3);
  GWW_LAUNCH_CHECK();
  const unsigned nb = (unsigned)ts_blocks(cap, TS_THREADS);
  hipLaunchKernelGGL(k_ts_split_count, dim3(nb), dim3(TS_THREADS), 0, s, values, diff, n_dev, (int)cap, tolerance, blk, counts + 2);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(TS_THREADS), 0, s, blk, (int)nb, counts, counts + 1);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ts_split_compact, dim3(nb), dim3(TS_THREADS), 0, s, values, diff, n_dev, (int)cap, tolerance,
                     (const unsigned long long*)blk, tp_values, fp_values);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_trig_steps_workspace_bytes(long n) {
  if (n < 1 || n > TS_NMAX) return 0;
  return ts_step_carve(nullptr, n).bytes;
}

extern "C" int gww_trig_steps_f64(const double* fp_sorted, const int* n_fp, long cap, const double* tp_sorted, const int* n_tp,
                                  long cap_tp, double duration, double prefactor, double Ninj, double* ranking, double* far,
                                  double* sens_frac, double* sens_vol, double* sens_vol_err, int* n_steps, void* ws,
                                  size_t ws_bytes, void* stream) {
  GWW_REQUIRE(fp_sorted && n_fp && tp_sorted && n_tp && ranking && far && sens_frac && sens_vol && sens_vol_err && n_steps && ws,
              "gww_trig_steps_f64: NULL argument");
  GWW_REQUIRE(cap >= 1 && cap <= TS_NMAX, "gww_trig_steps_f64: cap=%ld must be 1..2^27", cap);
  GWW_REQUIRE(cap_tp >= 1 && cap_tp <= TS_NMAX, "gww_trig_steps_f64: cap_tp=%ld must be 1..2^27", cap_tp);
  GWW_REQUIRE(duration > 0.0, "gww_trig_steps_f64: duration=%g must be positive", duration);
  GWW_REQUIRE(ws_bytes >= gww_trig_steps_workspace_bytes(cap), "gww_trig_steps_f64: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_trig_steps_workspace_bytes(cap));
  GWW_REQUIRE(aligned(ws, 16), "gww_trig_steps_f64: workspace must be 16-byte aligned");
  const TsStepWs w = ts_step_carve(ws, cap);
  hipStream_t s = (hipStream_t)stream;
  GWW_TRY(compact_launch(TsStepStarts{fp_sorted, n_fp, (int)cap, w.starts}, (unsigned)ts_blocks(cap, TS_THREADS), w.blk, n_steps,
                         nullptr, s));
  const TsStats O{ranking, far, sens_frac, sens_vol, sens_vol_err};
  hipLaunchKernelGGL(k_ts_step_stats, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, s, fp_sorted, n_fp, (int)cap,
                     (const int*)w.starts, (const int*)n_steps, tp_sorted, n_tp, (int)cap_tp, duration, prefactor, Ninj, O);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
