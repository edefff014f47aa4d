// The glitch scan (glitch_scan.py): the glitch head in eval mode over the windows of a strain series,
// and the events of every class built from the per-window results, all on the device.
//   k_head_scan       the chain walk of classify.hip's k_head_fwd without dropout, labels or saved activations (the
//                     inference instantiation chain_fwd<HeadChain, false, false>: same k order, same bits in the logits),
//                     tail: one wave per row -> class (argmax_better), its softmax probability, optionally all of them
//   k_events_walk     one wave per class walks the series 64 windows per ballot step, as cluster_wave.h does, but folds a
//                     step's triggers a whole run at a time: the previous trigger of every lane comes from the ballot, so
//                     the lanes that open an event are a second ballot, and the (few) runs between them are folded with one
//                     wave maximum each.  A closed event leaves (windows, last window, peak window) at its FIRST window's
//                     slot of the workspace; the opening lanes are the head flags
//   k_events_compact  one workgroup scans the head flags in window order and gathers the events: they come out ordered by
//                     their first window with no sort, times and probabilities are read back from the inputs by index
// No float atomics, no host synchronisation, every element of the workspace that is read has one writer: identical calls
// give identical bits.
#include "cluster_wave.h"
#include "device_sort.h"
#include "head_chain.h"

namespace gww {

using HeadChain = Chain<512, 256, 128>;      // models.glitch_classifier's head, as in classify.hip

// ---- head, eval mode --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CH_THREADS) void k_head_scan(const float* __restrict__ x, ChainFwdArgs<HeadChain::L> P, int B,
                                                          int d_in, int C, long row_off, int* __restrict__ cls,
                                                          float* __restrict__ prob, float* __restrict__ probs) {
  extern __shared__ __attribute__((aligned(16))) float sm_scan[];
  const ChainRows Z = chain_fwd<HeadChain, false, false>(sm_scan, x, P, B, d_in, C, NoDrop{});
  // tail: one wave per row, lane c holds logit c (k_head_fwd's argmax and its sums relative to the row maximum)
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = wave; m < CH_ROWS; m += CH_WAVES) {
    const long row = row0 + m;
    if (row >= B) break;                     // uniform per wave
    const float z = lane < C ? Z.p[m * Z.ld + lane] : -INFINITY;
    float bv = z;
    int bi = lane < C ? lane : CH_CMAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    const float mx = wave_max(z);
    const float e = lane < C ? expf(z - mx) : 0.f;
    const float se = wave_sum(e);
    const long o = row_off + row;
    if (lane == 0) {
      cls[o] = bi;
      prob[o] = 1.f / se;                    // e == 1 at the maximum: the predicted class's e / se
    }
    if (probs && lane < C) probs[o * C + lane] = e / se;
  }
}

// ---- events -----------------------------------------------------------------------------------------------------------
// workspace: four int32 arrays of n, each on a 256-byte boundary
struct EventWs {
  int *head, *cnt, *last, *peak;   // head[i]: window i opens an event; at such i: its windows, last window, peak window
  size_t bytes;
};
static EventWs events_carve(void* ws, long n) {
  Arena a;
  char* base = reinterpret_cast<char*>(ws);
  EventWs w;
  w.head = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.cnt = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.last = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.peak = reinterpret_cast<int*>(base + a.take((size_t)n * 4));
  w.bytes = a.total();
  return w;
}

// Workgroup c = class c, one wave.  Every head[i] has exactly one writer: the wave of cls[i], wave 0 for a class outside
// 0..63.  The running event is wave-uniform: first / last / peak window, the last stamp, the peak probability, the count.
__global__ __launch_bounds__(64) void k_events_walk(const double* __restrict__ times, const int* __restrict__ cls,
                                                    const float* __restrict__ prob, int n, float thr, double gap,
                                                    unsigned long long ignore, EventWs W) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const bool live = !((ignore >> c) & 1ull);
  bool have = false;
  int first = 0, last_i = 0, peak_i = 0, cnt = 0;
  double t_last = 0.0;
  float p_peak = 0.f;
  auto close = [&]() {
    if (lane == 0) { W.cnt[first] = cnt; W.last[first] = last_i; W.peak[first] = peak_i; }
  };
  // the next step's loads are issued before this step's fold
  int cl_n = -1;
  float p_n = 0.f;
  double t_n = 0.0;
  if (lane < n) { cl_n = cls[lane]; p_n = prob[lane]; t_n = times[lane]; }
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const int cl = cl_n;
    const float p = p_n;
    const double t = t_n;
    const bool in = i < n;
    {
      const long j = (long)i + 64;
      cl_n = -1;
      if (j < n) { cl_n = cls[j]; p_n = prob[j]; t_n = times[j]; }
    }
    const bool mine = in && (cl == c || (c == 0 && (cl < 0 || cl >= 64)));
    const bool trig = in && live && cl == c && p > thr;               // a NaN probability is no trigger
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(trig);
    // the previous trigger of this class: the next set lane below, else the running event's last window
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __builtin_clzll(below) : 0;
    const double tprev = __shfl(t, pl, 64);
    const bool hasprev = below != 0ull || have;
    const double tp = below ? tprev : t_last;
    const bool head = trig && (!hasprev || (t - tp) > gap);           // fp64, strict
    if (mine) W.head[i] = head ? 1 : 0;
    if (!mask) continue;
    const unsigned long long hm = __builtin_amdgcn_ballot_w64(head);
    unsigned long long rest = mask;
    while (rest) {                                                     // one trip per run of triggers of one event
      const int l0 = __builtin_ctzll(rest);
      if ((hm >> l0) & 1ull) {
        if (have) close();
        have = true;
        first = peak_i = base + l0;
        p_peak = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p), l0));
        cnt = 0;
      }
      const unsigned long long above = l0 == 63 ? 0ull : (~0ull << (l0 + 1));
      const unsigned long long hnext = hm & above;
      const unsigned long long seg = hnext ? rest & ((1ull << __builtin_ctzll(hnext)) - 1ull) : rest;
      cnt += __builtin_popcountll(seg);
      const int ll = 63 - __builtin_clzll(seg);
      last_i = base + ll;
      t_last = readlane_f64(t, ll);
      const bool inseg = (seg >> lane) & 1ull;
      const float mx = wave_max(inseg ? p : -INFINITY);
      if (mx > p_peak) {                                               // strict: an earlier equal peak stays
        p_peak = mx;
        peak_i = base + __builtin_ctzll(__builtin_amdgcn_ballot_w64(inseg && p == mx));   // the run's first maximum
      }
      rest &= ~seg;
    }
  }
  if (have) close();
}

// one workgroup of 1024: thread t of a trip owns windows base + 4 t .. + 3
constexpr int EV_THREADS = 1024, EV_WAVES = EV_THREADS / 64, EV_PER = 4;
__global__ __launch_bounds__(EV_THREADS) void k_events_compact(const double* __restrict__ times, const int* __restrict__ cls,
                                                               const float* __restrict__ prob, int n, EventWs W, int cap,
                                                               int* __restrict__ ev_cls, int* __restrict__ ev_first,
                                                               int* __restrict__ ev_n, double* __restrict__ ev_t_start,
                                                               double* __restrict__ ev_t_end, double* __restrict__ ev_t_peak,
                                                               float* __restrict__ ev_p_peak, int* __restrict__ count) {
  __shared__ int part[EV_WAVES];
  int carry = 0;
  for (long base = 0; base < n; base += EV_THREADS * EV_PER) {         // n is the workgroup's: every thread takes the same trips
    const long i0 = base + (long)threadIdx.x * EV_PER;
    int f[EV_PER], mine = 0;
#pragma unroll
    for (int u = 0; u < EV_PER; ++u) {
      f[u] = i0 + u < n ? W.head[i0 + u] : 0;
      mine += f[u];
    }
    int tot;
    int pos = carry + block_scan<int, EV_WAVES>(mine, part, &tot) - mine;
#pragma unroll
    for (int u = 0; u < EV_PER; ++u) {
      if (!f[u]) continue;
      if (pos < cap) {
        const int i = (int)(i0 + u), pk = W.peak[i];
        ev_cls[pos] = cls[i];
        ev_first[pos] = i;
        ev_n[pos] = W.cnt[i];
        ev_t_start[pos] = times[i];
        ev_t_end[pos] = times[W.last[i]];
        ev_t_peak[pos] = times[pk];
        ev_p_peak[pos] = prob[pk];
      }
      ++pos;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) count[0] = carry;                              // counts on past cap
}

}  // namespace gww

using namespace gww;

extern "C" int gww_head_scan_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, long row_offset,
                                 int* cls, float* prob, float* probs, void* stream) {
  const char* who = "gww_head_scan_f32";
  GWW_TRY(chain_check_shape(who, B, 1024, d_in, C, 1));
  GWW_REQUIRE(cls && prob, "%s: NULL cls or prob", who);
  GWW_REQUIRE(row_offset >= 0, "%s: row_offset=%ld is negative", who, row_offset);
  GWW_TRY(chain_check_operands(who, HeadChain::L, x, params, nullptr, nullptr));
  return chain_launch_fwd(k_head_scan, chain_lds_bytes<HeadChain>(d_in), B, nullptr, 1.0, nullptr, (hipStream_t)stream, x,
                          chain_fwd_args<HeadChain::L>(params, nullptr, nullptr), B, d_in, C, row_offset, cls, prob, probs);
}

extern "C" size_t gww_glitch_events_workspace_bytes(long n) {
  return n < 1 ? 0 : 4 * (((size_t)n * 4 + 255) / 256 * 256);   // events_carve
}

extern "C" int gww_glitch_events(const double* times, const int* cls, const float* prob, long n, float prob_threshold,
                                 double gap, unsigned long long ignore, int cap, int* ev_cls, int* ev_first, int* ev_n,
                                 double* ev_t_start, double* ev_t_end, double* ev_t_peak, float* ev_p_peak, int* count,
                                 void* ws, size_t ws_bytes, void* stream) {
  const char* who = "gww_glitch_events";
  GWW_REQUIRE(n >= 0 && n <= 2147483647L - 64 && cap >= 0, "%s: n=%ld must be 0..2^31-65 and cap=%d >= 0", who, n, cap);
  GWW_REQUIRE(count && (n == 0 || (times && cls && prob && ws)), "%s: NULL argument", who);
  GWW_REQUIRE(cap == 0 || (ev_cls && ev_first && ev_n && ev_t_start && ev_t_end && ev_t_peak && ev_p_peak),
              "%s: NULL event array with cap=%d", who, cap);
  GWW_REQUIRE(ws_bytes >= gww_glitch_events_workspace_bytes(n), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
              gww_glitch_events_workspace_bytes(n));
  GWW_REQUIRE(n == 0 || aligned(ws, 16), "%s: ws must be 16-byte aligned", who);
  const EventWs W = n ? events_carve(ws, n) : EventWs{nullptr, nullptr, nullptr, nullptr, 0};
  hipStream_t s = (hipStream_t)stream;
  if (n) {
    hipLaunchKernelGGL(k_events_walk, dim3(CH_CMAX), dim3(64), 0, s, times, cls, prob, (int)n, prob_threshold, gap, ignore, W);
    GWW_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_events_compact, dim3(1), dim3(EV_THREADS), 0, s, times, cls, prob, (int)n, W, cap, ev_cls, ev_first, ev_n,
                     ev_t_start, ev_t_end, ev_t_peak, ev_p_peak, count);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
