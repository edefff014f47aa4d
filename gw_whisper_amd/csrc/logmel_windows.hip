// Log-mel features of the overlapping windows of a strain series on gfx950: window w covers samples
// [w step, w step + L) of every row of series [R, N], L = n_samples of the front-end handle (so a window has no dead
// frame), and out [n, R, n_mels, n_frames] (or [R, n, ...]) holds, bit for bit, what logmel_any.hip's kernels give for
// the materialised window.  The sliding-window consumers (inference.evaluate_slices, real_events.scan_events) cut 2048
// samples every 204: consecutive windows share 90 % of their samples, and with step = s hop frame t of window w and
// frame t - s of window w + 1 see the same n_fft samples -- unless one of them touches its window's edge, where the
// reflect padding differs.  So (logmel_host.cpp: logmel_windows_plan decides; include/gww.h: gww_windows_plan)
//   shared route      k_logmel_stream_frames   raw log10 mel of the hop-spaced frames of the series from window w0's first
//                                              interior frame to window w0 + n - 1's last: no reflection, no maximum;
//                                              workspace [R, n_mels, G]
//                     k_logmel_window_edges    the edge_lo + edge_hi frames of every (window, row) that see the reflect
//                                              padding, reflected about the window's own first and last sample;
//                                              workspace [n, R, n_mels, E].  A tile packs edge frames of any windows.
//                     k_logmel_window_finalize one workgroup per (window, row): maximum over its n_mels x n_frames raw
//                                              values (interior from the stream, edges from the edge buffer), clamp to
//                                              max - 8, affine, whole 16-byte stores where n_frames % 4 == 0
//   per-window route  logmel_any.hip's own two kernels on the windows in place: a second stride, no copy
// For n_fft 128, hop 12, L 2048, step 204 (170 frames: 6 + 160 + 4) a batch of n windows runs 17 (n - 1) + 160 + 10 n
// DFTs per row instead of 170 n.
// Why the bits agree: every raw value comes from the functions of logmel_tile.h -- fold, n-ordered fmaf chains, power,
// k-ordered mel chain, log10 in fp64 -- which see a frame's n_fft samples and nothing of its slot, tile or kernel; the
// maximum is order-independent (fmaxf over the same set; the per-window route's ordered-key atomicMax is the same
// maximum) and the clamp and affine map are any_affine in both.
// Bytes per (window, row) on the shared route: the finalize pass reads its 4 n_mels n_frames raw values twice (the second
// time from L2) and writes 4 n_mels n_frames; the stream pass reads the series once (+ the tiles' overlap) and writes
// 4 n_mels s per window; the edge pass reads n_fft + hop (E - 1) samples and writes 4 n_mels E.
#include "logmel_tile.h"

namespace gww {

struct WinGeom {
  int R, n;            // rows, windows
  int L, F;            // window length, frames per window
  int lo, hi0, E;      // edge frames at the start, first edge frame at the end, edge frames per window
  int s;               // step / hop
  long G;              // stream frames
  long origin;         // w0 * step: window 0 of this call starts here
  long step, row_stride;
  long n_series;
};

// grid (cdiv(G, FT groups), R), 256 threads, p.lds_bytes of dynamic LDS
template <int FT>
__global__ __launch_bounds__(kAnyThreads, kAnyWaves) void k_logmel_stream_frames(const float* __restrict__ series, WinGeom g,
                                                                      LogmelAnyPlan p, AnyTables tb,
                                                                      float* __restrict__ stream) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = p.n_fft / 2, hop = p.hop, nm = p.n_mels;
  const AnyTile T = any_tile(lds, p, FT);
  const int ftw = T.ftw, tid = threadIdx.x, r = blockIdx.y;
  const long t0 = (long)blockIdx.x * ftw;                       // first stream frame of this tile
  const float* x = series + (long)r * g.row_stride;
  // stream frame j is frame lo + j of window 0: it starts lo hop - n_fft / 2 >= 0 samples behind the origin.  Frames past
  // the last one are never stored; what they would read behind the series is zero
  const long q0 = g.origin + (t0 + g.lo) * hop - H;
  for (int i = tid; i < T.span; i += kAnyThreads) {
    const long q = q0 + i;
    T.xs[i] = q < g.n_series ? x[q] : 0.0f;
  }
  any_load_twiddles(T, p, tb);
  __syncthreads();
  const float* xs = T.xs;
  any_fold(T, p, tb, [xs, hop](int f, int n) { return xs[f * hop + n]; });
  __syncthreads();
  any_dft_power<FT>(T, p);
  __syncthreads();
  for (int i = tid; i < ftw * nm; i += kAnyThreads) {
    const int m = i / ftw, f = i - m * ftw;
    const long j = t0 + f;
    if (j >= g.G) continue;
    stream[((long)r * nm + m) * g.G + j] = any_mel_log10(T, p, tb, f, m);
  }
}

// grid (cdiv(n R E, FT groups)), 256 threads, p.lds_bytes of dynamic LDS: edge frame j = (w R + r) E + e of the call, e
// counting the edge frames of a window in frame order
template <int FT>
__global__ __launch_bounds__(kAnyThreads, kAnyWaves) void k_logmel_window_edges(const float* __restrict__ series, WinGeom g,
                                                                     LogmelAnyPlan p, AnyTables tb,
                                                                     float* __restrict__ edges) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = p.n_fft / 2, hop = p.hop, nm = p.n_mels;
  const AnyTile T = any_tile(lds, p, FT);
  const int ftw = T.ftw, tid = threadIdx.x;
  const long j0 = (long)blockIdx.x * ftw, total = (long)g.n * g.R * g.E;
  any_load_twiddles(T, p, tb);
  // no staging: a tile's frames belong to different windows.  Reflected about the window's own first and last sample,
  // exactly as k_logmel_any_frames reflects about the segment's
  any_fold(T, p, tb, [&](int f, int n) {
    const long j = j0 + f;
    if (j >= total) return 0.0f;
    const long seg = j / g.E;
    const int e = (int)(j - seg * g.E);
    const long w = seg / g.R;
    const int r = (int)(seg - w * g.R);
    const int t = e < g.lo ? e : g.hi0 + (e - g.lo);
    long q = (long)t * hop - H + n;
    if (q < 0) q = -q;
    if (q >= g.L) q = 2L * (g.L - 1) - q;
    return (q >= 0 && q < g.L) ? series[(long)r * g.row_stride + g.origin + w * g.step + q] : 0.0f;
  });
  __syncthreads();
  any_dft_power<FT>(T, p);
  __syncthreads();
  for (int i = tid; i < ftw * nm; i += kAnyThreads) {
    const int m = i / ftw, f = i - m * ftw;
    const long j = j0 + f;
    if (j >= total) continue;
    const long seg = j / g.E;
    const int e = (int)(j - seg * g.E);
    edges[(seg * nm + m) * g.E + e] = any_mel_log10(T, p, tb, f, m);
  }
}

// grid (n R), 256 threads: one (window, row) per workgroup.  VEC: n_frames % 4 == 0 and out 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kAnyThreads) void k_logmel_window_finalize(const float* __restrict__ stream,
                                                                        const float* __restrict__ edges, WinGeom g,
                                                                        int nm, int rows_major, float* __restrict__ out) {
  __shared__ float red[4];
  const int tid = threadIdx.x, F = g.F;
  const long seg = blockIdx.x, w = seg / g.R;
  const int r = (int)(seg - w * g.R);
  const float* st = stream + (long)r * nm * g.G + w * g.s;      // st[m G + (t - lo)], lo <= t < hi0
  const float* ed = edges + seg * nm * g.E;                     // ed[m E + e]
  auto raw = [&](int m, int t) {
    return t < g.lo ? ed[m * g.E + t] : t >= g.hi0 ? ed[m * g.E + g.lo + (t - g.hi0)] : st[(long)m * g.G + (t - g.lo)];
  };
  float mx = -INFINITY;
  for (int i = tid; i < nm * F; i += kAnyThreads) {
    const int m = i / F;
    mx = fmaxf(mx, raw(m, i - m * F));
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float floor_v = mx - 8.0f;
  float* o = out + (rows_major ? (long)r * g.n + w : seg) * nm * F;
  if (VEC) {
    float4* o4 = reinterpret_cast<float4*>(o);
    for (int i = tid; i < nm * F / 4; i += kAnyThreads) {
      const int m = (i * 4) / F, t = i * 4 - m * F;             // F % 4 == 0: the four frames are of one mel row
      float4 v;
      v.x = any_affine(raw(m, t), floor_v);
      v.y = any_affine(raw(m, t + 1), floor_v);
      v.z = any_affine(raw(m, t + 2), floor_v);
      v.w = any_affine(raw(m, t + 3), floor_v);
      o4[i] = v;
    }
  } else {
    for (int i = tid; i < nm * F; i += kAnyThreads) {
      const int m = i / F;
      o[i] = any_affine(raw(m, i - m * F), floor_v);
    }
  }
}

int launch_logmel_windows(const LogmelAnyPlan& p, const gww_windows_plan& wp, const float* tables, const float* series,
                          int n_rows, int n_series, long row_stride, int step, int w0, int n_windows, float* out,
                          int out_rows_major, void* workspace, hipStream_t s) {
  GWW_REQUIRE((p.ft == 8 || p.ft == 4) && p.lds_bytes <= kAnyLdsMax, "logmel_windows: bad plan");
  GWW_REQUIRE(n_rows >= 1 && n_windows >= 1 && w0 >= 0 && step >= 1, "logmel_windows: n_rows=%d n_windows=%d w0=%d step=%d",
              n_rows, n_windows, w0, step);
  const long segs = (long)n_windows * n_rows;
  GWW_REQUIRE(segs <= 0x7FFFFFFFL, "logmel_windows: n_windows=%d x n_rows=%d exceeds what a grid indexes (2^31 - 1)",
              n_windows, n_rows);
  const long origin = (long)w0 * step;
  if (wp.route == GWW_WINDOWS_PER_WINDOW) {
    // the general kernels on the windows in place: the output's inner index on gridDim.y, its outer one on gridDim.z (16
    // bits each: the outer one loops here)
    float* seg_max = static_cast<float*>(workspace);
    GWW_HIP(hipMemsetAsync(seg_max, 0, sizeof(float) * (size_t)segs, s));
    const int inner = out_rows_major ? n_windows : n_rows, outer = out_rows_major ? n_rows : n_windows;
    const long inner_stride = out_rows_major ? (long)step : row_stride, outer_stride = out_rows_major ? row_stride : (long)step;
    GWW_REQUIRE(inner <= 65535, "logmel_windows: %s=%d (1 .. 65535 per call on the per-window route in this layout)",
                out_rows_major ? "n_windows" : "n_rows", inner);
    for (int o0 = 0; o0 < outer; o0 += 65535) {
      const int m = outer - o0 < 65535 ? outer - o0 : 65535;
      const long seg0 = (long)o0 * inner;
      GWW_TRY(launch_logmel_any(p, tables, series + origin + o0 * outer_stride, inner, p.chunk, p.n_frames, inner_stride,
                                out + seg0 * p.n_mels * p.n_frames, seg_max + seg0, s, m, outer_stride));
    }
    return GWW_OK;
  }
  GWW_REQUIRE(n_rows <= 65535, "logmel_windows: n_rows=%d (1 .. 65535 on the shared route)", n_rows);
  WinGeom g;
  g.R = n_rows;
  g.n = n_windows;
  g.L = p.chunk;
  g.F = p.n_frames;
  g.lo = wp.edge_lo;
  g.hi0 = wp.edge_lo + wp.interior;
  g.E = wp.edge_lo + wp.edge_hi;
  g.s = step / p.hop;
  g.G = wp.stream_frames;
  g.origin = origin;
  g.step = step;
  g.row_stride = row_stride;
  g.n_series = n_series;
  const AnyTables tb = any_tables(tables, p.n_fft);
  const int ftw = p.ft * p.groups;
  float* stream = static_cast<float*>(workspace);
  float* edges = stream + (long)n_rows * p.n_mels * g.G;
  const long stream_tiles = cdiv(g.G, ftw), edge_tiles = cdiv(segs * g.E, ftw);
  GWW_REQUIRE(stream_tiles <= 0x7FFFFFFFL && edge_tiles <= 0x7FFFFFFFL, "logmel_windows: n_windows=%d: too many tiles for a grid",
              n_windows);
  const dim3 gs((unsigned)stream_tiles, (unsigned)n_rows), ge((unsigned)edge_tiles);
  if (p.ft == 8) {
    hipLaunchKernelGGL(k_logmel_stream_frames<8>, gs, dim3(kAnyThreads), p.lds_bytes, s, series, g, p, tb, stream);
    GWW_LAUNCH_CHECK();
    if (g.E > 0) hipLaunchKernelGGL(k_logmel_window_edges<8>, ge, dim3(kAnyThreads), p.lds_bytes, s, series, g, p, tb, edges);
  } else {
    hipLaunchKernelGGL(k_logmel_stream_frames<4>, gs, dim3(kAnyThreads), p.lds_bytes, s, series, g, p, tb, stream);
    GWW_LAUNCH_CHECK();
    if (g.E > 0) hipLaunchKernelGGL(k_logmel_window_edges<4>, ge, dim3(kAnyThreads), p.lds_bytes, s, series, g, p, tb, edges);
  }
  GWW_LAUNCH_CHECK();
  const dim3 gf((unsigned)segs);
  if (p.n_frames % 4 == 0 && aligned(out, 16))
    hipLaunchKernelGGL(k_logmel_window_finalize<true>, gf, dim3(kAnyThreads), 0, s, stream, edges, g, p.n_mels, out_rows_major,
                       out);
  else
    hipLaunchKernelGGL(k_logmel_window_finalize<false>, gf, dim3(kAnyThreads), 0, s, stream, edges, g, p.n_mels, out_rows_major,
                       out);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww
