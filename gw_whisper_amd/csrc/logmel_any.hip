// Log-mel front end for ANY supported configuration (include/gww.h: gww_frontend_cfg) on gfx950: the general twin of
// logmel.hip, whose kernels stay the ones Whisper's published configuration runs.
//
// HF:models/whisper/feature_extraction_whisper.py (_np_extract_fbank_features) for
// WhisperFeatureExtractor(feature_size, sampling_rate, hop_length, chunk_length, n_fft):
//   zero-pad to n_samples -> reflect-pad n_fft / 2 -> n_fft-point periodic-Hann DFT every hop ->
//   |X|^2 (frames 0 .. n_samples / hop - 1) -> mel[n_mels, n_fft / 2 + 1] @ P -> log10(max(., 1e-10)) ->
//   per-segment max -> max(x, max - 8) -> (x + 4) / 4.
//
// Bytes per segment -- the floor, not the bound: as measured the kernel is VALU-issue-bound (0.24 ms for the 41 MB of 256
// one-second segments under Whisper's window, far from the HBM rate, and slower there than the fixed MFMA kernel of
// logmel.hip: profiles/short_context.md).  n input samples, live = ceil((n + n_fft / 2) / hop) frames
// that can see one of them:
//   in   4 n (+ 4 (n_fft - hop) per tile, the overlap of neighbouring tiles)
//   out  4 n_mels n_frames written by the finalize pass, which also reads back the 4 n_mels live raw values the frames
//        kernel wrote: 4 n_mels (n_frames + 2 live) in all.
//   2 s at 2048 Hz, n_fft 128, hop 16 (256 frames, all live):  16 KB in + 240 KB;  1 s at 16 kHz, chunk 1 (100 frames): 64 KB
//   in + 94 KB -- against 64 KB + 960 KB for the same second under the 30 s configuration.
// Two kernels, the dataflow of logmel.hip's VALU pair with every size taken from the handle:
//   k_logmel_any_frames    DFT + mel + log10 of the LIVE frames only, raw log-mel written in place, per-segment maximum
//                          by atomicMax on the ordered key
//   k_logmel_any_finalize  one [n_frames] row per workgroup: clamp to max - 8, affine, the constant of the dead frames
//                          (bitwise the same in every dead frame of a row: what k_stem_detect looks for)
// The per-frame arithmetic -- fold, DFT, power, mel, log10 -- lives in logmel_tile.h, which logmel_windows.hip (the windows of
// a series, each frame once) includes too: one body, so a frame's value does not depend on the kernel that computes it.
// The DFT folds the real input, x[n] +- x[n_fft - n] (half the multiply-adds), against the n_fft-entry twiddle table; the
// windowed even / odd frames and the twiddles sit in LDS; fp32 throughout.  A workgroup of 256 threads owns FT x G frames:
// G = 1, 2 or 4 thread groups (as many as 256 threads hold copies of the n_fft / 2 + 1 bins, in whole waves), each thread
// one bin (a stride of 256 / G bins when there are more) of the FT frames of its group.  FT (8 or 4) and G are chosen at
// handle creation so that the tile fits 64 KB of LDS: n_fft 1024 with hop 1024 takes 49 KB at FT 4.
// What that tile choice costs (correctness is not touched).  G comes from n_fft / 2 + 1 alone, and the "+ 1" -- the Nyquist
// bin -- spills a power-of-two n_fft into the next group size: n_fft 128 has 65 bins, so G = 2 with groups of 128 threads,
// of which 63 idle through the DFT loop (a group of 64 would run the loop twice for one bin, the same time per frame);
// n_fft 400 keeps 201 of 256 threads busy, n_fft 64 (33 bins) 33 of 64.  A lane reads its twiddles at ct[(k n) mod n_fft],
// a stride of k words across the wave: even k collide on the LDS banks (2-way for k = 2 mod 4, more the more twos k
// holds), where the ev / od reads are wave-uniform broadcasts.  Taking bin n_fft / 2 out of the loop (its "twiddles" are
// +-1: an alternating sum) and walking each lane's twiddle in registers by a rotation recurrence would remove both; the
// step after that is the one DESIGN.md names, the two contractions on the fp32 matrix cores.
#include "logmel_tile.h"
#include "device_sort.h"

namespace gww {

// The LDS tile (logmel_tile.h: AnyTile) in floats
static size_t any_lds_floats(int n_fft, int hop, int S, int ftw) {
  const size_t span4 = ((size_t)hop * (ftw - 1) + n_fft + 3) / 4 * 4;
  return span4 + 2 * (size_t)ftw * S + 2 * (size_t)n_fft + (size_t)ftw * (S + 1) + 4;
}

int logmel_any_plan(const gww_frontend_cfg* c, LogmelAnyPlan* p) {
  p->n_mels = c->n_mels;
  p->n_fft = c->n_fft;
  p->hop = c->hop_length;
  p->chunk = c->n_samples;
  p->n_frames = c->n_samples / c->hop_length;
  const int nfreq = c->n_fft / 2 + 1;
  p->S = (nfreq + 3) / 4 * 4;
  const int gmax = nfreq <= 64 ? 4 : nfreq <= 128 ? 2 : 1;
  for (int ft = 8; ft >= 4; ft /= 2)
    for (int g = gmax; g >= 1; g /= 2) {
      const size_t bytes = any_lds_floats(c->n_fft, c->hop_length, p->S, ft * g) * sizeof(float);
      if (bytes <= kAnyLdsMax) {
        p->ft = ft;
        p->groups = g;
        p->lds_bytes = bytes;
        return GWW_OK;
      }
    }
  return fail(GWW_ERR_ARG, "logmel_any_plan: n_fft=%d hop_length=%d: no tile fits the LDS", c->n_fft, c->hop_length);
}

// grid (cdiv(live, FT G), n_seg, n_outer), 256 threads, p.lds_bytes of dynamic LDS.  Segment blockIdx.z * n_seg + blockIdx.y
// starts at wave + blockIdx.z * outer_stride + blockIdx.y * stride: one stride for a batch of segments, two for the
// windows of a multi-row series read in place (logmel_windows.hip)
template <int FT>
__global__ __launch_bounds__(kAnyThreads, kAnyWaves) void k_logmel_any_frames(const float* __restrict__ wave, long stride, int n_eff,
                                                                   int live, LogmelAnyPlan p, AnyTables tb,
                                                                   float* __restrict__ out,
                                                                   unsigned int* __restrict__ seg_max,
                                                                   long outer_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = p.n_fft / 2, hop = p.hop, nm = p.n_mels;
  const AnyTile T = any_tile(lds, p, FT);
  const int ftw = T.ftw;

  const int tid = threadIdx.x;
  const int seg = blockIdx.z * gridDim.y + blockIdx.y;
  const int t0 = blockIdx.x * ftw;
  const float* x = wave + (long)blockIdx.z * outer_stride + (long)blockIdx.y * stride;

  // the samples of this tile: reflected once at either end of the n_samples buffer, zero from n_eff on (and wherever a
  // frame past the last one would reach: those frames are never stored)
  for (int i = tid; i < T.span; i += kAnyThreads) {
    long q = (long)t0 * hop - H + i;
    if (q < 0) q = -q;
    if (q >= p.chunk) q = 2L * (p.chunk - 1) - q;
    T.xs[i] = (q >= 0 && q < n_eff) ? x[q] : 0.0f;
  }
  any_load_twiddles(T, p, tb);
  __syncthreads();
  const float* xs = T.xs;
  any_fold(T, p, tb, [xs, hop](int f, int n) { return xs[f * hop + n]; });
  __syncthreads();
  any_dft_power<FT>(T, p);
  __syncthreads();

  // mel projection + log10; thread -> (mel, frame), frame fastest: a store instruction writes runs of one mel row
  float lmax = -INFINITY;
  for (int i = tid; i < ftw * nm; i += kAnyThreads) {
    const int m = i / ftw, f = i - m * ftw;
    const int t = t0 + f;
    if (t >= live) continue;
    const float lg = any_mel_log10(T, p, tb, f, m);
    out[((long)seg * nm + m) * p.n_frames + t] = lg;
    lmax = fmaxf(lmax, lg);
  }
  lmax = wave_max(lmax);
  if ((tid & 63) == 0) T.red[tid >> 6] = lmax;
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(fmaxf(T.red[0], T.red[1]), fmaxf(T.red[2], T.red[3]));
    if (m > -INFINITY) atomicMax(&seg_max[seg], ordered_u32(m));
  }
}

// grid (n_mels, n_seg), 256 threads: one [n_frames] row per workgroup.  VEC: n_frames % 4 == 0 and out 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kAnyThreads) void k_logmel_any_finalize(float* __restrict__ out, int live, int n_frames,
                                                                     const unsigned int* __restrict__ seg_max) {
  const int seg = blockIdx.z * gridDim.y + blockIdx.y, m = blockIdx.x;
  float mx = from_ordered_u32(seg_max[seg]);
  mx = fmaxf(mx, live < n_frames ? -10.0f : mx);     // dead frames contribute log10(1e-10) = -10
  const float floor_v = mx - 8.0f;
  const float padv = (fmaxf(-10.0f, floor_v) + 4.0f) * 0.25f;
  float* rowf = out + ((long)seg * gridDim.x + m) * n_frames;
  if (VEC) {
    float4* row = reinterpret_cast<float4*>(rowf);
    for (int i = threadIdx.x; i < n_frames / 4; i += kAnyThreads) {
      const int t = i * 4;
      float4 v;
      if (t >= live) {
        v = make_float4(padv, padv, padv, padv);
      } else {
        v = row[i];
        v.x = any_affine(v.x, floor_v);
        v.y = (t + 1 < live) ? any_affine(v.y, floor_v) : padv;
        v.z = (t + 2 < live) ? any_affine(v.z, floor_v) : padv;
        v.w = (t + 3 < live) ? any_affine(v.w, floor_v) : padv;
      }
      row[i] = v;
    }
  } else {
    for (int t = threadIdx.x; t < n_frames; t += kAnyThreads) rowf[t] = t < live ? any_affine(rowf[t], floor_v) : padv;
  }
}

int launch_logmel_any(const LogmelAnyPlan& p, const float* tables, const float* wave, int n_seg, int n_eff, int live,
                      long wave_stride, float* out, float* seg_max, hipStream_t s, int n_outer, long outer_stride) {
  GWW_REQUIRE(live >= 1 && live <= p.n_frames && n_eff >= 0 && n_eff <= p.chunk, "logmel_any: live=%d n_eff=%d out of range",
              live, n_eff);
  GWW_REQUIRE(n_seg >= 1 && n_seg <= 65535, "logmel_any: n_seg=%d (1 .. 65535 per call)", n_seg);
  GWW_REQUIRE(n_outer >= 1 && n_outer <= 65535, "logmel_any: n_outer=%d (1 .. 65535 per call)", n_outer);
  GWW_REQUIRE((p.ft == 8 || p.ft == 4) && p.lds_bytes <= kAnyLdsMax, "logmel_any: bad plan");
  const AnyTables tb = any_tables(tables, p.n_fft);
  unsigned int* mx = reinterpret_cast<unsigned int*>(seg_max);
  const dim3 g1((unsigned)cdiv(live, p.ft * p.groups), (unsigned)n_seg, (unsigned)n_outer);
  if (p.ft == 8)
    hipLaunchKernelGGL(k_logmel_any_frames<8>, g1, dim3(kAnyThreads), p.lds_bytes, s, wave, wave_stride, n_eff, live, p, tb,
                       out, mx, outer_stride);
  else
    hipLaunchKernelGGL(k_logmel_any_frames<4>, g1, dim3(kAnyThreads), p.lds_bytes, s, wave, wave_stride, n_eff, live, p, tb,
                       out, mx, outer_stride);
  GWW_LAUNCH_CHECK();
  const dim3 g2((unsigned)p.n_mels, (unsigned)n_seg, (unsigned)n_outer);
  if (p.n_frames % 4 == 0 && aligned(out, 16))
    hipLaunchKernelGGL(k_logmel_any_finalize<true>, g2, dim3(kAnyThreads), 0, s, out, live, p.n_frames, mx);
  else
    hipLaunchKernelGGL(k_logmel_any_finalize<false>, g2, dim3(kAnyThreads), 0, s, out, live, p.n_frames, mx);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww
