// The per-frame arithmetic of the general log-mel front end, shared by logmel_any.hip (one segment per grid row) and
// logmel_windows.hip (the windows of a series): the LDS tile, the even / odd fold against the window table, the n-ordered
// fmaf chains against the twiddles, re * re + im * im, the k-ordered mel chain and log10 in fp64.  Every kernel that
// produces a raw log-mel value runs THESE functions, so a frame's value depends on its n_fft samples alone -- not on its
// slot in the tile, its thread group or the kernel around it.  That is what makes a shared frame bit-identical to the
// same frame computed per window.
#pragma once

#include "common.h"

#include <math.h>

namespace gww {

constexpr int kAnyThreads = 256;
constexpr size_t kAnyLdsMax = 64 * 1024;
// waves per SIMD the frame kernels are compiled for (80 VGPRs; the LDS tile leaves room for more).  Without the bound the
// FT 8 kernels compile to 82 - 134 VGPRs, depending on nothing but their addressing; with it they keep five dwords of
// scratch outside the DFT loop and measure 2 - 3 % faster than at five waves (profiles/logmel_windows.md)
constexpr int kAnyWaves = 6;

struct AnyTables {
  const float *win, *cost, *sint, *fbT;   // [n_fft] x 3, [n_fft / 2 + 1][n_mels]
};

__host__ __device__ inline AnyTables any_tables(const float* tables, int n_fft) {
  AnyTables tb;
  tb.win = tables;
  tb.cost = tables + n_fft;
  tb.sint = tables + 2 * n_fft;
  tb.fbT = tables + 3 * n_fft;
  return tb;
}

// The LDS tile in floats: xs [span4] | ev [ftw][S] | od [ftw][S] | ct [n_fft] | st [n_fft] | pw [ftw][S + 1] | red [4]
struct AnyTile {
  float *xs, *ev, *od, *ct, *st, *pw, *red;
  int ftw, span;
};

__device__ __forceinline__ AnyTile any_tile(float* lds, const LogmelAnyPlan& p, int FT) {
  const int N = p.n_fft, S = p.S;
  AnyTile t;
  t.ftw = FT * p.groups;
  t.span = p.hop * (t.ftw - 1) + N;
  const int span4 = (t.span + 3) / 4 * 4;
  t.xs = lds;
  t.ev = t.xs + span4;
  t.od = t.ev + t.ftw * S;
  t.ct = t.od + t.ftw * S;
  t.st = t.ct + N;
  t.pw = t.st + N;
  t.red = t.pw + t.ftw * (S + 1);
  return t;
}

__device__ __forceinline__ void any_load_twiddles(const AnyTile& T, const LogmelAnyPlan& p, const AnyTables& tb) {
  for (int i = threadIdx.x; i < p.n_fft; i += kAnyThreads) {
    T.ct[i] = tb.cost[i];
    T.st[i] = tb.sint[i];
  }
}

// windowed even / odd parts of the tile's frames; columns H + 1 .. S - 1 are zero.  sample(f, n): sample n of frame f
template <class Sample>
__device__ __forceinline__ void any_fold(const AnyTile& T, const LogmelAnyPlan& p, const AnyTables& tb, Sample sample) {
  const int N = p.n_fft, H = N / 2, S = p.S;
  for (int i = threadIdx.x; i < T.ftw * S; i += kAnyThreads) {
    const int f = i / S, n = i - f * S;
    float e = 0.f, o = 0.f;
    if (n <= H) {
      const float a = sample(f, n) * tb.win[n];
      if (n == 0 || n == H) {
        e = a;
      } else {
        // a +- x w with the second product fused: what -ffp-contract=fast made of "a + b, a - b" in the kernel the
        // published results and the golden files come from, written out so that no context can choose otherwise
        const float xb = sample(f, N - n), wb = tb.win[N - n];
        e = fmaf(xb, wb, a);
        o = fmaf(-xb, wb, a);
      }
    }
    T.ev[i] = e;
    T.od[i] = o;
  }
}

// the power spectrum of the tile's frames into pw: thread -> one bin (a stride of the group size when there are more) of
// the FT frames of its group
template <int FT>
__device__ __forceinline__ void any_dft_power(const AnyTile& T, const LogmelAnyPlan& p) {
  const int N = p.n_fft, nfreq = N / 2 + 1, S = p.S, PS = S + 1;
  const int tid = threadIdx.x;
  const int gsz = kAnyThreads / p.groups;          // a multiple of 64: a wave serves one group
  const int g = tid / gsz, b = tid - g * gsz;
  const float* evg = T.ev + g * FT * S;
  const float* odg = T.od + g * FT * S;
  const float *ct = T.ct, *st = T.st;
  for (int k = b; k < nfreq; k += gsz) {
    float re[FT], im[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) re[f] = im[f] = 0.f;
    int idx = 0;   // (k n) mod n_fft
    for (int n = 0; n < S; n += 4) {
      float c[4], s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = ct[idx];
        s[j] = st[idx];
        idx += k;
        if (idx >= N) idx -= N;
      }
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const float4 e4 = *reinterpret_cast<const float4*>(&evg[f * S + n]);
        const float4 o4 = *reinterpret_cast<const float4*>(&odg[f * S + n]);
        re[f] = fmaf(e4.x, c[0], re[f]);
        re[f] = fmaf(e4.y, c[1], re[f]);
        re[f] = fmaf(e4.z, c[2], re[f]);
        re[f] = fmaf(e4.w, c[3], re[f]);
        im[f] = fmaf(o4.x, s[0], im[f]);
        im[f] = fmaf(o4.y, s[1], im[f]);
        im[f] = fmaf(o4.z, s[2], im[f]);
        im[f] = fmaf(o4.w, s[3], im[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) T.pw[(g * FT + f) * PS + k] = fmaf(re[f], re[f], im[f] * im[f]);   // (pinned likewise)
  }
}

// raw log-mel of mel m of the tile's frame f
__device__ __forceinline__ float any_mel_log10(const AnyTile& T, const LogmelAnyPlan& p, const AnyTables& tb, int f, int m) {
  const int nfreq = p.n_fft / 2 + 1, nm = p.n_mels;
  const float* pf = T.pw + f * (p.S + 1);
  float acc = 0.f;
  for (int k = 0; k < nfreq; ++k) acc = fmaf(tb.fbT[k * nm + m], pf[k], acc);
  // log10 in fp64, rounded once (see logmel.hip: the dead frames' -10.0 must be what a live 1e-10 gives)
  return (float)log10((double)fmaxf(acc, 1e-10f));
}

__device__ __forceinline__ float any_affine(float v, float floor_v) { return (fmaxf(v, floor_v) + 4.0f) * 0.25f; }

}  // namespace gww
