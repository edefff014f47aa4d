// gw_whisper_amd -- the constant tail of a padded log-mel: detection and the fill of the residual stream (bf16 inference stem).
//
// The features of this workload are the log-mel of ~1 s of strain zero-padded to 30 s (Signal_vs_Noise/src/dataset.py:20-21,
// :46): behind the ~102 frames that see a sample every frame of a segment holds ONE value per mel bin (k_logmel_finalize's padv),
// so conv1's output is one row per segment from there on and conv2's, before the position embedding is added, one row for
// tokens 126 .. 1498.  encoder.hip then runs the stem on the first kStemTc = 256 frames only (conv1_mel.hip and gemm_v4.hip on a
// compact c1') and k_stem_fill expands the result; k_stem_detect decides ON THE DEVICE, per forward and per (half) batch,
// whether that is allowed: no host synchronisation, the full stem stays enqueued behind the shortcut and returns at once.
//
// Index derivation (Tc = kStemTc, Tt = Tc / 2 = kStemTt, Tin = t_in, T = Tin / 2; frames t, tokens j):
//   detected: mel[b, m, t] has the bits of mel[b, m, Tc - 6] for all t in [Tc - 6, Tin).
//   conv1 (k = 3, padding 1): c1[t] reads mel[t - 1 .. t + 1], mel[-1] = mel[Tin] = 0.
//     -> c1[t] is one row g1 for t in [Tc - 5, Tin - 2]; c1[Tin - 1] = f(const, const, 0) =: the edge row.
//     the compact c1' (the first Tc frames as a sequence of their own, frame Tc = padding):
//     c1'[t] = c1[t] for t <= Tc - 2 (reads mel up to Tc - 1), c1'[Tc - 1] = f(const, const, 0) = the edge row.
//   conv2 (k = 3, stride 2, padding 1): token j reads c1 frames 2 j - 1 .. 2 j + 1.
//     real token j is position-free constant  <=>  2 j - 1 >= Tc - 5 and 2 j + 1 <= Tin - 2  <=>  Tt - 2 <= j <= T - 2.
//     compact token j <= Tt - 3 reads c1' frames <= Tc - 5 <= Tc - 2: the real token j.
//     compact token Tt - 2 reads c1' frames Tc - 5 .. Tc - 3 = g1 g1 g1: the shared row of the real tokens Tt - 2 .. T - 2.
//     compact token Tt - 1 reads c1' frames Tc - 3, Tc - 2, Tc - 1 = g1 g1 edge = what real token T - 1 reads
//     (c1 frames Tin - 3, Tin - 2, Tin - 1); it gets pos[T - 1] from the compact position table (encoder.hip: pos_c).
//   An element changed at t = Tc - 7 is outside the detected range and reaches c1 frames <= Tc - 6, tokens <= Tt - 3, which the
//   compact stem computes from the data: the shortcut stays exact.
//
// Bit-identity: conv2's epilogue is out = fma(x, r, pos[j]) (gemm_v4.hip: EPI_CONV2T), one rounding.  The compact conv2 stores
// the shared row's x and r apart (xs[b, Tt - 2, :] and tr[b, :]) and k_stem_fill computes the same fma with the real pos[j].
#include "common.h"

namespace gww {

namespace {
constexpr int DET_U = 4;   // 16-byte loads in flight per thread
}

// flag (set to 1 in front of the launch) is cleared iff some mel[r, t], t in [t0, Tin), differs in its BIT PATTERN from mel[r, t0]
// (integers: NaN and -0 can never make the shortcut differ from the full stem).  Row r = (segment, mel bin), Tin % 4 == 0,
// ta = the first multiple of 4 above t0, q4 = (Tin - ta) / 4.  A thread that finds the flag cleared stops reading, so dense
// features cost one tile per resident workgroup.
__global__ __launch_bounds__(256) void k_stem_detect(const unsigned* __restrict__ mel, int* flag, long n_items, int Tin, int t0,
                                                     int ta, int q4) {
  const long stride = (long)gridDim.x * (256 * DET_U);
  for (long base = (long)blockIdx.x * (256 * DET_U) + threadIdx.x; base < n_items; base += stride) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    u32x4 v[DET_U];
    unsigned ref[DET_U];
    bool bad = false;
#pragma unroll
    for (int u = 0; u < DET_U; ++u) {
      long i = base + u * 256;
      i = i < n_items ? i : n_items - 1;   // (the tail repeats the last item: no branch around the loads)
      const long r = i / q4;
      const int k = (int)(i - r * q4);
      const unsigned* row = mel + r * Tin;
      ref[u] = row[t0];
      v[u] = *reinterpret_cast<const u32x4*>(row + ta + 4 * k);
      if (k == 0)   // the up to three elements between t0 and the first aligned one
        for (int t = t0 + 1; t < ta; ++t) bad |= row[t] != ref[u];
    }
#pragma unroll
    for (int u = 0; u < DET_U; ++u)
      bad |= v[u][0] != ref[u] || v[u][1] != ref[u] || v[u][2] != ref[u] || v[u][3] != ref[u];
    if (bad) {
      __hip_atomic_store(flag, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an ordinary vector store)
      return;
    }
  }
}

// x [B, T, d] fp32 from the compact stem (runs iff *flag == 1):
//   x[b, j] = xs[b, j]                       j <= Tt - 3
//   x[b, j] = fma(xs[b, Tt - 2], tr[b], pos[j])   Tt - 2 <= j <= T - 2     (xs[b, Tt - 2] holds x, tr[b] the sigmoid factor r)
//   x[b, T - 1] = xs[b, Tt - 1]
// Thread (c, y) owns the 16-byte column c of rows j0 + y, j0 + y + ny, ... of its block's row range: the template operands stay
// in registers, pos rows come from the L2 (every segment reads the same ones), the stores are whole 16-byte columns of a row.
__global__ __launch_bounds__(256) void k_stem_fill(const f32x4* __restrict__ xs, const f32x4* __restrict__ tr,
                                                   const f32x4* __restrict__ pos, f32x4* __restrict__ x,
                                                   const int* __restrict__ flag, int T, int Tt, int d4, int rows_per_block) {
  if (*flag == 0) return;
  const int b = blockIdx.y;
  const int j0 = blockIdx.x * rows_per_block, j1 = min(j0 + rows_per_block, T);
  const int ny = blockDim.y;
  const f32x4* xsb = xs + (long)b * Tt * d4;
  f32x4* xb = x + (long)b * T * d4;
  for (int c = threadIdx.x; c < d4; c += blockDim.x) {
    // rows copied from the compact stem
    for (int j = j0 + threadIdx.y; j < j1; j += ny) {
      if (j <= Tt - 3) xb[(long)j * d4 + c] = xsb[(long)j * d4 + c];
      else if (j == T - 1) xb[(long)j * d4 + c] = xsb[(long)(Tt - 1) * d4 + c];
    }
    // the shared row under its ~1 400 position rows
    const int a0 = max(j0, Tt - 2), a1 = min(j1, T - 1);
    if (a0 >= a1) continue;
    const f32x4 xt = xsb[(long)(Tt - 2) * d4 + c], rt = tr[(long)b * d4 + c];
#pragma unroll 4
    for (int j = a0 + threadIdx.y; j < a1; j += ny) {
      const f32x4 p = pos[(long)j * d4 + c];
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = __builtin_fmaf(xt[k], rt[k], p[k]);
      xb[(long)j * d4 + c] = v;
    }
  }
}

bool stem_tail_supported(int t_in, int d) {
  // (t_in % 4: the 16-byte loads of the detection; 4 kStemTc: below that there is little to skip; d: one 16-byte column per thread)
  return t_in % 4 == 0 && t_in >= 4 * kStemTc && d % 4 == 0 && d / 4 <= 256;
}

// flag <- 1 iff every row of mel [rows, t_in] is bitwise constant on [kStemTc - 6, t_in)
int launch_stem_detect(const float* mel, int* flag, long rows, int t_in, hipStream_t s) {
  GWW_REQUIRE(mel && flag, "stem_detect: NULL operand");
  GWW_REQUIRE(t_in % 4 == 0 && t_in > kStemTc && (((uintptr_t)mel) & 15) == 0, "stem_detect: t_in=%d or alignment unsupported", t_in);
  GWW_HIP(hipMemsetD32Async((hipDeviceptr_t)flag, 1, 1, s));
  if (rows <= 0) return GWW_OK;
  const int t0 = kStemTc - 6, ta = (t0 + 4) & ~3, q4 = (t_in - ta) / 4;
  const long n_items = rows * q4;
  const long tiles = cdiv(n_items, 256 * DET_U);
  hipLaunchKernelGGL(k_stem_detect, dim3((unsigned)(tiles < 2048 ? tiles : 2048)), dim3(256), 0, s, (const unsigned*)mel, flag,
                     n_items, t_in, t0, ta, q4);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

int launch_stem_fill(const float* xs, const float* tr, const float* pos, float* x, const int* flag, int B, int T, int d,
                     hipStream_t s, int Tt) {
  GWW_REQUIRE(xs && tr && pos && x && flag, "stem_fill: NULL operand");
  GWW_REQUIRE(d % 4 == 0 && d / 4 <= 256 && Tt >= 3 && T > Tt && B <= 65535, "stem_fill: bad shape B=%d T=%d d=%d", B, T, d);
  if (B == 0) return GWW_OK;
  const int d4 = d / 4, ny = 256 / d4 > 0 ? 256 / d4 : 1;
  const int rpb = 60;
  hipLaunchKernelGGL(k_stem_fill, dim3((unsigned)cdiv(T, rpb), (unsigned)B), dim3(d4, ny), 0, s, (const f32x4*)xs,
                     (const f32x4*)tr, (const f32x4*)pos, (f32x4*)x, flag, T, Tt, d4, rpb);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

// x fp32 [B, T, d] <- the residual stream the compact stem describes (k_stem_fill; a no-op where *flag == 0)
extern "C" int gww_stem_fill_f32(const float* xs, const float* tr, const float* pos, const int* flag, float* x, int B, int T, int Tt,
                                 int d, void* stream) {
  GWW_REQUIRE(B >= 0 && ((((uintptr_t)xs) | ((uintptr_t)tr) | ((uintptr_t)pos) | ((uintptr_t)x)) & 15) == 0,
              "gww_stem_fill_f32: B < 0 or operands not 16-byte aligned");
  return gww::launch_stem_fill(xs, tr, pos, x, flag, B, T, d, (hipStream_t)stream, Tt);
}
