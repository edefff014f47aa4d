// Shared device/host helpers for libgww (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/gww.h"
#include <vector>

namespace gww {

// ---- error plumbing -------------------------------------------------------
extern thread_local char g_err[512];
int fail(int code, const char* fmt, ...);

#define GWW_HIP(expr)                                                                 \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return ::gww::fail(GWW_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                         __FILE__, __LINE__);                                         \
  } while (0)

#define GWW_LAUNCH_CHECK() GWW_HIP(hipGetLastError())

#define GWW_REQUIRE(cond, ...)                       \
  do {                                               \
    if (!(cond)) return ::gww::fail(GWW_ERR_ARG, __VA_ARGS__); \
  } while (0)

#define GWW_TRY(expr)          \
  do {                         \
    int _rc = (expr);          \
    if (_rc != GWW_OK) return _rc; \
  } while (0)

// ---- vector types ---------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int kWave = 64;

// fp32 -> bf16 bits, round to nearest even.  A plain cast lowers to
// v_cvt_pk_bf16_f32 on gfx950 and keeps NaNs NaN.
__device__ __forceinline__ unsigned short f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float bf2f(unsigned short u) {
  return __builtin_bit_cast(float, ((unsigned int)u) << 16);
}
// two values -> one dword, ONE v_cvt_pk_bf16_f32 (the scalar casts above cost three instructions per pair)
__device__ __forceinline__ unsigned int pack2bf(float lo, float hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2_t));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// fp64 sum over a workgroup of 256 threads in a fixed LDS tree: of one partial per thread, or of v[0 .. n) with thread t
// taking t, t + 256, ... first.  All 256 threads call it, once per kernel; its barriers order what came before it.
__device__ __forceinline__ double block_sum_f64(double s) {
  __shared__ double part[256];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  return part[0];
}
__device__ __forceinline__ double block_sum_f64(const float* __restrict__ v, int n) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  return block_sum_f64(s);
}

// exact (erf) GELU, nn.functional.gelu default
__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// GELU for the bf16 path: erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7, far below the
// bf16 rounding of the result); ~12 VALU ops instead of ocml erff's ~40.
__device__ __forceinline__ float gelu_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  p *= t;
  const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);
  const float erf_abs = fmaf(-p, e, 1.0f);              // erf(|x|/sqrt2)
  const float h = 0.5f * x;
  return fmaf(h, copysignf(erf_abs, x), h);             // 0.5 x (1 + erf(x/sqrt2))
}

// x * sigmoid(p(x)), p an odd quintic fitted to the erf GELU (the fused block's form, mlp_fused.hip): |err| <= 2.6e-5,
// 7 plain VALU operations + v_exp_f32 + v_rcp_f32 -- a third cheaper than the erf polynomial of gelu_fast
__device__ __forceinline__ float gelu_sig4(float x) {
  const float s = fminf(x * x, 64.0f);
  float q = fmaf(s, 0.0010148164f, -0.1067791331f);
  q = fmaf(s, q, -2.3011178f);
  const float e = __builtin_amdgcn_exp2f(x * q);
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}
// ... and its sigmoid factor alone: gelu_sig4(x) == x * gelu_sig4_sigma(x), operation for operation (the compact conv stem
// stores x and this factor apart, gemm_v4.hip: EPI_CONV2T).  Keep the two in step.
__device__ __forceinline__ float gelu_sig4_sigma(float x) {
  const float s = fminf(x * x, 64.0f);
  float q = fmaf(s, 0.0010148164f, -0.1067791331f);
  q = fmaf(s, q, -2.3011178f);
  const float e = __builtin_amdgcn_exp2f(x * q);
  return __builtin_amdgcn_rcpf(1.0f + e);
}

// gelu'(z) = Phi(z) + z phi(z) for the training backward: the same 7.1.26 polynomial, whose exp(-z^2 / 2) factor is
// sqrt(2 pi) phi(z) -- 16 VALU operations (two transcendental) where ocml erff + expf take about sixty
__device__ __forceinline__ float dgelu_fast(float z) {
  const float az = fabsf(z) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  p *= t;
  const float e = __builtin_amdgcn_exp2f(-az * az * 1.44269504088896340736f);   // exp(-z^2 / 2)
  const float erf_abs = fmaf(-p, e, 1.0f);
  return fmaf(0.5f, copysignf(erf_abs, z), fmaf(z * 0.3989422804f, e, 0.5f));
}

static inline long cdiv(long a, long b) { return (a + b - 1) / b; }
// p is a multiple of a (a power of two)
static inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// The residual stream [M, 384] fp32 in ACCUMULATOR order (k_mlp_fused, FwdPlan::x_native): between two fused blocks of the
// inference forward x_next has one reader, the same wave and lane that wrote it, so each 32-row wave slice keeps its own
// 48 KiB but holds them as the 48 accumulator pieces of the wave, 1 KiB each: piece 4 t + cc is the 16 bytes every lane
// (r, hh) owns of columns 32 t + 8 cc + 4 hh .. + 3, lane after lane.  Byte offset of element (g, c); a row past M is
// clamped to M - 1 first, as the kernel's dead lanes are.  The buffer spans whole 128-row panels: x_native_bytes.
__host__ __device__ inline size_t x_native_offset(long g, int c, long M) {
  if (g > M - 1) g = M - 1;
  const size_t slice = (size_t)(g >> 5);   // 4 P + w: panel P = g >> 7, wave w = (g >> 5) & 3
  const int r = (int)(g & 31), t = c >> 5, cc = (c >> 3) & 3, hh = (c >> 2) & 1, k = c & 3;
  return (slice * 48 + (size_t)(4 * t + cc)) * 1024 + (size_t)(r + 32 * hh) * 16 + (size_t)(4 * k);
}
inline size_t x_native_bytes(long M) { return (size_t)cdiv(M, 128) * 128 * 384 * 4; }

// Byte offsets of consecutive buffers carved out of one allocation, each on a 256-byte boundary
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
  size_t total() const { return off; }
};

// Laboratory switches (kernel variants kept for A/B measurements, tuning aids): read from the environment ONLY in the
// -DGWW_LAB build that tools/ use (make LAB=1 -> libgww_lab.so).  In the product library they are compile-time constants:
// no environment variable changes what libgww.so computes or launches (no global mutable state).
#ifdef GWW_LAB
long lab_int(const char* name, long dflt);   // encoder.hip
#else
constexpr long lab_int(const char*, long dflt) { return dflt; }
#endif

// the constant tail of a padded log-mel (stem_tail.hip): the stem on the first kStemTc frames, kStemTt compact tokens
constexpr int kStemTc = 256, kStemTt = kStemTc / 2;

// Batched weight preparation (elementwise.hip::k_prep_batch): the small row-wise kernels of a weight update collected
// into one launch per dependency phase.  Ops of ONE batch must not read each other's outputs; flush() between phases.
enum { PREP_PACK16, PREP_PACK32, PREP_COPY, PREP_LNFOLD, PREP_TRANSPOSE, PREP_DORA };
constexpr int kPrepMaxOps = 40;      // 40 x 80-byte descriptors + the prefix table stay below the 4-KiB kernel-argument limit
constexpr int kPrepMaxRank = 1024;   // LoRA rank the DoRA body stages in LDS
struct PrepOp {
  const void *a, *b, *c, *d;   // inputs   (kind-specific, see PrepBatch's methods)
  void *o0, *o1, *o2;          // outputs
  int kind, blocks, N, K;      // workgroups of the op; rows; columns (Kpad / d_in / Cn)
  int C, taps;                 // pack: input channels, taps; DoRA: C = rank
  float scale;
  int pad_;
};
struct PrepArgs {
  int n;
  int first[kPrepMaxOps + 1];  // first workgroup of op i; first[n] = grid size
  PrepOp op[kPrepMaxOps];
};
struct PrepBatch {
  std::vector<PrepArgs> args;  // nothing is launched before flush(): a full table opens the next one
  hipStream_t s;
  explicit PrepBatch(hipStream_t st) : s(st) {}
  int add(const PrepOp& o);
  int flush();                 // one launch per table, in order
  int pack(const float* w, void* out, int out_bf16, int N, int C, int taps, int Kpad, float scale);
  int copy(const float* in, float* out, int n, float scale);
  int ln_fold(const float* w, const float* g, const float* bl, const float* bias, float scale, int N, int K, void* wp,
              float* u, float* cb);
  int transpose(const void* in, void* out, int R, int Cn);
  int dora(const float* w0, const float* a, const float* b, const float* m, float scaling, int d_out, int d_in, int r,
           float* w_eff, float* norm_out);
};

// GEMM epilogues
enum : int {
  EPI_BIAS = 0,        // C = acc + bias                    (bf16 / f32 store)
  EPI_GELU = 1,        // C = gelu(acc + bias)
  EPI_RESID = 2,       // C(f32) = resid + acc + bias       (may alias resid)
  EPI_CONV2 = 3,       // conv2: gelu(acc+bias) + pos[t], rows remapped (see gemm_bf16.hip)
};

}  // namespace gww

#include "launchers.h"   // every cross-file launcher, declared once
