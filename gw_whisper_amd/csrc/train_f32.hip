// Kernels of the exact-fp32 DoRA / LoRA training step (encoder_train_f32.hip: gww_encoder_train_forward_f32 / _backward_f32).
// Every contraction runs on v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fmaf chain), every reduction in a fixed
// order: no float atomics, two identical calls give identical bits.
//
//   k_gemm_f32_dx     C [M, N] = A [M, K] W [K, N] with W the STORED [K][N] weight panel (the [out][in] panel of
//                     gemm_f32.hip read un-transposed): the dX GEMMs of the backward, no second set of fp32 panels.
//   k_rowred_f32      partial slabs of C [P, Q] = sum_m P(m, p) Q(m, q), rows m split into fixed slabs: a general fp32
//                     row-reduction (weight-gradient shaped) GEMM; the adapter gradients dB = dy^T u, dA = v^T x use it.
//   k_adapter_uv_f32  u = x A^T, v = (g dy) B  [M, 64] (rank padded to 64 with zeros)
//   k_colsum2_f32     per slab: sum_m dy y and sum_m dy (the magnitude gradient)
//   k_adapter_reduce_f32  sums the slabs in slab order and accumulates into dA / dB / dm
//   element-wise      exact GELU and its derivative, a - b, and the conv stem's dz2 / dz1 / dmel in fp32
#include "common.h"

#include <algorithm>

namespace gww {

namespace {
constexpr int GM = 64, GN = 64, GK = 32, GLD = GK + 1;

__device__ __forceinline__ float gelu_grad_exact(float z) {   // Phi(z) + z phi(z)
  return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}
}  // namespace

// ---------------------------------------------------------------- dX GEMM: C = A W, W [K][N]
// 64 x 64 x 32 tiles, 256 threads = 2 x 2 waves of 32 x 32 (the tiling of k_gemm_f32).  K % 32 == 0, N % 4 == 0.
__global__ __launch_bounds__(256) void k_gemm_f32_dx(const float* __restrict__ A, long lda, const float* __restrict__ W,
                                                     float* __restrict__ C, long ldc, long M, int N, int K, int tiles_n) {
  __shared__ float As[GM][GLD];
  __shared__ float Ws[GN][GLD];   // Ws[n][k]
  const long tm = blockIdx.x / tiles_n;
  const int tn = (int)(blockIdx.x - tm * tiles_n);
  const long m0 = tm * GM;
  const int n0 = tn * GN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      {   // A: 64 rows x 32 k
        const int row = c >> 3, kc = (c & 7) * 4;
        long ar = m0 + row;
        if (ar >= M) ar = M - 1;
        const float4 av = *reinterpret_cast<const float4*>(A + ar * lda + k0 + kc);
        As[row][kc] = av.x; As[row][kc + 1] = av.y; As[row][kc + 2] = av.z; As[row][kc + 3] = av.w;
      }
      {   // W: 32 k rows x 64 n, contiguous along n
        const int kr = c >> 4, nc = (c & 15) * 4;
        int n = n0 + nc;
        if (n > N - 4) n = N - 4;
        const float4 wv = *reinterpret_cast<const float4*>(W + (long)(k0 + kr) * N + n);
        Ws[nc][kr] = wv.x; Ws[nc + 1][kr] = wv.y; Ws[nc + 2][kr] = wv.z; Ws[nc + 3][kr] = wv.w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 4) {
      float af[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = As[wm * 32 + i * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[j] = Ws[wn * 32 + j * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = m0 + wm * 32 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + (lane >> 4) * 4;
      if (m < M && n < N) *reinterpret_cast<float4*>(C + m * ldc + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

int launch_gemm_f32_dx(const float* A, long lda, const float* W, float* C, long ldc, long M, int N, int K,
                       hipStream_t s) {
  GWW_REQUIRE(A && W && C, "gemm_f32_dx: NULL operand");
  GWW_REQUIRE(K > 0 && K % GK == 0 && N > 0 && N % 4 == 0, "gemm_f32_dx: K=%d must be a multiple of %d, N=%d of 4", K, GK,
              N);
  GWW_REQUIRE(lda % 4 == 0 && ldc % 4 == 0 && lda >= K && ldc >= N, "gemm_f32_dx: bad row strides %ld / %ld", lda, ldc);
  GWW_REQUIRE(((((uintptr_t)A) | ((uintptr_t)W) | ((uintptr_t)C)) & 15) == 0, "gemm_f32_dx: operands must be 16-byte aligned");
  if (M <= 0) return GWW_OK;
  const int tiles_n = (int)cdiv(N, GN);
  const long n_tiles = cdiv(M, GM) * tiles_n;
  GWW_REQUIRE(n_tiles < 2147483647L, "gemm_f32_dx: grid too large");
  hipLaunchKernelGGL(k_gemm_f32_dx, dim3((unsigned)n_tiles), dim3(256), 0, s, A, lda, W, C, ldc, M, N, K, tiles_n);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

// ---------------------------------------------------------------- row-reduction GEMM (slabs)
// part[slab][p][q] (p < PP, q < QP: padded to 64) = sum over the rows m of the slab of P[m * ldp + p] Q[m * ldq + q].
// Grid (p tiles x q tiles, slabs); columns past Pn / Qn are clamped on load (their slab entries are never read).
__global__ __launch_bounds__(256) void k_rowred_f32(const float* __restrict__ P, long ldp, int Pn,
                                                    const float* __restrict__ Q, long ldq, int Qn, long M, long rows_per_slab,
                                                    int tiles_q, int PP, int QP, float* __restrict__ part) {
  __shared__ float Ps[64][GLD];   // Ps[p][m]
  __shared__ float Qs[64][GLD];   // Qs[q][m]
  const int tp = blockIdx.x / tiles_q, tq = blockIdx.x - tp * tiles_q;
  const int p0 = tp * 64, q0 = tq * 64;
  const long mb = (long)blockIdx.y * rows_per_slab;
  long me = mb + rows_per_slab;
  if (me > M) me = M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long m0 = mb; m0 < me; m0 += GK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, mr = c >> 4, cc = (c & 15) * 4;
      const long m = m0 + mr;
      float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), qv = pv;
      if (m < me) {
        int pc = p0 + cc, qc = q0 + cc;
        if (pc > Pn - 4) pc = Pn - 4;
        if (qc > Qn - 4) qc = Qn - 4;
        pv = *reinterpret_cast<const float4*>(P + m * ldp + pc);
        qv = *reinterpret_cast<const float4*>(Q + m * ldq + qc);
      }
      Ps[cc][mr] = pv.x; Ps[cc + 1][mr] = pv.y; Ps[cc + 2][mr] = pv.z; Ps[cc + 3][mr] = pv.w;
      Qs[cc][mr] = qv.x; Qs[cc + 1][mr] = qv.y; Qs[cc + 2][mr] = qv.z; Qs[cc + 3][mr] = qv.w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 4) {
      float pf[2], qf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) pf[i] = Ps[wp * 32 + i * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) qf[j] = Qs[wq * 32 + j * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[j], pf[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.y * PP * QP;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = p0 + wp * 32 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = q0 + wq * 32 + j * 16 + (lane >> 4) * 4;
      *reinterpret_cast<float4*>(out + (size_t)p * QP + q) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

// ---------------------------------------------------------------- adapter gradients
// U [M, 64] = x A^T (blockIdx.y == 0) or V [M, 64] = (g dy) B, g = yscale mag / nrm (blockIdx.y == 1); columns >= r are
// zero.  64 rows per workgroup, 4 waves x 16 rows, 4 MFMA column tiles of 16.
__global__ __launch_bounds__(256) void k_adapter_uv_f32(const float* __restrict__ X, long ldx, const float* __restrict__ dY,
                                                        long ldy, const float* __restrict__ A, const float* __restrict__ Bm,
                                                        const float* __restrict__ mag, const float* __restrict__ nrm,
                                                        float yscale, int r, int d_in, int d_out, long M,
                                                        float* __restrict__ U, float* __restrict__ V) {
  __shared__ float Xs[64][GLD];   // Xs[m][k]
  __shared__ float Ws[64][GLD];   // Ws[j][k]
  const bool isV = blockIdx.y == 1;
  const float* src = isV ? dY : X;
  const long ld = isV ? ldy : ldx;
  const int K = isV ? d_out : d_in;
  float* out = isV ? V : U;
  const long m0 = (long)blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, row = c >> 3, kc = (c & 7) * 4;
      long m = m0 + row;
      if (m >= M) m = M - 1;
      const float4 v = *reinterpret_cast<const float4*>(src + m * ld + k0 + kc);
      Xs[row][kc] = v.x; Xs[row][kc + 1] = v.y; Xs[row][kc + 2] = v.z; Xs[row][kc + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = tid + 256 * i, j = c >> 5, kk = c & 31, k = k0 + kk;
      float w = 0.f;
      if (j < r) w = isV ? yscale * (mag[k] / nrm[k]) * Bm[(long)k * r + j] : A[(long)j * d_in + k];
      Ws[j][kk] = w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 4) {
      const float xf = Xs[wave * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ws[j * 16 + (lane & 15)][kk + (lane >> 4)], xf, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  const long m = m0 + wave * 16 + (lane & 15);
  if (m < M) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(out + m * 64 + j * 16 + (lane >> 4) * 4) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  }
}

// per slab and column c < d_out: [sum_m dy y, sum_m dy] -> part[slab][2][d_out]; rows in order within a thread
__global__ __launch_bounds__(256) void k_colsum2_f32(const float* __restrict__ dY, const float* __restrict__ Y, long ldy,
                                                     int d_out, long M, long rows_per_slab, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d_out) return;
  const long mb = (long)blockIdx.y * rows_per_slab;
  long me = mb + rows_per_slab;
  if (me > M) me = M;
  float s = 0.f, t = 0.f;
  for (long m = mb; m < me; ++m) {
    const float g = dY[m * ldy + c];
    s = fmaf(g, Y[m * ldy + c], s);
    t += g;
  }
  float* o = part + (size_t)blockIdx.y * 2 * d_out;
  o[c] = s;
  o[d_out + c] = t;
}

// one thread per output element of dA [r, d_in] | dB [d_out, r] | dm [d_out]: slabs summed in slab order
__global__ __launch_bounds__(256) void k_adapter_reduce_f32(const float* __restrict__ partA, int nsA, int QPA,
                                                            const float* __restrict__ partB, int nsB, int PPB,
                                                            const float* __restrict__ partM, int nsM, int r, int d_in,
                                                            int d_out, const float* __restrict__ bias, float yscale,
                                                            float scaling, const float* __restrict__ mag,
                                                            const float* __restrict__ nrm, float* dA, float* dB, float* dm) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long nA = (long)r * d_in, nB = (long)d_out * r;
  if (i < nA) {   // dA[j][k] = s sum v[., j] x[., k]: slab [64][QPA]
    const int j = (int)(i / d_in), k = (int)(i - (long)j * d_in);
    float acc = 0.f;
    for (int sl = 0; sl < nsA; ++sl) acc += partA[((size_t)sl * 64 + j) * QPA + k];
    dA[i] += scaling * acc;
  } else if (i < nA + nB) {   // dB[c][j] = s yscale g_c sum dy[., c] u[., j]: slab [PPB][64]
    const long e = i - nA;
    const int c = (int)(e / r), j = (int)(e - (long)c * r);
    float acc = 0.f;
    for (int sl = 0; sl < nsB; ++sl) acc += partB[((size_t)sl * PPB + c) * 64 + j];
    dB[e] += scaling * yscale * (mag[c] / nrm[c]) * acc;
  } else if (i < nA + nB + d_out) {   // dm[c] = (sum dy y - b sum dy) / m
    const int c = (int)(i - nA - nB);
    float sy = 0.f, sd = 0.f;
    for (int sl = 0; sl < nsM; ++sl) {
      sy += partM[(size_t)sl * 2 * d_out + c];
      sd += partM[(size_t)sl * 2 * d_out + d_out + c];
    }
    dm[c] += (sy - bias[c] * sd) / mag[c];
  }
}

namespace {
struct AdapterPlanF32 {
  long Mp, rpsA, rpsB, rpsM;
  int nsA, nsB, nsM, PPB, QPA;
  size_t u, v, pa, pb, pm, total;
};
// slab counts: enough workgroups to fill the device (~1024), at least 32 rows per slab
AdapterPlanF32 adapter_plan_f32(long M, int d_in, int d_out) {
  AdapterPlanF32 p{};
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  auto slabs = [&](long tiles, long& rps) {
    long ns = std::max(1L, std::min(1024 / std::max(1L, tiles), cdiv(M, 256)));
    rps = cdiv(cdiv(M, ns), GK) * GK;
    return (int)cdiv(M, rps);
  };
  p.Mp = M;
  p.QPA = (int)cdiv(d_in, 64) * 64;
  p.PPB = (int)cdiv(d_out, 64) * 64;
  p.nsA = slabs(p.QPA / 64, p.rpsA);
  p.nsB = slabs(p.PPB / 64, p.rpsB);
  p.nsM = slabs(cdiv(d_out, 256) * 4, p.rpsM);
  size_t off = 0;
  p.u = off; off += al((size_t)M * 64 * 4);
  p.v = off; off += al((size_t)M * 64 * 4);
  p.pa = off; off += al((size_t)p.nsA * 64 * p.QPA * 4);
  p.pb = off; off += al((size_t)p.nsB * p.PPB * 64 * 4);
  p.pm = off; off += al((size_t)p.nsM * 2 * d_out * 4);
  p.total = off;
  return p;
}
}  // namespace

size_t adapter_grads_f32_scratch_bytes(long M, int d_in, int d_out, int r) {
  if (M <= 0 || d_in <= 0 || d_out <= 0 || r < 1 || r > 64) return 0;
  return adapter_plan_f32(M, d_in, d_out).total;
}

int launch_adapter_grads_f32(const float* X, long ldx, const float* dY, const float* Y, long ldy, const float* bias,
                             float yscale, float scaling, const float* A, const float* Bm, const float* mag,
                             const float* nrm, float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r,
                             hipStream_t s, void* scratch, size_t scratch_bytes) {
  GWW_REQUIRE(X && dY && Y && bias && A && Bm && mag && nrm && dA && dB && dm, "adapter_grads_f32: NULL argument");
  GWW_REQUIRE(r >= 1 && r <= 64, "adapter_grads_f32: rank r=%d is outside 1..64", r);
  GWW_REQUIRE(d_in > 0 && d_out > 0 && d_in % 32 == 0 && d_out % 32 == 0,
              "adapter_grads_f32: d_in=%d and d_out=%d must be positive multiples of 32", d_in, d_out);
  GWW_REQUIRE(M >= 0 && ldx >= d_in && ldy >= d_out && ldx % 4 == 0 && ldy % 4 == 0 &&
                  ((((uintptr_t)X) | ((uintptr_t)dY) | ((uintptr_t)Y)) & 15) == 0,
              "adapter_grads_f32: row strides (ldx=%ld ldy=%ld) must be multiples of 4 >= d_in / d_out and X / dY / Y "
              "16-byte aligned", ldx, ldy);
  GWW_REQUIRE((((uintptr_t)scratch) & 255) == 0, "adapter_grads_f32: scratch must be 256-byte aligned");
  if (M == 0) return GWW_OK;
  const AdapterPlanF32 p = adapter_plan_f32(M, d_in, d_out);
  char* ws = (char*)scratch;
  bool own = false;
  if (!ws || scratch_bytes < p.total) {
    GWW_HIP(hipMallocAsync((void**)&ws, p.total, s));
    own = true;
  }
  float* U = (float*)(ws + p.u);
  float* V = (float*)(ws + p.v);
  float* pa = (float*)(ws + p.pa);
  float* pb = (float*)(ws + p.pb);
  float* pm = (float*)(ws + p.pm);
  hipLaunchKernelGGL(k_adapter_uv_f32, dim3((unsigned)cdiv(M, 64), 2), dim3(256), 0, s, X, ldx, dY, ldy, A, Bm, mag, nrm,
                     yscale, r, d_in, d_out, M, U, V);
  // dA slabs: P = V [M, 64] (p = rank), Q = x [M, d_in];  dB slabs: P = dy [M, d_out], Q = U [M, 64] (q = rank)
  hipLaunchKernelGGL(k_rowred_f32, dim3((unsigned)(p.QPA / 64), (unsigned)p.nsA), dim3(256), 0, s, V, 64L, 64, X, ldx, d_in,
                     M, p.rpsA, p.QPA / 64, 64, p.QPA, pa);
  hipLaunchKernelGGL(k_rowred_f32, dim3((unsigned)(p.PPB / 64), (unsigned)p.nsB), dim3(256), 0, s, dY, ldy, d_out, U, 64L,
                     64, M, p.rpsB, 1, p.PPB, 64, pb);
  hipLaunchKernelGGL(k_colsum2_f32, dim3((unsigned)cdiv(d_out, 256), (unsigned)p.nsM), dim3(256), 0, s, dY, Y, ldy, d_out,
                     M, p.rpsM, pm);
  const long n_out = (long)r * (d_in + d_out) + d_out;
  hipLaunchKernelGGL(k_adapter_reduce_f32, dim3((unsigned)cdiv(n_out, 256)), dim3(256), 0, s, pa, p.nsA, p.QPA, pb, p.nsB,
                     p.PPB, pm, p.nsM, r, d_in, d_out, bias, yscale, scaling, mag, nrm, dA, dB, dm);
  GWW_LAUNCH_CHECK();
  if (own) GWW_HIP(hipFreeAsync(ws, s));
  return GWW_OK;
}

// ---------------------------------------------------------------- element-wise
// out = gelu(z) (g == NULL) or out = g * gelu'(z); exact erf forms.  n % 4 == 0; out may alias g.
__global__ __launch_bounds__(256) void k_gelu_f32(const float* __restrict__ z, const float* g, float* out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 zv = reinterpret_cast<const f32x4*>(z)[i];
    f32x4 o;
    if (g) {
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = gv[j] * gelu_grad_exact(zv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = gelu_erf(zv[j]);
    }
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

int launch_gelu_f32(const float* z, const float* g, float* out, long n, hipStream_t s) {
  GWW_REQUIRE(z && out && n % 4 == 0, "gelu_f32: NULL operand or n %% 4 != 0");
  if (n == 0) return GWW_OK;
  const long blocks = std::min(cdiv(n / 4, 256), 16384L);
  hipLaunchKernelGGL(k_gelu_f32, dim3((unsigned)blocks), dim3(256), 0, s, z, g, out, n / 4);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

__global__ __launch_bounds__(256) void k_sub_f32(const float* __restrict__ a, const float* __restrict__ b,
                                                 float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
    reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(a)[i] - reinterpret_cast<const f32x4*>(b)[i];
}

int launch_sub_f32(const float* a, const float* b, float* out, long n, hipStream_t s) {
  GWW_REQUIRE(a && b && out && n % 4 == 0, "sub_f32: NULL operand or n %% 4 != 0");
  if (n == 0) return GWW_OK;
  const long blocks = std::min(cdiv(n / 4, 256), 16384L);
  hipLaunchKernelGGL(k_sub_f32, dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n / 4);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

// conv stem backward in fp32 (the bf16 forms and their index maps: train_ops.hip)
// dz2[b (T+1) + t] = t < T ? dx0[b T + t] * gelu'(z2[b (T+1) + t]) : 0          (4 columns per thread)
__global__ __launch_bounds__(256) void k_stem_dz2_f32(const float* __restrict__ dx0, const float* __restrict__ z2,
                                                      float* __restrict__ out, int T, int d4, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long row = i / d4;
    const int c4 = (int)(i - row * d4);
    const long b = row / (T + 1);
    const int t = (int)(row - b * (T + 1));
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (t < T) {
      const f32x4 g = reinterpret_cast<const f32x4*>(dx0)[(b * T + t) * d4 + c4];
      const f32x4 z = reinterpret_cast<const f32x4*>(z2)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = g[j] * gelu_grad_exact(z[j]);
    }
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// col [B (T+1), 3 d] -> dz1 rows b (Tin + 2) + t1 (t1 >= Tin zeroed), times gelu'(z1).  In place (out == z1) ok.
__global__ __launch_bounds__(256) void k_stem_dz1_f32(const float* __restrict__ col, const float* z1, float* out, int T,
                                                      int Tin, int d, long n4) {
  const int d4 = d / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long row = i / d4;
    const int c4 = (int)(i - row * d4);
    const long b = row / (Tin + 2);
    const int t1 = (int)(row - b * (Tin + 2));
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (t1 < Tin) {
      const int p = t1 + 1;
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      auto add = [&](long crow, int tap) { g += *reinterpret_cast<const f32x4*>(col + (crow * 3 + tap) * d + 4 * c4); };
      if (p & 1) {
        add(b * (T + 1) + (p - 1) / 2, 1);
      } else {
        if (p / 2 < T) add(b * (T + 1) + p / 2, 0);
        add(b * (T + 1) + p / 2 - 1, 2);
      }
      const f32x4 z = reinterpret_cast<const f32x4*>(z1)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = g[j] * gelu_grad_exact(z[j]);
    }
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// dmel[b, c, tau] = sum_k col1[b, tau + 1 - k][k C + c], 0 <= tau + 1 - k < Tin; 64 time steps per workgroup via LDS
__global__ __launch_bounds__(256) void k_stem_dmel_f32(const float* __restrict__ col1, float* __restrict__ dmel, int Tin,
                                                       int C, int Kp) {
  constexpr int TT = 64;
  extern __shared__ float smf[];   // [TT + 2][3 C + 1]
  const int ld = 3 * C + 1;
  const int b = blockIdx.y, tau0 = blockIdx.x * TT;
  for (int i = threadIdx.x; i < (TT + 2) * 3 * C; i += 256) {
    const int rl = i / (3 * C), k = i - rl * 3 * C;
    const int t1 = tau0 - 1 + rl;
    smf[rl * ld + k] = (t1 >= 0 && t1 < Tin) ? col1[((long)b * (Tin + 2) + t1) * Kp + k] : 0.f;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < C * TT; o += 256) {
    const int c = o / TT, tl = o - c * TT;
    const int tau = tau0 + tl;
    if (tau >= Tin) continue;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) v += smf[(tl + 2 - k) * ld + k * C + c];
    dmel[((long)b * C + c) * Tin + tau] = v;
  }
}

int launch_stem_dz2_f32(const float* dx0, const float* z2, float* out, int B, int T, int d, hipStream_t s) {
  GWW_REQUIRE(d % 4 == 0, "stem_dz2_f32: d must be a multiple of 4");
  const long n4 = (long)B * (T + 1) * (d / 4);
  const long blocks = std::min(cdiv(n4, 256), 16384L);
  hipLaunchKernelGGL(k_stem_dz2_f32, dim3((unsigned)blocks), dim3(256), 0, s, dx0, z2, out, T, d / 4, n4);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

int launch_stem_dz1_f32(const float* col, const float* z1, float* out, int B, int T, int Tin, int d, hipStream_t s) {
  GWW_REQUIRE(d % 4 == 0 && Tin == 2 * T, "stem_dz1_f32: bad shape");
  const long n4 = (long)B * (Tin + 2) * (d / 4);
  const long blocks = std::min(cdiv(n4, 256), 16384L);
  hipLaunchKernelGGL(k_stem_dz1_f32, dim3((unsigned)blocks), dim3(256), 0, s, col, z1, out, T, Tin, d, n4);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

int launch_stem_dmel_f32(const float* col1, float* dmel, int B, int Tin, int C, int Kp, hipStream_t s) {
  GWW_REQUIRE(3 * C <= Kp, "stem_dmel_f32: col1 row shorter than 3 taps");
  const size_t lds = (size_t)(64 + 2) * (3 * C + 1) * 4;
  hipLaunchKernelGGL(k_stem_dmel_f32, dim3((unsigned)cdiv(Tin, 64), (unsigned)B), dim3(256), lds, s, col1, dmel, Tin, C, Kp);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" size_t gww_adapter_grads_f32_scratch_bytes(long M, int d_in, int d_out, int r) {
  return adapter_grads_f32_scratch_bytes(M, d_in, d_out, r);
}

extern "C" int gww_adapter_grads_f32(const float* X, long ldx, const float* dY, const float* Y, long ldy,
                                     const float* bias_st, float yscale, float scaling, const float* A, const float* B,
                                     const float* mag, const float* nrm, float* dA, float* dB, float* dm, long M,
                                     int d_in, int d_out, int r, void* scratch, size_t scratch_bytes, void* stream) {
  return launch_adapter_grads_f32(X, ldx, dY, Y, ldy, bias_st, yscale, scaling, A, B, mag, nrm, dA, dB, dm, M, d_in, d_out,
                                  r, (hipStream_t)stream, scratch, scratch_bytes);
}
