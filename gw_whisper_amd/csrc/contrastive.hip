// Kernels of the MLGWSC-1 training program (harness/run_mlgwsc_train.py, gw_whisper_amd/mlgwsc_train.py), fp32 (the tail
// backward's two scalar sums are formed in fp64) and without float atomics: every reduction runs in a fixed order, so two
// identical calls give identical bits.
//
//   InfoNCE (ContrastivePretrainer._info_nce, MLGWSC-1/train.py:410-424) forward + backward;
//   the backward of the Q-adapter's tail (pool -> affine -> FiLM, qscan._AdapterTail) as one gather pass;
//   batch assembly X = noise[i] + snr * wave[j] of BinaryGWDataset / PretrainDataset (train.py:262-273, 342-351).
#include <math.h>

#include "common.h"

namespace gww {
namespace {

// ---------------------------------------------------------------------------------------------------------
// InfoNCE.  Z = [normalize(z1); normalize(z2)] [2B, P], S = Z Z^T / tau with the diagonal excluded, pair(r) = r +- B:
//     L = (1/B) sum_r [ LSE_{j != r} S_rj - S_{r,pair(r)} ]
// which is the reference's mean_i[-log(pos_i / den1_i) - log(pos_i / den2_i)].  The LSE subtracts the row maximum: where
// the reference's fp32 exp(S) is finite the result is the same; for tau below about 1 / 88.7 exp(1 / tau) overflows fp32
// and the reference returns inf / NaN, these kernels stay finite.
// One workgroup (4 waves) per row r; wave w takes the columns j = w, w + 4, ...; a lane holds P / 64 elements of n_r
// (P <= 1024) and the dot product n_r . n_j is a butterfly wave sum.  The four waves' partials combine in wave order.
constexpr int NCE_PMAX = 1024, NCE_PL = NCE_PMAX / kWave, NCE_WAVES = 4;
constexpr float NCE_EPS = 1e-12f;   // F.normalize's eps

__global__ __launch_bounds__(64) void k_nce_normalize(const float* __restrict__ z1, const float* __restrict__ z2, int B,
                                                      int P, float* __restrict__ n, float* __restrict__ nrm) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* z = r < B ? z1 + (long)r * P : z2 + (long)(r - B) * P;
  float s = 0.f;
  for (int p = lane; p < P; p += kWave) s += z[p] * z[p];
  const float nr = sqrtf(wave_sum(s));
  const float den = fmaxf(nr, NCE_EPS);
  for (int p = lane; p < P; p += kWave) n[(long)r * P + p] = z[p] / den;
  if (lane == 0) nrm[r] = nr;
}

__device__ __forceinline__ void nce_load_row(const float* __restrict__ row, int P, int lane, float (&v)[NCE_PL]) {
#pragma unroll
  for (int k = 0; k < NCE_PL; ++k) {
    const int p = lane + kWave * k;
    v[k] = p < P ? row[p] : 0.f;
  }
}

__device__ __forceinline__ float nce_dot(const float (&a)[NCE_PL], const float (&b)[NCE_PL]) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < NCE_PL; ++k) d += a[k] * b[k];
  return wave_sum(d);
}

// lse[r] = LSE_{j != r} S_rj, term[r] = lse[r] - S_{r,pair(r)}.  Two passes over the row: the maximum M (at the smallest
// column j* attaining it) and S_{r,pair}, then rest = sum_{j != r, j*} exp(S_rj - M); lse = M + log1p(rest) and
// term = (M - S_{r,pair}) + log1p(rest) keep their relative accuracy when the pair dominates the row (a small loss).
__global__ __launch_bounds__(256) void k_nce_lse(const float* __restrict__ n, int B, int P, float tau,
                                                 float* __restrict__ lse, float* __restrict__ term) {
  __shared__ float sm[NCE_WAVES], sl[NCE_WAVES], sp[NCE_WAVES];
  __shared__ int sj[NCE_WAVES];
  const int r = blockIdx.x, N = 2 * B, lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  const int pair = r < B ? r + B : r - B;
  float nr[NCE_PL], nj[NCE_PL];
  nce_load_row(n + (long)r * P, P, lane, nr);
  float m = -INFINITY, spos = 0.f;
  int jm = N;
  for (int j = w; j < N; j += NCE_WAVES) {
    if (j == r) continue;
    nce_load_row(n + (long)j * P, P, lane, nj);
    const float s = nce_dot(nr, nj) / tau;
    if (j == pair) spos = s;
    if (s > m) { m = s; jm = j; }
  }
  if (lane == 0) { sm[w] = m; sj[w] = jm; sp[w] = spos; }
  __syncthreads();
  float M = sm[0];
  int jstar = sj[0];
  for (int i = 1; i < NCE_WAVES; ++i)
    if (sm[i] > M || (sm[i] == M && sj[i] < jstar)) { M = sm[i]; jstar = sj[i]; }
  float rest = 0.f;
  for (int j = w; j < N; j += NCE_WAVES) {
    if (j == r || j == jstar) continue;
    nce_load_row(n + (long)j * P, P, lane, nj);
    rest += expf(nce_dot(nr, nj) / tau - M);
  }
  if (lane == 0) sl[w] = rest;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float lp = log1pf(((sl[0] + sl[1]) + sl[2]) + sl[3]);
    lse[r] = M + lp;
    term[r] = (M - sp[pair % NCE_WAVES]) + lp;
  }
}

// fixed-order block sum of x[0..n) (256 threads); the result is valid in thread 0
__device__ float block_sum_256(const float* __restrict__ x, long n, float* red) {
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) s += x[i];
  s = wave_sum(s);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void k_nce_loss(const float* __restrict__ term, int B, float* __restrict__ loss) {
  __shared__ float red[4];
  const float s = block_sum_256(term, 2L * B, red);
  if (threadIdx.x == 0) loss[0] = s / (float)B;
}

// dz_r from dn_r = (g / (B tau)) sum_{j != r} [softmax_rj + softmax_jr - 2 [j == pair(r)]] n_j  (S symmetric), then back
// through n = z / max(|z|, eps): (dn - n (n . dn)) / |z| where |z| >= eps, dn / eps below it.
__global__ __launch_bounds__(256) void k_nce_backward(const float* __restrict__ n, const float* __restrict__ nrm,
                                                      const float* __restrict__ lse, const float* __restrict__ term,
                                                      int B, int P, float tau,
                                                      const float* __restrict__ dloss, float* __restrict__ dz1,
                                                      float* __restrict__ dz2) {
  __shared__ float part[NCE_WAVES][NCE_PMAX];
  __shared__ float red[NCE_WAVES];
  const int r = blockIdx.x, N = 2 * B, lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  const int pair = r < B ? r + B : r - B;
  float nr[NCE_PL], nj[NCE_PL], acc[NCE_PL];
  nce_load_row(n + (long)r * P, P, lane, nr);
#pragma unroll
  for (int k = 0; k < NCE_PL; ++k) acc[k] = 0.f;
  const float lse_r = lse[r];
  // the pair's coefficient softmax_r,pair - 1 + softmax_pair,r - 1 = expm1(-term[r]) + expm1(-term[pair]) (S symmetric):
  // no cancellation when the pair dominates its rows
  const float c_pair = expm1f(-term[r]) + expm1f(-term[pair]);
  for (int j = w; j < N; j += NCE_WAVES) {
    if (j == r) continue;
    nce_load_row(n + (long)j * P, P, lane, nj);
    const float s = nce_dot(nr, nj) / tau;
    const float c = j == pair ? c_pair : expf(s - lse_r) + expf(s - lse[j]);
#pragma unroll
    for (int k = 0; k < NCE_PL; ++k) acc[k] += c * nj[k];
  }
#pragma unroll
  for (int k = 0; k < NCE_PL; ++k) {
    const int p = lane + kWave * k;
    if (p < P) part[w][p] = acc[k];
  }
  __syncthreads();
  const float g = dloss[0] / ((float)B * tau);
  float dn[NCE_PMAX / 256], nv[NCE_PMAX / 256], dot = 0.f;
#pragma unroll
  for (int k = 0; k < NCE_PMAX / 256; ++k) {
    const int p = threadIdx.x + 256 * k;
    dn[k] = nv[k] = 0.f;
    if (p < P) {
      dn[k] = g * (((part[0][p] + part[1][p]) + part[2][p]) + part[3][p]);
      nv[k] = n[(long)r * P + p];
      dot += nv[k] * dn[k];
    }
  }
  dot = wave_sum(dot);
  if (lane == 0) red[w] = dot;
  __syncthreads();
  dot = ((red[0] + red[1]) + red[2]) + red[3];
  const float nz = nrm[r];
  float* dz = r < B ? dz1 + (long)r * P : dz2 + (long)(r - B) * P;
#pragma unroll
  for (int k = 0; k < NCE_PMAX / 256; ++k) {
    const int p = threadIdx.x + 256 * k;
    if (p < P) dz[p] = nz >= NCE_EPS ? (dn[k] - nv[k] * dot) / nz : dn[k] / NCE_EPS;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Backward of the adapter tail  out = (scale * pool(y) + bias) * gamma_i + beta_i  (forward: k_qadapter_tail, qscan.hip).
// PyTorch's adaptive pooling: output row f covers input rows [floor(f Hin / F), ceil((f + 1) Hin / F)), column t covers
// [floor(t Win / T), ceil((t + 1) Win / T)).  Input row h is covered by the output rows [floor(h F / Hin),
// ceil((h + 1) F / Hin)) and likewise for columns, so d_y is a GATHER: one workgroup per (input row h, window b) reduces
// every covering g row along T first (staged in LDS, weighted by 1 / column count), then along F, in a fixed order.
// The workgroup that owns output row f (h == its first input row) also recomputes pool(y) for that row from the y rows
// it covers and forms its partial sums of g * pool(y) and g; a second single-workgroup launch adds the partials in
// (b, h) order and writes d_scale = gamma_i S_gp, d_bias = gamma_i S_g, d_gamma_i = scale S_gp + bias S_g, d_beta_i = S_g.
// The two scalar sums run over B F T (7.7 M at 32 windows) terms of both signs: the recomputed pool(y) and the sums are
// fp64 -- in fp32 their rounding leaves an error near 1e-7 sqrt(B F T) |g p|, which exceeds 1e-5 of a sum that cancels.
constexpr int TB_MAXW = 4096, TB_MAXT = 4096, TB_WL = TB_MAXW / 256;

__global__ __launch_bounds__(256) void k_tail_backward(const float* __restrict__ g, long g_bstride, const float* __restrict__ y,
                                                       int Hin, int Win, int F, int Tn, const float* __restrict__ scale,
                                                       const float* __restrict__ gamma_i, float* __restrict__ dy,
                                                       double* __restrict__ part) {
  __shared__ float gs[TB_MAXT];
  __shared__ double rp[TB_MAXW];
  __shared__ double red[2][4];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int f0 = (int)(((long)h * F) / Hin);
  const int f1 = min(F, (int)((((long)h + 1) * F + Hin - 1) / Hin));
  const float* yb = y + (long)b * Hin * Win;
  float acc[TB_WL];
#pragma unroll
  for (int k = 0; k < TB_WL; ++k) acc[k] = 0.f;
  double sgp = 0.0, sg = 0.0;
  for (int f = f0; f < f1; ++f) {
    const int r0 = (int)(((long)f * Hin) / F), r1 = (int)((((long)f + 1) * Hin + F - 1) / F);
    const bool owner = r0 == h;                   // uniform over the workgroup
    const float* gr = g + (long)b * g_bstride + (long)f * Tn;
    __syncthreads();                              // the previous row's readers of gs / rp are done
    if (owner)
      for (int c = tid; c < Win; c += 256) {
        double s = 0.0;
        for (int r = r0; r < r1; ++r) s += (double)yb[(long)r * Win + c];
        rp[c] = s;
      }
    __syncthreads();
    const float inv_r = 1.0f / (float)(r1 - r0);
    for (int t = tid; t < Tn; t += 256) {
      const int k0 = (int)(((long)t * Win) / Tn), k1 = (int)((((long)t + 1) * Win + Tn - 1) / Tn);
      const float gv = gr[t];
      gs[t] = gv / (float)(k1 - k0);
      if (owner) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) s += rp[k];
        sgp += (double)gv * (s / (double)((r1 - r0) * (k1 - k0)));
        sg += (double)gv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TB_WL; ++k) {
      const int wc = tid + 256 * k;
      if (wc < Win) {
        const int t0 = (int)(((long)wc * Tn) / Win);
        const int t1 = min(Tn, (int)((((long)wc + 1) * Tn + Win - 1) / Win));
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += gs[t];
        acc[k] += s * inv_r;
      }
    }
  }
  const float a = scale[0] * gamma_i[0];
  float* dyr = dy + ((long)b * Hin + h) * Win;
#pragma unroll
  for (int k = 0; k < TB_WL; ++k) {
    const int wc = tid + 256 * k;
    if (wc < Win) dyr[wc] = acc[k] * a;
  }
  sgp = wave_sum_f64(sgp);
  sg = wave_sum_f64(sg);
  if (tid % kWave == 0) { red[0][tid / kWave] = sgp; red[1][tid / kWave] = sg; }
  __syncthreads();
  if (tid == 0) {
    double* o = part + 2 * ((long)b * Hin + h);
    o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

__global__ __launch_bounds__(256) void k_tail_backward_reduce(const double* __restrict__ part, long n,
                                                              const float* __restrict__ scale, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma_i, float* __restrict__ d_scale,
                                                              float* __restrict__ d_bias, float* __restrict__ d_gamma_i,
                                                              float* __restrict__ d_beta_i) {
  __shared__ double red[2][4];
  double sgp = 0.0, sg = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) { sgp += part[2 * i]; sg += part[2 * i + 1]; }
  sgp = wave_sum_f64(sgp);
  sg = wave_sum_f64(sg);
  if (threadIdx.x % kWave == 0) { red[0][threadIdx.x / kWave] = sgp; red[1][threadIdx.x / kWave] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double Sgp = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const double Sg = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const double gam = gamma_i[0];
    d_scale[0] = (float)(gam * Sgp);
    d_bias[0] = (float)(gam * Sg);
    d_gamma_i[0] = (float)((double)scale[0] * Sgp + (double)bias[0] * Sg);
    d_beta_i[0] = (float)Sg;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Batch assembly: out[r, :] = noise[in_r, :] + snr_r * wave[iw_r, :] (iw_r < 0: noise only), the reference's torch
// expression `noises[i] + snr * waveforms[i]` bit for bit -- an fp32 product rounded, then an fp32 sum rounded.  The _rn
// intrinsics lower to plain fmul / fadd, which the library's -ffp-contract=fast still fuses into one v_fma: an empty asm
// on the product keeps the two roundings.  A row whose index lies outside its array is written NaN instead of being read
// out of bounds (the host wrapper validates the plan first).
__global__ __launch_bounds__(256) void k_assemble(const float* __restrict__ noise, long n_noise, const float* __restrict__ wave,
                                                  long n_wave, long L, const int* __restrict__ idx_noise,
                                                  const int* __restrict__ idx_wave, const float* __restrict__ snr,
                                                  float* __restrict__ out) {
  const int r = blockIdx.y;
  const long in = idx_noise[r], iw = idx_wave[r];
  const bool bad = in < 0 || in >= n_noise || iw >= n_wave || (iw >= 0 && wave == nullptr);
  const float s = snr[r];
  float* o = out + (long)r * L;
  const float* nz = noise + (bad ? 0 : in) * L;
  const float* wv = (bad || iw < 0) ? nullptr : wave + iw * L;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < L; e += (long)gridDim.x * 256) {
    if (bad) o[e] = __int_as_float(0x7fc00000);
    else if (wv == nullptr) o[e] = nz[e];
    else {
      float p = __fmul_rn(s, wv[e]);
      asm volatile("" : "+v"(p));   // the rounded product must reach the add: no fusion into one v_fma
      o[e] = __fadd_rn(nz[e], p);
    }
  }
}

}  // namespace
}  // namespace gww

extern "C" int gww_info_nce_forward_f32(const float* z1, const float* z2, int B, int P, float tau, float* n, float* nrm,
                                        float* lse, float* term, float* loss, void* stream) {
  GWW_REQUIRE(z1 && z2 && n && nrm && lse && term && loss, "gww_info_nce_forward_f32: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= (1 << 28) && P >= 1 && P <= gww::NCE_PMAX,
              "gww_info_nce_forward_f32: need B >= 1 and 1 <= P <= %d (B=%d P=%d)", gww::NCE_PMAX, B, P);
  GWW_REQUIRE(tau > 0.f && isfinite(tau), "gww_info_nce_forward_f32: temperature must be positive and finite");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gww::k_nce_normalize, dim3((unsigned)(2 * B)), dim3(64), 0, s, z1, z2, B, P, n, nrm);
  hipLaunchKernelGGL(gww::k_nce_lse, dim3((unsigned)(2 * B)), dim3(256), 0, s, n, B, P, tau, lse, term);
  hipLaunchKernelGGL(gww::k_nce_loss, dim3(1), dim3(256), 0, s, term, B, loss);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_info_nce_backward_f32(const float* n, const float* nrm, const float* lse, const float* term, int B,
                                         int P, float tau, const float* dloss, float* dz1, float* dz2, void* stream) {
  GWW_REQUIRE(n && nrm && lse && term && dloss && dz1 && dz2, "gww_info_nce_backward_f32: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= (1 << 28) && P >= 1 && P <= gww::NCE_PMAX,
              "gww_info_nce_backward_f32: need B >= 1 and 1 <= P <= %d (B=%d P=%d)", gww::NCE_PMAX, B, P);
  GWW_REQUIRE(tau > 0.f && isfinite(tau), "gww_info_nce_backward_f32: temperature must be positive and finite");
  hipLaunchKernelGGL(gww::k_nce_backward, dim3((unsigned)(2 * B)), dim3(256), 0, (hipStream_t)stream, n, nrm, lse, term, B,
                     P, tau, dloss, dz1, dz2);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_qadapter_tail_backward_workspace_bytes(int B, int Hin) {
  if (B < 0 || Hin < 0) return 0;
  return (size_t)2 * sizeof(double) * (size_t)B * (size_t)Hin;
}

extern "C" int gww_qadapter_tail_backward_f32(const float* g, long g_batch_stride, const float* y, int B, int Hin, int Win,
                                              int F, int T, const float* scale, const float* bias, const float* gamma_i,
                                              float* d_y, void* ws, size_t ws_bytes, float* d_scale, float* d_bias,
                                              float* d_gamma_i, float* d_beta_i, void* stream) {
  GWW_REQUIRE(g && y && scale && bias && gamma_i && d_y && ws && d_scale && d_bias && d_gamma_i && d_beta_i,
              "gww_qadapter_tail_backward_f32: NULL argument");
  GWW_REQUIRE(B >= 1 && Hin > 0 && Win > 0 && Win <= gww::TB_MAXW && F > 0 && T > 0 && T <= gww::TB_MAXT,
              "gww_qadapter_tail_backward_f32: bad shape B=%d Hin=%d Win=%d F=%d T=%d", B, Hin, Win, F, T);
  GWW_REQUIRE(g_batch_stride >= (long)F * T, "gww_qadapter_tail_backward_f32: g batch stride %ld < F * T", g_batch_stride);
  if (ws_bytes < gww_qadapter_tail_backward_workspace_bytes(B, Hin))
    return ::gww::fail(GWW_ERR_WORKSPACE, "gww_qadapter_tail_backward_f32: workspace %zu bytes < required %zu", ws_bytes,
                gww_qadapter_tail_backward_workspace_bytes(B, Hin));
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  for (int b0 = 0; b0 < B; b0 += 65535) {   // gridDim.y limit
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    hipLaunchKernelGGL(gww::k_tail_backward, dim3((unsigned)Hin, (unsigned)nb), dim3(256), 0, s, g + (long)b0 * g_batch_stride,
                       g_batch_stride, y + (long)b0 * Hin * Win, Hin, Win, F, T, scale, gamma_i, d_y + (long)b0 * Hin * Win,
                       part + 2L * b0 * Hin);
  }
  hipLaunchKernelGGL(gww::k_tail_backward_reduce, dim3(1), dim3(256), 0, s, part, (long)B * Hin, scale, bias, gamma_i, d_scale,
                     d_bias, d_gamma_i, d_beta_i);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_assemble_batch_f32(const float* noise, long n_noise, const float* wave, long n_wave, long row_len,
                                      const int* idx_noise, const int* idx_wave, const float* snr, int R, float* out,
                                      void* stream) {
  GWW_REQUIRE(noise && idx_noise && idx_wave && snr && out, "gww_assemble_batch_f32: NULL argument");
  GWW_REQUIRE(R >= 1 && R <= 65535 && row_len >= 1 && n_noise >= 1 && n_wave >= 0,
              "gww_assemble_batch_f32: bad shape R=%d row_len=%ld n_noise=%ld n_wave=%ld", R, row_len, n_noise, n_wave);
  const long blocks = (row_len + 255) / 256;
  hipLaunchKernelGGL(gww::k_assemble, dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)R), dim3(256), 0,
                     (hipStream_t)stream, noise, n_noise, wave, n_wave, row_len, idx_noise, idx_wave, snr, out);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
