// The CNN decoder head of the two-detector model (models.TwoChannelLIGOBinaryClassifierCNN): per sample x [2, d] ->
// Conv1d(2 -> 64) -> ReLU -> Conv1d(64 -> 128) -> ReLU -> Conv1d(128 -> 256) -> ReLU -> mean over d -> Linear(256, C),
// every conv k = 3, pad = 1.  Exact fp32 like the MLP heads (head_chain.h): the two wide convolutions are implicit GEMMs
// on v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain), no float atomics, every reduction in a fixed order.
//
// Forward, ONE launch (k_cnn_fwd): a workgroup of 512 threads owns one sample and walks its length in tiles of 64
// positions.  Per tile: x with a halo of 3 -> c1 (VALU, K = 6) in LDS as [position][channel] -> c2 = W2 * im2col(c1) in
// LDS -> c3 = W3 * im2col(c2) in the accumulators, whose ReLU feeds the per-lane running sums of the mean.  The im2col is
// never formed: the B operand of a k step is a read of the LDS tile shifted by the tap.  The weights are read in torch's
// own layout [Cout][Cin * 3] (16 bytes per lane per 16 k), so k runs (channel, tap) as it does there.  Nothing of a sample
// depends on the batch: a sample's logits have the same bits alone, at any index and in any batch.
//
// Backward: plain launches over the saved post-ReLU activations --
//   k_cnn_bwd_head   pooled rows, dpool = dlogits W4 / d, dz3 = (h3 > 0) ? dpool : 0
//   k_cnn_pack_t     the mirrored, transposed weights of the two data-gradient convolutions (per call: per weight version)
//   k_cnn_conv_t     dz_in = (h_in > 0) ? conv(Wm, dz_out) : 0 -- the forward's implicit GEMM, once per layer
//   k_cnn_dx         dx = conv^T(W1, dz1), VALU
//   k_cnn_wgrad      dW[co][ci][tap] and db[co] over a slice of the batch: a 64 x 64 x 3 tile per workgroup, partials
//   k_cnn_wgrad1     the same for conv1 (384 + 64 numbers), VALU
//   k_cnn_lin_grads  dW4, db4 from the pooled rows
//   k_cnn_reduce     the partials summed slice after slice
#include "head_chain.h"

namespace gww {

constexpr int CN_C1 = 64, CN_C2 = 128, CN_C3 = 256;
constexpr int CN_T = 64;                    // positions of one forward tile (conv3's)
constexpr int CN_THREADS = 512;
constexpr int CN_WAVES = CN_THREADS / 64;
constexpr int CN_S1 = CN_C1 + 4;            // LDS row pitch of the c1 tile (floats): rows stay 16-byte aligned
constexpr int CN_S2 = CN_C2 + 4;
constexpr int CN_R2 = 80;                   // c2 rows: positions t0 - 1 .. t0 + 78 (five MFMA tiles; conv3 reads rows 0 .. 65)
constexpr int CN_R1 = CN_R2 + 2;            // c1 rows: positions t0 - 2 .. t0 + 79
constexpr int CN_RX = CN_R1 + 2;            // x rows:  positions t0 - 3 .. t0 + 80
constexpr int CN_FWD_LDS = (CN_R1 * CN_S1 + CN_R2 * CN_S2 + 2 * CN_RX + 2 * CN_C3) * 4;   // the pooled row is fp64
constexpr int CN_SPLIT_MAX = 32;            // batch slices of the weight-gradient partials

// acc[ct][pt] += W[co0 + 16 ct + i][(ci, tap)] * in[row 16 pt + j + tap][ci]   (i, j the 16 x 16 tile; k = 3 ci + tap runs
// 0 .. 3 CIN - 1 in 16-blocks, the order inside a block permuted as in head_chain.h: MFMA u of a block takes k = 4 q + u
// from lane group q).  `in`: the LDS tile [row][channel] of pitch S whose row 0 is the position in FRONT of the first
// output position; W: [.][3 CIN] in global memory, 16-byte aligned.  The A fragments of the next block are requested
// before the MFMAs of this one.
template <int CIN, int NCT, int NPT>
__device__ __forceinline__ void conv_tile(const float* in, int S, const float* __restrict__ W, int co0,
                                          f32x4 (&acc)[NCT][NPT]) {
  constexpr int K = 3 * CIN;
  static_assert(CIN % 16 == 0, "a pass of three 16-blocks covers 16 channels");
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  int off[3][4];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = 16 * s + 4 * q + u;
      off[s][u] = (kk % 3) * S + kk / 3;
    }
  const float* wp = W + (long)(co0 + c) * K + 4 * q;
  const float* ip = in + c * S;
  float4 a[NCT], an[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    a[ct] = *reinterpret_cast<const float4*>(wp + (long)ct * 16 * K);
    an[ct] = a[ct];
  }
#pragma unroll 1
  for (int it = 0; it < CIN / 16; ++it) {   // (unrolled further, the LDS reads of every pass are hoisted and spill)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int kn = it * 48 + 16 * (s + 1);
      if (kn < K) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) an[ct] = *reinterpret_cast<const float4*>(wp + (long)ct * 16 * K + kn);
      }
      float bv[NPT][4];
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[pt][u] = ip[pt * 16 * S + it * 16 + off[s][u]];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct].x, bv[pt][0], acc[ct][pt], 0, 0, 0);
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct].y, bv[pt][1], acc[ct][pt], 0, 0, 0);
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct].z, bv[pt][2], acc[ct][pt], 0, 0, 0);
          acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct].w, bv[pt][3], acc[ct][pt], 0, 0, 0);
        }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) a[ct] = an[ct];
    }
  }
}

struct CnnParams {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid = B.  saved (SAVE): [B, 64 + 128 + 256, d], the three post-ReLU activations of a sample one after the other.
template <bool SAVE>
__global__ __launch_bounds__(CN_THREADS) void k_cnn_fwd(const float* __restrict__ x, CnnParams P, int d, int C,
                                                        float* __restrict__ logits, float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float sm_cnn[];
  float* const c1 = sm_cnn;                       // [CN_R1][CN_S1]
  float* const c2 = c1 + CN_R1 * CN_S1;           // [CN_R2][CN_S2]
  float* const xs = c2 + CN_R2 * CN_S2;           // [2][CN_RX]
  double* const pool = reinterpret_cast<double*>(xs + 2 * CN_RX);   // [256] (an even number of floats in front of it)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
  const long b = blockIdx.x;
  const float* xb = x + b * 2 * d;
  float* const s1 = SAVE ? saved + b * (long)(CN_C1 + CN_C2 + CN_C3) * d : nullptr;
  float* const s2 = SAVE ? s1 + (long)CN_C1 * d : nullptr;
  float* const s3 = SAVE ? s2 + (long)CN_C2 * d : nullptr;

  // conv1: this thread's output channel is the same in every pass (512 % 64 == 0)
  const int co1 = tid & 63;
  float w1r[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) w1r[i] = P.w1[co1 * 6 + i];
  const float b1r = P.b1[co1];
  // conv2: wave w owns channels 16 w .. + 15 on five position tiles; conv3: channels 32 w .. + 31 on four
  const float4 b2r = *reinterpret_cast<const float4*>(P.b2 + 16 * wave + 4 * q);
  float4 b3r[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) b3r[ct] = *reinterpret_cast<const float4*>(P.b3 + 32 * wave + 16 * ct + 4 * q);
  // the mean and the Linear behind it are summed in fp64 and rounded once: a logit is a sum of d * 256 terms, and in fp32
  // the order of that sum alone would cost more than everything in front of it
  double psum[2][4] = {{0., 0., 0., 0.}, {0., 0., 0., 0.}};

  for (int t0 = 0; t0 < d; t0 += CN_T) {
    for (int i = tid; i < 2 * CN_RX; i += CN_THREADS) {
      const int ci = i / CN_RX, r = i - ci * CN_RX, pos = t0 - 3 + r;
      xs[i] = (pos >= 0 && pos < d) ? xb[ci * d + pos] : 0.f;
    }
    __syncthreads();
    for (int row = tid >> 6; row < CN_R1; row += CN_THREADS / 64) {
      const int pos = t0 - 2 + row;
      float v = 0.f;                               // the next layer's zero padding, and what lies beyond the sample
      if (pos >= 0 && pos < d) {
        float acc = b1r;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
          for (int t = 0; t < 3; ++t) acc = fmaf(w1r[ci * 3 + t], xs[ci * CN_RX + row + t], acc);
        v = fmaxf(acc, 0.f);
      }
      c1[row * CN_S1 + co1] = v;
    }
    __syncthreads();
    if (SAVE) {
      for (int i = tid; i < CN_C1 * CN_T; i += CN_THREADS) {
        const int co = i >> 6, p = i & 63;
        s1[(long)co * d + t0 + p] = c1[(p + 2) * CN_S1 + co];
      }
    }
    {
      f32x4 acc[1][5];
#pragma unroll
      for (int pt = 0; pt < 5; ++pt) acc[0][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      conv_tile<CN_C1, 1, 5>(c1, CN_S1, P.w2, 16 * wave, acc);
      const int co = 16 * wave + 4 * q;
#pragma unroll
      for (int pt = 0; pt < 5; ++pt) {
        const int row = 16 * pt + c, pos = t0 - 1 + row;
        const bool in = pos >= 0 && pos < d;
        const float4 v = {in ? fmaxf(acc[0][pt][0] + b2r.x, 0.f) : 0.f, in ? fmaxf(acc[0][pt][1] + b2r.y, 0.f) : 0.f,
                          in ? fmaxf(acc[0][pt][2] + b2r.z, 0.f) : 0.f, in ? fmaxf(acc[0][pt][3] + b2r.w, 0.f) : 0.f};
        *reinterpret_cast<float4*>(c2 + row * CN_S2 + co) = v;
        if (SAVE && row >= 1 && row <= CN_T) {       // the tile's own 64 positions (all inside the sample)
          s2[(long)(co + 0) * d + pos] = v.x;
          s2[(long)(co + 1) * d + pos] = v.y;
          s2[(long)(co + 2) * d + pos] = v.z;
          s2[(long)(co + 3) * d + pos] = v.w;
        }
      }
    }
    __syncthreads();
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      conv_tile<CN_C2, 2, 4>(c2, CN_S2, P.w3, 32 * wave, acc);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int co = 32 * wave + 16 * ct + 4 * q;
        const float bb[4] = {b3r[ct].x, b3r[ct].y, b3r[ct].z, b3r[ct].w};
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = fmaxf(acc[ct][pt][r] + bb[r], 0.f);
            psum[ct][r] += (double)v;
            if (SAVE) s3[(long)(co + r) * d + t0 + 16 * pt + c] = v;
          }
      }
    }
    // (the next tile's first barrier stands between this tile's readers of c1 / c2 and their next writers)
  }
  // the mean: the 16 lanes of a channel in a fixed butterfly, one division by d
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = psum[ct][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
      if (c == 0) pool[32 * wave + 16 * ct + 4 * q + r] = v / (double)d;
    }
  __syncthreads();
  for (int cls = wave; cls < C; cls += CN_WAVES) {
    double v = 0.;
#pragma unroll
    for (int i = 0; i < 4; ++i) v = fma((double)P.w4[cls * CN_C3 + lane + 64 * i], pool[lane + 64 * i], v);
    v = wave_sum_f64(v);
    if (lane == 0) logits[b * C + cls] = (float)(v + (double)P.b4[cls]);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// grid (B, 4), 256 threads: wave w of block y owns channels 64 y + 16 w .. + 15 of sample b.
__global__ __launch_bounds__(256) void k_cnn_bwd_head(const float* __restrict__ saved, const float* __restrict__ dlogits,
                                                      const float* __restrict__ w4, int d, int C, float* __restrict__ dz3,
                                                      float* __restrict__ pooled) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.x;
  const float* h3 = saved + (b * (CN_C1 + CN_C2 + CN_C3) + CN_C1 + CN_C2) * d;
  for (int i = 0; i < 16; ++i) {
    const int co = 64 * blockIdx.y + 16 * wave + i;
    float g = 0.f;
    for (int cls = 0; cls < C; ++cls) g = fmaf(dlogits[b * C + cls], w4[cls * CN_C3 + co], g);
    g = g / (float)d;
    float s = 0.f;
    for (int p = lane; p < d; p += 64) {
      const float h = h3[(long)co * d + p];
      s += h;
      dz3[(b * CN_C3 + co) * d + p] = h > 0.f ? g : 0.f;
    }
    s = wave_sum(s);
    if (lane == 0) pooled[b * CN_C3 + co] = s / (float)d;
  }
}

// wm3 [128][256 * 3], wm2 [64][128 * 3]: wm[ci][3 co + t] = w[co][ci][2 - t]
__global__ __launch_bounds__(256) void k_cnn_pack_t(const float* __restrict__ w2, const float* __restrict__ w3,
                                                    float* __restrict__ wm2, float* __restrict__ wm3) {
  const int n3 = CN_C2 * CN_C3 * 3, n2 = CN_C1 * CN_C2 * 3;
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n3) {
    const int ci = i / (CN_C3 * 3), r = i - ci * (CN_C3 * 3), co = r / 3, t = r - 3 * co;
    wm3[i] = w3[(co * CN_C2 + ci) * 3 + 2 - t];
  } else if (i < n3 + n2) {
    i -= n3;
    const int ci = i / (CN_C2 * 3), r = i - ci * (CN_C2 * 3), co = r / 3, t = r - 3 * co;
    wm2[i] = w2[(co * CN_C1 + ci) * 3 + 2 - t];
  }
}

// dzi[b][co][p] = (h[b][co][p] > 0) ? sum_(ci, t) wm[co][3 ci + t] dzo[b][ci][p + t - 1] : 0.  grid (d / 64, B); dzo / dzi /
// h: [., CIN or COUT, d] with the sample strides given (h lives inside `saved`).  LDS: 66 rows of CIN + 4.
template <int CIN, int COUT>
__global__ __launch_bounds__(CN_THREADS) void k_cnn_conv_t(const float* __restrict__ dzo, const float* __restrict__ wm,
                                                           const float* __restrict__ h, long h_stride,
                                                           float* __restrict__ dzi, int d) {
  extern __shared__ __attribute__((aligned(16))) float sm_cnn[];
  constexpr int S = CIN + 4, ROWS = CN_T + 2;
  constexpr int NWC = COUT / 16, NWP = CN_WAVES / NWC, NPT = 4 / NWP;
  static_assert(NWC * NWP == CN_WAVES && NPT * NWP == 4, "eight waves tile COUT x 64");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
  const long b = blockIdx.y;
  const int t0 = blockIdx.x * CN_T;
  const float* src = dzo + b * CIN * d;
  for (int i = tid; i < CIN * ROWS; i += CN_THREADS) {
    const int ch = i / ROWS, r = i - ch * ROWS, pos = t0 - 1 + r;
    sm_cnn[r * S + ch] = (pos >= 0 && pos < d) ? src[(long)ch * d + pos] : 0.f;
  }
  __syncthreads();
  const int wc = wave % NWC, wp = wave / NWC;
  f32x4 acc[1][NPT];
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) acc[0][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
  conv_tile<CIN, 1, NPT>(sm_cnn + wp * NPT * 16 * S, S, wm, 16 * wc, acc);
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = 16 * wc + 4 * q + r, pos = t0 + (wp * NPT + pt) * 16 + c;
      const float hv = h[b * h_stride + (long)co * d + pos];
      dzi[(b * COUT + co) * d + pos] = hv > 0.f ? acc[0][pt][r] : 0.f;
    }
}

// dx[b][ci][p] = sum_(co, t) w1[co][ci][t] dz1[b][co][p + 1 - t].  grid (d / 128, B), 128 threads.
__global__ __launch_bounds__(128) void k_cnn_dx(const float* __restrict__ dz1, const float* __restrict__ w1, int d,
                                                float* __restrict__ dx) {
  __shared__ float w[CN_C1 * 6];
  for (int i = threadIdx.x; i < CN_C1 * 6; i += 128) w[i] = w1[i];
  __syncthreads();
  const long b = blockIdx.y;
  const int p = blockIdx.x * 128 + threadIdx.x;
  const float* z = dz1 + b * CN_C1 * d;
  float a0 = 0.f, a1 = 0.f;
  for (int co = 0; co < CN_C1; ++co) {
    const float* zr = z + (long)co * d;
    const float zl = p > 0 ? zr[p - 1] : 0.f, zc = zr[p], zn = p + 1 < d ? zr[p + 1] : 0.f;
    // tap t meets dz1 at p + 1 - t
    a0 = fmaf(w[co * 6 + 0], zn, a0);
    a0 = fmaf(w[co * 6 + 1], zc, a0);
    a0 = fmaf(w[co * 6 + 2], zl, a0);
    a1 = fmaf(w[co * 6 + 3], zn, a1);
    a1 = fmaf(w[co * 6 + 4], zc, a1);
    a1 = fmaf(w[co * 6 + 5], zl, a1);
  }
  dx[(b * 2 + 0) * d + p] = a0;
  dx[(b * 2 + 1) * d + p] = a1;
}

// Partial dW[co][ci][t] = sum over the slice's samples and all p of dz[b][co][p] hin[b][ci][p + t - 1], and db[co] = the sum
// of dz.  grid (CO / 64 * CI / 64, slices), 256 threads: wave w owns rows co0 + 16 w .. + 15 of the 64 x 64 x 3 tile.  Lane
// (c, q) feeds dz[co0 + 16 w + c][p0 + 4 q .. + 3] (16 bytes) and hin[ci0 + 16 t + c][p0 + 4 q - 1 .. + 4]; the positions
// of a 16-block never leave the sample (d % 16 == 0), and its two outer neighbours are zero at the sample's ends.
// part: [slice][CO * CI * 3], partb: [slice][CO].
template <int CO, int CI>
__global__ __launch_bounds__(256) void k_cnn_wgrad(const float* __restrict__ dz, const float* __restrict__ hin, long h_stride,
                                                   int B, int d, int per_slice, float* __restrict__ part,
                                                   float* __restrict__ partb) {
  constexpr int TK = CI / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int tn = blockIdx.x / TK, tk = blockIdx.x - tn * TK;
  const int co = tn * 64 + wave * 16, ci0 = tk * 64;
  const int b_lo = blockIdx.y * per_slice, b_hi = min(B, b_lo + per_slice);
  f32x4 acc[4][3], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[t][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = tk == 0;
  for (int b = b_lo; b < b_hi; ++b) {
    const float* zr = dz + ((long)b * CO + co + c) * d + 4 * q;
    const float* hr = hin + (long)b * h_stride + (long)(ci0 + c) * d + 4 * q;
    for (int p0 = 0; p0 < d; p0 += 16) {
      const float4 a = *reinterpret_cast<const float4*>(zr + p0);
      const int pl = p0 + 4 * q - 1, pr = p0 + 4 * q + 4;
      float4 f[4];
      float l[4], r[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float* hp = hr + (long)t * 16 * d + p0;
        f[t] = *reinterpret_cast<const float4*>(hp);
        l[t] = pl >= 0 ? hp[-1] : 0.f;
        r[t] = pr < d ? hp[4] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, l[t], acc[t][0], 0, 0, 0);
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f[t].x, acc[t][0], 0, 0, 0);
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f[t].y, acc[t][0], 0, 0, 0);
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, f[t].z, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, f[t].x, acc[t][1], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f[t].y, acc[t][1], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f[t].z, acc[t][1], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, f[t].w, acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, f[t].y, acc[t][2], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f[t].z, acc[t][2], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f[t].w, acc[t][2], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, r[t], acc[t][2], 0, 0, 0);
      }
      if (do_bias) {
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, 1.f, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, 1.f, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, 1.f, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, 1.f, accb, 0, 0, 0);
      }
    }
  }
  float* po = part + (long)blockIdx.y * CO * CI * 3;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = co + 4 * q + r;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < 3; ++k) po[((long)n * CI + ci0 + 16 * t + c) * 3 + k] = acc[t][k][r];
    if (do_bias && c == 0) partb[(long)blockIdx.y * CO + n] = accb[r];
  }
}

// conv1's partials: grid (64, slices), 256 threads; part [slice][64 * 6], partb [slice][64]
__global__ __launch_bounds__(256) void k_cnn_wgrad1(const float* __restrict__ dz1, const float* __restrict__ x, int B, int d,
                                                    int per_slice, float* __restrict__ part, float* __restrict__ partb) {
  __shared__ float red[7][256];
  const int co = blockIdx.x, tid = threadIdx.x;
  const int b_lo = blockIdx.y * per_slice, b_hi = min(B, b_lo + per_slice);
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = b_lo; b < b_hi; ++b) {
    const float* z = dz1 + ((long)b * CN_C1 + co) * d;
    const float* xb = x + (long)b * 2 * d;
    for (int p = tid; p < d; p += 256) {
      const float a = z[p];
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) {
        const float* xr = xb + ci * d;
        acc[ci * 3 + 0] = fmaf(a, p > 0 ? xr[p - 1] : 0.f, acc[ci * 3 + 0]);
        acc[ci * 3 + 1] = fmaf(a, xr[p], acc[ci * 3 + 1]);
        acc[ci * 3 + 2] = fmaf(a, p + 1 < d ? xr[p + 1] : 0.f, acc[ci * 3 + 2]);
      }
      acc[6] += a;
    }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) red[i][tid] = acc[i];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int i = 0; i < 7; ++i) red[i][tid] += red[i][tid + o];
    __syncthreads();
  }
  if (tid < 6) part[(long)blockIdx.y * CN_C1 * 6 + co * 6 + tid] = red[tid][0];
  if (tid == 6) partb[(long)blockIdx.y * CN_C1 + co] = red[6][0];
}

// dW4[cls][co] = sum_b dlogits[b][cls] pooled[b][co], db4[cls] = sum_b dlogits[b][cls]; grid C, 256 threads
__global__ __launch_bounds__(256) void k_cnn_lin_grads(const float* __restrict__ dlogits, const float* __restrict__ pooled,
                                                       int B, int C, float* __restrict__ dw4, float* __restrict__ db4) {
  const int cls = blockIdx.x, co = threadIdx.x;
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < B; ++b) {
    const float g = dlogits[(long)b * C + cls];
    s = fmaf(g, pooled[(long)b * CN_C3 + co], s);
    sb += g;
  }
  dw4[cls * CN_C3 + co] = s;
  if (co == 0) db4[cls] = sb;
}

struct CnnReduce {
  const float* part[6];
  float* out[6];
  int n[6], first[7];   // elements of a segment; its first thread
};
__global__ __launch_bounds__(256) void k_cnn_reduce(CnnReduce R, int slices) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R.first[6]) return;
  int s = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (i >= R.first[k]) s = k;
  const int e = i - R.first[s];
  float v = 0.f;
  for (int k = 0; k < slices; ++k) v += R.part[s][(long)k * R.n[s] + e];
  R.out[s][e] = v;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static bool cnn_d_supported(int d) { return d == 128 || d == 384 || d == 512 || d == 768 || d == 1024 || d == 1280; }
static int cnn_check_shape(const char* who, int B, int d, int C) {
  GWW_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d must be 1..65535", who, B);
  GWW_REQUIRE(cnn_d_supported(d), "%s: d=%d must be an encoder width (128, 384, 512, 768, 1024, 1280)", who, d);
  GWW_REQUIRE(C >= 1 && C <= CH_CMAX, "%s: C=%d must be 1..%d", who, C, CH_CMAX);
  return GWW_OK;
}
static int cnn_slices(int B, int* per_slice) {
  const int per = (int)cdiv(B, CN_SPLIT_MAX);
  *per_slice = per;
  return (int)cdiv(B, per);
}
// the backward's workspace, in floats
struct CnnWs {
  size_t dz3, dz2, dz1, pooled, wm3, wm2, p3, pb3, p2, pb2, p1, pb1, total;
  CnnWs(int B, int d) {
    int per;
    const size_t S = (size_t)cnn_slices(B, &per), Bd = (size_t)B * d;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += (n + 3) / 4 * 4; return at; };   // 16-byte aligned pieces
    dz3 = take(Bd * CN_C3);
    dz2 = take(Bd * CN_C2);
    dz1 = take(Bd * CN_C1);
    pooled = take((size_t)B * CN_C3);
    wm3 = take((size_t)CN_C2 * CN_C3 * 3);
    wm2 = take((size_t)CN_C1 * CN_C2 * 3);
    p3 = take(S * CN_C3 * CN_C2 * 3);
    pb3 = take(S * CN_C3);
    p2 = take(S * CN_C2 * CN_C1 * 3);
    pb2 = take(S * CN_C2);
    p1 = take(S * CN_C1 * 6);
    pb1 = take(S * CN_C1);
    total = o;
  }
};

}  // namespace gww

using namespace gww;

extern "C" size_t gww_cnn_head_saved_bytes(int B, int d) {
  if (B < 1 || !cnn_d_supported(d)) return 0;
  return (size_t)B * (CN_C1 + CN_C2 + CN_C3) * d * sizeof(float);
}

extern "C" size_t gww_cnn_head_workspace_bytes(int B, int d, int C) {
  if (B < 1 || B > 65535 || !cnn_d_supported(d) || C < 1 || C > CH_CMAX) return 0;
  return CnnWs(B, d).total * sizeof(float);
}

extern "C" int gww_cnn_head_forward_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                        const float* w3, const float* b3, const float* w4, const float* b4, int B, int d,
                                        int C, float* logits, float* saved, void* stream) {
  GWW_TRY(cnn_check_shape("gww_cnn_head_forward_f32", B, d, C));
  GWW_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && w4 && b4, "gww_cnn_head_forward_f32: NULL input");
  GWW_REQUIRE(logits, "gww_cnn_head_forward_f32: NULL output");
  GWW_REQUIRE(aligned16({w2, w3, b2, b3}), "gww_cnn_head_forward_f32: w2, w3, b2, b3 must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const CnnParams P{w1, b1, w2, b2, w3, b3, w4, b4};
  if (saved) {
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cnn_fwd<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CN_FWD_LDS));
    hipLaunchKernelGGL(k_cnn_fwd<true>, dim3((unsigned)B), dim3(CN_THREADS), CN_FWD_LDS, s, x, P, d, C, logits, saved);
  } else {
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cnn_fwd<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CN_FWD_LDS));
    hipLaunchKernelGGL(k_cnn_fwd<false>, dim3((unsigned)B), dim3(CN_THREADS), CN_FWD_LDS, s, x, P, d, C, logits, saved);
  }
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_cnn_head_backward_f32(const float* x, const float* saved, const float* dlogits, const float* w1,
                                         const float* w2, const float* w3, const float* w4, int B, int d, int C, float* dx,
                                         float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, float* dw4,
                                         float* db4, void* workspace, size_t workspace_bytes, void* stream) {
  GWW_TRY(cnn_check_shape("gww_cnn_head_backward_f32", B, d, C));
  GWW_REQUIRE(x && saved && dlogits && w1 && w2 && w3 && w4, "gww_cnn_head_backward_f32: NULL input");
  GWW_REQUIRE(dx && dw1 && db1 && dw2 && db2 && dw3 && db3 && dw4 && db4, "gww_cnn_head_backward_f32: NULL output");
  GWW_REQUIRE(workspace, "gww_cnn_head_backward_f32: NULL workspace");
  GWW_REQUIRE(aligned16({saved, workspace}), "gww_cnn_head_backward_f32: saved and workspace must be 16-byte aligned");
  const CnnWs L(B, d);
  if (workspace_bytes < L.total * sizeof(float))
    return fail(GWW_ERR_WORKSPACE, "gww_cnn_head_backward_f32: workspace of %zu bytes, gww_cnn_head_workspace_bytes says %zu",
                workspace_bytes, L.total * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const long hs = (long)(CN_C1 + CN_C2 + CN_C3) * d;          // sample stride inside `saved`
  const float *h1 = saved, *h2 = saved + (long)CN_C1 * d;
  int per;
  const int slices = cnn_slices(B, &per);

  hipLaunchKernelGGL(k_cnn_bwd_head, dim3((unsigned)B, 4), dim3(256), 0, s, saved, dlogits, w4, d, C, ws + L.dz3, ws + L.pooled);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cnn_pack_t, dim3((unsigned)cdiv((CN_C2 * CN_C3 + CN_C1 * CN_C2) * 3, 256)), dim3(256), 0, s, w2, w3,
                     ws + L.wm2, ws + L.wm3);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cnn_lin_grads, dim3((unsigned)C), dim3(256), 0, s, dlogits, (const float*)(ws + L.pooled), B, C, dw4, db4);
  GWW_LAUNCH_CHECK();
  constexpr int lds3 = (CN_T + 2) * (CN_C3 + 4) * 4, lds2 = (CN_T + 2) * (CN_C2 + 4) * 4;
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cnn_conv_t<CN_C3, CN_C2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds3));
  hipLaunchKernelGGL((k_cnn_conv_t<CN_C3, CN_C2>), dim3((unsigned)(d / CN_T), (unsigned)B), dim3(CN_THREADS), lds3, s,
                     (const float*)(ws + L.dz3), (const float*)(ws + L.wm3), h2, hs, ws + L.dz2, d);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_cnn_conv_t<CN_C2, CN_C1>), dim3((unsigned)(d / CN_T), (unsigned)B), dim3(CN_THREADS), lds2, s,
                     (const float*)(ws + L.dz2), (const float*)(ws + L.wm2), h1, hs, ws + L.dz1, d);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cnn_dx, dim3((unsigned)(d / 128), (unsigned)B), dim3(128), 0, s, (const float*)(ws + L.dz1), w1, d, dx);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_cnn_wgrad<CN_C3, CN_C2>), dim3((CN_C3 / 64) * (CN_C2 / 64), (unsigned)slices), dim3(256), 0, s,
                     (const float*)(ws + L.dz3), h2, hs, B, d, per, ws + L.p3, ws + L.pb3);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_cnn_wgrad<CN_C2, CN_C1>), dim3((CN_C2 / 64) * (CN_C1 / 64), (unsigned)slices), dim3(256), 0, s,
                     (const float*)(ws + L.dz2), h1, hs, B, d, per, ws + L.p2, ws + L.pb2);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cnn_wgrad1, dim3(CN_C1, (unsigned)slices), dim3(256), 0, s, (const float*)(ws + L.dz1), x, B, d, per,
                     ws + L.p1, ws + L.pb1);
  GWW_LAUNCH_CHECK();
  CnnReduce R;
  const float* parts[6] = {ws + L.p3, ws + L.pb3, ws + L.p2, ws + L.pb2, ws + L.p1, ws + L.pb1};
  float* outs[6] = {dw3, db3, dw2, db2, dw1, db1};
  const int ns[6] = {CN_C3 * CN_C2 * 3, CN_C3, CN_C2 * CN_C1 * 3, CN_C2, CN_C1 * 6, CN_C1};
  R.first[0] = 0;
  for (int i = 0; i < 6; ++i) {
    R.part[i] = parts[i];
    R.out[i] = outs[i];
    R.n[i] = ns[i];
    R.first[i + 1] = R.first[i] + ns[i];
  }
  hipLaunchKernelGGL(k_cnn_reduce, dim3((unsigned)cdiv(R.first[6], 256)), dim3(256), 0, s, R, slices);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
