// The exact-fp32 MLP chain behind the glitch head (classify.hip), the detection head (detect.hip) and the binary heads
// (binary_head.hip): d_in -> hidden widths -> C, ReLU (and optionally dropout) between the layers.  Every contraction is a
// v_mfma_f32_16x16x4_f32 chain (bit for bit a k-ordered fmaf chain), no float atomics, every reduction in a fixed order: two
// identical calls give identical bits, and two heads give identical bits wherever their layers agree.  One workgroup of
// CH_THREADS owns CH_ROWS rows and walks the whole chain with the activations in two LDS buffers that take turns; the
// weights stream from L2.  A head is a Chain<...>, a forward kernel with its tail and its C entries; the backward kernels,
// the loss mean, the operand check and the two host paths (chain_launch_fwd, chain_backward) are here, once.
#pragma once
#include <initializer_list>

#include "common.h"

namespace gww {

constexpr int CH_ROWS = 16;                 // rows of one workgroup (one MFMA tile)
constexpr int CH_THREADS = 512;             // 8 waves
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_PAD = 4;                   // LDS row padding (floats): rows stay 16-byte aligned
constexpr int CH_CMAX = 64;

// A chain of L linear layers with the hidden widths H...; the last layer's width is C at run time, CH_CMAX for sizing.
// Forward, layer i reads LDS buffer i & 1 (x is loaded into buffer 0) and writes buffer (i + 1) & 1; backward, layer i's dz
// lives in buffer (L - 1 - i) & 1.  fwd_w / bwd_w: the widest row a buffer holds on that walk (x not counted).
template <int... H>
struct Chain {
  static constexpr int L = sizeof...(H) + 1;
  static constexpr int out(int i, int C = CH_CMAX) {
    constexpr int h[] = {H...};
    return i < L - 1 ? h[i] : C;
  }
  static constexpr int in(int i, int d_in) { return i == 0 ? d_in : out(i - 1); }
  static constexpr int hidden_sum() { return (H + ...); }
  static constexpr int fwd_w(int b) {
    int w = 0;
    for (int i = 0; i < L; ++i)
      if (((i + 1) & 1) == b && out(i) > w) w = out(i);
    return w;
  }
  static constexpr int bwd_w(int b) {
    int w = 0;
    for (int i = 0; i < L; ++i)
      if (((L - 1 - i) & 1) == b && out(i) > w) w = out(i);
    return w;
  }
  static constexpr size_t bwd_lds_bytes() { return (size_t)CH_ROWS * (bwd_w(0) + bwd_w(1) + 2 * CH_PAD) * sizeof(float); }
};

// torch's argmax order: a NaN is the maximum, ties go to the lowest index
__device__ __forceinline__ bool argmax_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// out[m][n] = act(sum_k in[m][k] W[n][k] + bias[n]) for the workgroup's 16 rows; in / out in LDS.  A wave owns 16-column
// tiles; lane (c = lane & 15, q = lane >> 4) reads W[n0 + c][k + 4 q .. + 3] and in[c][k + 4 q .. + 3] as one 16-byte
// load each and feeds four MFMAs (the k order inside a 16-block is permuted; it is the same in every call and in every
// kernel built from this function).  DROPOUT: dr.apply(v, layer, idx4) masks and rescales the four activations of element
// index 4 idx4 .. + 3.  save == nullptr: nothing leaves LDS.
template <bool HIDDEN, bool DROPOUT, class Drop>
__device__ __forceinline__ void chain_layer_fwd(const float* in, int ldi, float* out, int ldo, const float* __restrict__ W,
                                                const float* __restrict__ bias, int K, int N, int layer, const Drop& dr,
                                                float* __restrict__ save, long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += CH_WAVES) {
    const int n0 = t * 16;
    int wr = n0 + c;
    if (wr >= N) wr = N - 1;
    const float* wp = W + (long)wr * K + 4 * q;
    const float* ip = in + c * ldi + 4 * q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 64) {          // K is a multiple of 64: four 16-byte loads of each operand in flight
      float4 w[4], a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        w[u] = *reinterpret_cast<const float4*>(wp + k + 16 * u);
        a[u] = *reinterpret_cast<const float4*>(ip + k + 16 * u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].x, a[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].y, a[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].z, a[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].w, a[u].w, acc, 0, 0, 0);
      }
    }
    // acc[r] = out[m = c][n = n0 + 4 q + r]
    const int n = n0 + 4 * q;
    const long row = row0 + c;
    if (HIDDEN) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + n);
      float v[4] = {fmaxf(acc[0] + bv.x, 0.f), fmaxf(acc[1] + bv.y, 0.f), fmaxf(acc[2] + bv.z, 0.f),
                    fmaxf(acc[3] + bv.w, 0.f)};
      if constexpr (DROPOUT) dr.apply(v, layer, (unsigned)((row * N + n) >> 2));
      const float4 o = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<float4*>(out + c * ldo + n) = o;
      if (save && row < B) *reinterpret_cast<float4*>(save + row * N + n) = o;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) {
          const float v = acc[r] + bias[n + r];
          out[c * ldo + n + r] = v;
          if (save && row < B) save[row * N + n + r] = v;
        }
    }
  }
}

template <int L>
struct ChainFwdArgs {
  const float* W[L];
  const float* b[L];
  float* save[L];     // h1 .. h(L-1), logits
};
struct NoDrop {};
struct ChainRows {    // the workgroup's 16 rows of something in LDS
  const float* p;
  int ld;
};

// x -> ... -> logits for the workgroup's rows; sm: chain_lds_bytes(d_in) of LDS.  Returns the logits' place in LDS, behind a
// barrier.  SAVE: every layer's output also goes to P.save.
template <class CH, bool SAVE, bool DROPOUT, class Drop>
__device__ __forceinline__ ChainRows chain_fwd(float* sm, const float* __restrict__ x, const ChainFwdArgs<CH::L>& P, int B,
                                               int d_in, int C, const Drop& dr) {
  const int ld[2] = {(d_in > CH::fwd_w(0) ? d_in : CH::fwd_w(0)) + CH_PAD, CH::fwd_w(1) + CH_PAD};
  float* const buf[2] = {sm, sm + CH_ROWS * ld[0]};
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int d4 = d_in >> 2;
  for (int i = threadIdx.x; i < CH_ROWS * d4; i += CH_THREADS) {
    const int m = i / d4, k = (i - m * d4) * 4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + m < B) v = *reinterpret_cast<const float4*>(x + (row0 + m) * d_in + k);
    *reinterpret_cast<float4*>(buf[0] + m * ld[0] + k) = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CH::L - 1; ++i) {
    chain_layer_fwd<true, DROPOUT>(buf[i & 1], ld[i & 1], buf[(i + 1) & 1], ld[(i + 1) & 1], P.W[i], P.b[i], CH::in(i, d_in),
                                   CH::out(i), i, dr, SAVE ? P.save[i] : nullptr, row0, B);
    __syncthreads();
  }
  constexpr int l = CH::L - 1;
  chain_layer_fwd<false, false>(buf[l & 1], ld[l & 1], buf[CH::L & 1], ld[CH::L & 1], P.W[l], P.b[l], CH::in(l, d_in), C, l, dr,
                                SAVE ? P.save[l] : nullptr, row0, B);
  __syncthreads();
  return ChainRows{buf[CH::L & 1], ld[CH::L & 1]};
}

// ---- forward, x walked in k chunks ---------------------------------------------------------------------------------------
// The same chain for a first layer whose input row does not fit LDS next to the widest hidden row (Chain<1024, 512, 256> at
// d_in >= 1536: 16 (d_in + 1024 + 8) 4 bytes pass the 163 840 of a workgroup).  Buffer 0 is fwd_w(0) wide and holds x one
// chunk of fwd_w(0) columns at a time; a wave keeps the accumulators of all its first-layer tiles across the chunks.  Every
// accumulator sees k in the order of chain_layer_fwd (ascending 64-blocks, u, x y z w), so the bits are those of chain_fwd
// wherever both can run.
template <class CH>
static size_t chain_chunked_lds_bytes() {
  return (size_t)CH_ROWS * (CH::fwd_w(0) + CH::fwd_w(1) + 2 * CH_PAD) * sizeof(float);
}

template <class CH, bool SAVE>
__device__ __forceinline__ ChainRows chain_fwd_chunked(float* sm, const float* __restrict__ x, const ChainFwdArgs<CH::L>& P,
                                                       int B, int d_in, int C) {
  constexpr int KC = CH::fwd_w(0), N0 = CH::out(0), TPW = N0 / 16 / CH_WAVES, TG = TPW % 4 == 0 ? 4 : 1;
  static_assert(KC % 64 == 0 && N0 % (16 * CH_WAVES) == 0 && N0 <= CH::fwd_w(1), "chunked first layer: whole tiles per wave");
  constexpr int ld[2] = {KC + CH_PAD, CH::fwd_w(1) + CH_PAD};
  float* const buf[2] = {sm, sm + CH_ROWS * ld[0]};
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  f32x4 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < d_in; k0 += KC) {
    const int kc = d_in - k0 < KC ? d_in - k0 : KC;      // a multiple of 64
    const int k4 = kc >> 2;
    if (k0) __syncthreads();                             // the previous chunk has been read
    for (int i = threadIdx.x; i < CH_ROWS * k4; i += CH_THREADS) {
      const int m = i / k4, k = (i - m * k4) * 4;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (row0 + m < B) v = *reinterpret_cast<const float4*>(x + (row0 + m) * d_in + k0 + k);
      *reinterpret_cast<float4*>(buf[0] + m * ld[0] + k) = v;
    }
    __syncthreads();
    // k outside, the wave's tiles inside in groups of TG: one read of the x operand serves TG tiles, whose weight loads are
    // in flight together and whose MFMA chains are independent of one another
    const float* ip = buf[0] + c * ld[0] + 4 * q;
    const float* wp = P.W[0] + (long)(wave * 16 + c) * d_in + k0 + 4 * q;
    for (int k = 0; k < kc; k += 64) {
      float4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(ip + k + 16 * u);
#pragma unroll
      for (int j0 = 0; j0 < TPW; j0 += TG) {
        float4 w[TG][4];
#pragma unroll
        for (int j = 0; j < TG; ++j)
#pragma unroll
          for (int u = 0; u < 4; ++u)
            w[j][u] = *reinterpret_cast<const float4*>(wp + (long)(j0 + j) * (CH_WAVES * 16) * d_in + k + 16 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < TG; ++j) {
            f32x4& A = acc[j0 + j];
            A = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u].x, a[u].x, A, 0, 0, 0);
            A = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u].y, a[u].y, A, 0, 0, 0);
            A = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u].z, a[u].z, A, 0, 0, 0);
            A = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u].w, a[u].w, A, 0, 0, 0);
          }
      }
    }
  }
  // acc[j][r] = h1[m = c][n = 16 (wave + 8 j) + 4 q + r]: the HIDDEN epilogue of chain_layer_fwd
  const long row = row0 + c;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int n = (wave + j * CH_WAVES) * 16 + 4 * q;
    const float4 bv = *reinterpret_cast<const float4*>(P.b[0] + n);
    const float4 o = {fmaxf(acc[j][0] + bv.x, 0.f), fmaxf(acc[j][1] + bv.y, 0.f), fmaxf(acc[j][2] + bv.z, 0.f),
                      fmaxf(acc[j][3] + bv.w, 0.f)};
    *reinterpret_cast<float4*>(buf[1] + c * ld[1] + n) = o;
    if (SAVE && P.save[0] && row < B) *reinterpret_cast<float4*>(P.save[0] + row * N0 + n) = o;
  }
  __syncthreads();
#pragma unroll
  for (int i = 1; i < CH::L - 1; ++i) {
    chain_layer_fwd<true, false>(buf[i & 1], ld[i & 1], buf[(i + 1) & 1], ld[(i + 1) & 1], P.W[i], P.b[i], CH::out(i - 1),
                                 CH::out(i), i, NoDrop{}, SAVE ? P.save[i] : nullptr, row0, B);
    __syncthreads();
  }
  constexpr int l = CH::L - 1;
  chain_layer_fwd<false, false>(buf[l & 1], ld[l & 1], buf[CH::L & 1], ld[CH::L & 1], P.W[l], P.b[l], CH::out(l - 1), C, l,
                                NoDrop{}, SAVE ? P.save[l] : nullptr, row0, B);
  __syncthreads();
  return ChainRows{buf[CH::L & 1], ld[CH::L & 1]};
}

// ---- backward, input side -------------------------------------------------------------------------------------------
// out[m][k] = sum_n dz[m][n] W[n][k] for the workgroup's 16 rows (dz in LDS, its columns zero-padded to a multiple of 16).
// A wave owns 64-column strips: lane (c, q) reads W[n + q][k0 + 4 c .. + 3] as one 16-byte load (a 256-byte run per row)
// and feeds four MFMAs whose outputs are the four columns k0 + 4 c + j.  acc[j][r] = out[m = 4 q + r][k0 + 4 c + j].
// MASK: keep the lanes whose saved activation is positive (the ReLU was open and, after dropout, the unit kept; SCALED:
// times `scale` = 1 / (1 - p)), write the layer's dz to LDS + workspace.
template <bool MASK, bool SCALED>
__device__ __forceinline__ void chain_layer_bwd(const float* dz, int ldz, float* out, int ldo, const float* __restrict__ W,
                                                int N, int K, const float* __restrict__ hsave, float scale,
                                                float* __restrict__ gout, long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int strips = K >> 6;
  for (int t = wave; t < strips; t += CH_WAVES) {
    const int k0 = t * 64 + 4 * c;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; n += 16) {          // dz columns are zero-padded to a multiple of 16 in LDS
      float a[4];
      float4 w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int nn = n + 4 * u + q;
        a[u] = dz[c * ldz + nn];
        w[u] = *reinterpret_cast<const float4*>(W + (long)(nn < N ? nn : N - 1) * K + k0);
        if (nn >= N) w[u] = float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].z, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].w, acc[3], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * q + r;
      const long row = row0 + m;
      float4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
      if (MASK) {
        float4 h = {0.f, 0.f, 0.f, 0.f};
        if (row < B) h = *reinterpret_cast<const float4*>(hsave + row * K + k0);
        const float s = SCALED ? scale : 1.f;   // x * 1.f folds away: the unscaled form is a plain select
        v.x = h.x > 0.f ? v.x * s : 0.f;
        v.y = h.y > 0.f ? v.y * s : 0.f;
        v.z = h.z > 0.f ? v.z * s : 0.f;
        v.w = h.w > 0.f ? v.w * s : 0.f;
        *reinterpret_cast<float4*>(out + m * ldo + k0) = v;
      }
      if (row < B) *reinterpret_cast<float4*>(gout + row * K + k0) = v;
    }
  }
}

template <int L>
struct ChainBwdArgs {
  const float* W[L];
  const float* h[L - 1];
  float* dz[L];       // the workspace (chain_carve)
  float* dx;
};

// dz_L (times the device scalar gscale, if given) -> ... -> dx for the workgroup's rows, every layer's dz left in A.dz.
// buf0 / buf1: the two LDS buffers, [CH_ROWS][CH::bwd_w(b) + CH_PAD] floats, 16-byte aligned.
template <class CH, bool SCALED>
__device__ __forceinline__ void chain_bwd(float* buf0, float* buf1, const float* __restrict__ dz_in,
                                          const float* __restrict__ gscale, const ChainBwdArgs<CH::L>& A, int B, int d_in, int C,
                                          float scale) {
  constexpr int L = CH::L, ld[2] = {CH::bwd_w(0) + CH_PAD, CH::bwd_w(1) + CH_PAD};
  float* const buf[2] = {buf0, buf1};
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const float g = gscale ? gscale[0] : 1.f;
  const int C16 = (C + 15) & ~15;
  for (int i = threadIdx.x; i < CH_ROWS * C16; i += CH_THREADS) {
    const int m = i / C16, n = i - m * C16;
    float v = 0.f;
    if (row0 + m < B && n < C) {
      v = g * dz_in[(row0 + m) * C + n];
      A.dz[L - 1][(row0 + m) * C + n] = v;
    }
    buf0[m * ld[0] + n] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = L - 1; i > 0; --i) {
    const int s = (L - 1 - i) & 1;
    chain_layer_bwd<true, SCALED>(buf[s], ld[s], buf[s ^ 1], ld[s ^ 1], A.W[i], CH::out(i, C), CH::out(i - 1), A.h[i - 1], scale,
                                  A.dz[i - 1], row0, B);
    __syncthreads();
  }
  constexpr int s = (L - 1) & 1;
  chain_layer_bwd<false, false>(buf[s], ld[s], nullptr, 0, A.W[0], CH::out(0), d_in, nullptr, 1.f, A.dx, row0, B);
}

// The backward-input kernel of a chain.  SCALED: the head has dropout, `scale` = 1 / (1 - p).  DYN_LDS: a chain whose two
// buffers pass the 64 KiB of static LDS takes its CH::bwd_lds_bytes() from the launch.  Same layer walk, same bits.
template <class CH, bool SCALED, bool DYN_LDS>
__global__ __launch_bounds__(CH_THREADS) void k_chain_bwd_in(const float* __restrict__ dz_in, const float* __restrict__ gscale,
                                                             ChainBwdArgs<CH::L> A, int B, int d_in, int C, float scale) {
  constexpr int n0 = CH_ROWS * (CH::bwd_w(0) + CH_PAD), n1 = CH_ROWS * (CH::bwd_w(1) + CH_PAD);
  if constexpr (DYN_LDS) {
    extern __shared__ __attribute__((aligned(16))) float sm_chain[];
    chain_bwd<CH, SCALED>(sm_chain, sm_chain + n0, dz_in, gscale, A, B, d_in, C, scale);
  } else {
    __shared__ __attribute__((aligned(16))) float buf0[n0];
    __shared__ __attribute__((aligned(16))) float buf1[n1];
    chain_bwd<CH, SCALED>(buf0, buf1, dz_in, gscale, A, B, d_in, C, scale);
  }
}

// ---- backward, weight side ------------------------------------------------------------------------------------------
struct ChainWgradLayer {
  const float* dz;    // [B, N]
  const float* h;     // [B, K]   the layer's input
  float* dW;          // [N, K]
  float* db;          // [N]
  int N, K, tiles_k, first;   // first workgroup of the layer
};
template <int L>
struct ChainWgradArgs {
  ChainWgradLayer l[L];
};

// ONE launch of 256 threads for all the layers.  dW[n][k] = sum_b dz[b][n] h[b][k]: 64 x 64 tile per workgroup, wave w rows
// n0 + 16 w .. + 15.  Lane (c, q) reads dz[b + q][n0 + 16 w + c] and h[b + q][k0 + 4 c .. + 3]; acc[j][r] =
// dW[n0 + 16 w + 4 q + r][k0 + 4 c + j].  The k-tile 0 workgroups also run the same dz operand against ones: every column
// of that accumulator is the bias gradient.
template <int L>
__device__ __forceinline__ void chain_bwd_w(const ChainWgradArgs<L>& A, int B) {
  int li = 0;
#pragma unroll
  for (int i = 1; i < L; ++i)
    if ((int)blockIdx.x >= A.l[i].first) li = i;
  const ChainWgradLayer Y = A.l[li];
  const int tile = blockIdx.x - Y.first;
  const int tn = tile / Y.tiles_k, tk = tile - tn * Y.tiles_k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int nb = tn * 64 + wave * 16;
  if (nb >= Y.N) return;                     // uniform per wave; no barrier below
  const int na = nb + c;
  const bool nok = na < Y.N;
  const int k0 = tk * 64 + 4 * c;
  const float* dzp = Y.dz + (nok ? na : Y.N - 1);
  const float* hp = Y.h + k0;
  f32x4 acc[4], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = tk == 0;
  for (int b = 0; b < B; b += 16) {
    float a[4], one[4];
    float4 h[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int bb = b + 4 * u + q;
      const bool ok = bb < B;
      const long br = ok ? bb : B - 1;
      a[u] = dzp[br * Y.N];
      h[u] = *reinterpret_cast<const float4*>(hp + br * Y.K);
      if (!ok || !nok) a[u] = 0.f;
      if (!ok) h[u] = float4{0.f, 0.f, 0.f, 0.f};
      one[u] = ok ? 1.f : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], h[u].x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], h[u].y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], h[u].z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], h[u].w, acc[3], 0, 0, 0);
      if (do_bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], one[u], accb, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = nb + 4 * q + r;
    if (n < Y.N) {
      *reinterpret_cast<float4*>(Y.dW + (long)n * Y.K + k0) = float4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
      if (do_bias && c == 0) Y.db[n] = accb[r];
    }
  }
}

template <int L>
__global__ __launch_bounds__(256) void k_chain_bwd_w(ChainWgradArgs<L> A, int B) {
  chain_bwd_w(A, B);
}

// loss = sum(row_loss) / div, one workgroup, fp64 partial sums in a fixed tree, rounded to fp32 once.  div: B, or
// (double)B * (double)C (exact for every admitted B and C).  A template, as the other two, so that only a file that launches
// it carries it; block_sum_f64 is a tree of 256 threads.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_chain_mean(const float* __restrict__ row_loss, int B, double div,
                                                        float* __restrict__ loss) {
  static_assert(THREADS == 256, "block_sum_f64");
  const double s = block_sum_f64(row_loss, B);
  if (threadIdx.x == 0) loss[0] = (float)(s / div);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int chain_check_shape(const char* who, int B, int Bmax, int d_in, int C, int Cmin) {
  GWW_REQUIRE(B >= 1 && B <= Bmax, "%s: B=%d must be 1..%d", who, B, Bmax);
  GWW_REQUIRE(d_in >= 128 && d_in <= 1280 && d_in % 128 == 0, "%s: d_in=%d must be a multiple of 128 in 128..1280", who, d_in);
  GWW_REQUIRE(C >= Cmin && C <= CH_CMAX, "%s: C=%d must be %d..%d", who, C, Cmin, CH_CMAX);
  return GWW_OK;
}
static bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (((uintptr_t)p) & 15) return false;
  return true;
}
// The one check of a chain's operands (include/gww.h: gww_mlp_params / _acts / _grads).  P->n_layers is the chain's L; x and
// every pointer of the L layers are non-NULL and 16-byte aligned, except the last layer's bias, the logits and the bias
// gradients, which are accessed by elements and only have to be there.  G == NULL: a forward, which reads the biases and,
// with H, writes the activations and the logits.  G != NULL: a backward, which reads w and H->h only.
static int chain_check_operands(const char* who, int L, const float* x, const gww_mlp_params* P, const gww_mlp_acts* H,
                                const gww_mlp_grads* G) {
  GWW_REQUIRE(x && P && (H || !G), "%s: NULL x or parameter block", who);
  GWW_REQUIRE(P->n_layers == L, "%s: n_layers=%d, but the chain has %d layers", who, P->n_layers, L);
  bool there = true, al = aligned16({x});
  auto see = [&](const void* p, bool align) {
    there = there && p;
    al = al && !(align && (((uintptr_t)p) & 15));
  };
  for (int i = 0; i < L; ++i) {
    see(P->w[i], true);
    if (!G) see(P->b[i], i < L - 1);
    if (H && i < L - 1) see(H->h[i], true);
    if (G) see(G->dw[i], true), see(G->db[i], false);
  }
  if (H && !G) see(H->logits, false);
  GWW_REQUIRE(there, "%s: NULL pointer among the %d layers' operands", who, L);
  GWW_REQUIRE(al, "%s: x and the %d layers' operands must be 16-byte aligned", who, L);
  return GWW_OK;
}
// dynamic LDS of the forward walk
template <class CH>
static size_t chain_lds_bytes(int d_in) {
  return (size_t)CH_ROWS * ((d_in > CH::fwd_w(0) ? d_in : CH::fwd_w(0)) + CH::fwd_w(1) + 2 * CH_PAD) * sizeof(float);
}
// workspace of the backward: dz1 [B, out(0)] | dz2 [B, out(1)] | ... | dzL [B, C]
template <class CH>
static size_t chain_workspace_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * (CH::hidden_sum() + C) * sizeof(float);
}
template <class CH>
static void chain_carve(float* ws, int B, float* (&dz)[CH::L]) {
  for (int i = 0; i < CH::L; ++i) {
    dz[i] = ws;
    ws += (size_t)B * CH::out(i);
  }
}
// the weight-gradient table of one step (h[0] = x); returns the grid size
template <class CH>
static int chain_wgrad_table(ChainWgradArgs<CH::L>& T, const float* x, const ChainBwdArgs<CH::L>& A, const gww_mlp_grads& G,
                             int d_in, int C) {
  int first = 0;
  for (int i = 0; i < CH::L; ++i) {
    const int N = CH::out(i, C), K = CH::in(i, d_in);
    T.l[i] = ChainWgradLayer{A.dz[i], i ? A.h[i - 1] : x, G.dw[i], G.db[i], N, K, K / 64, first};
    first += (int)cdiv(N, 64) * (K / 64);
  }
  return first;
}

// The forward kernel's arguments from the blocks.  h == NULL: no hidden activation leaves LDS (the score forms).
template <int L>
static ChainFwdArgs<L> chain_fwd_args(const gww_mlp_params* P, float* const* h, float* logits) {
  ChainFwdArgs<L> A;
  for (int i = 0; i < L; ++i) {
    A.W[i] = P->w[i];
    A.b[i] = P->b[i];
    A.save[i] = i == L - 1 ? logits : h ? h[i] : nullptr;
  }
  return A;
}

// The forward of every head: the caller's kernel (its chain walk and its tail) over ceil(B / 16) workgroups with `lds`
// bytes of dynamic LDS, then loss = sum(row_loss) / div.  loss == NULL: no loss, one launch (the score forms).
template <class... KA, class... A>
static int chain_launch_fwd(void (*kernel)(KA...), size_t lds, int B, const float* row_loss, double div, float* loss,
                            hipStream_t s, A... args) {
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(B, CH_ROWS)), dim3(CH_THREADS), lds, s, args...);
  GWW_LAUNCH_CHECK();
  if (!loss) return GWW_OK;
  hipLaunchKernelGGL(k_chain_mean<256>, dim3(1), dim3(256), 0, s, row_loss, B, div, loss);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

// The backward of every head, checks included: k_chain_bwd_in over the same row blocks, then ONE k_chain_bwd_w launch for
// all the layers.  scale: 1 / (1 - p) of a head with dropout (SCALED), else 1.
template <class CH, bool SCALED, bool DYN_LDS>
static int chain_backward(const char* who, const float* x, const gww_mlp_params* P, const gww_mlp_acts* H, const float* dz,
                          const float* dloss, int B, int d_in, int C, float scale, float* ws, size_t ws_bytes, float* dx,
                          const gww_mlp_grads* G, hipStream_t s) {
  constexpr int L = CH::L;
  GWW_REQUIRE(dz && ws && dx && G, "%s: NULL dz, ws, dx or gradient block", who);
  GWW_TRY(chain_check_operands(who, L, x, P, H, G));
  GWW_REQUIRE(aligned16({ws, dx}), "%s: ws and dx must be 16-byte aligned", who);
  GWW_REQUIRE(ws_bytes >= chain_workspace_bytes<CH>(B, C), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
              chain_workspace_bytes<CH>(B, C));
  ChainBwdArgs<L> A;
  for (int i = 0; i < L; ++i) A.W[i] = P->w[i];
  for (int i = 0; i < L - 1; ++i) A.h[i] = H->h[i];
  A.dx = dx;
  chain_carve<CH>(ws, B, A.dz);
  const size_t lds = DYN_LDS ? CH::bwd_lds_bytes() : 0;
  if (DYN_LDS)
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chain_bwd_in<CH, SCALED, DYN_LDS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_chain_bwd_in<CH, SCALED, DYN_LDS>), dim3((unsigned)cdiv(B, CH_ROWS)), dim3(CH_THREADS), lds, s, dz, dloss,
                     A, B, d_in, C, scale);
  GWW_LAUNCH_CHECK();
  ChainWgradArgs<L> T;
  const int grid = chain_wgrad_table<CH>(T, x, A, *G, d_in, C);
  hipLaunchKernelGGL(k_chain_bwd_w<L>, dim3((unsigned)grid), dim3(256), 0, s, T, B);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

// The backward of Chain<512, 256, 128, 64> without dropout, instantiated once, in detect.hip: the detection head's and the
// one-detector binary head's.
using DetChain = Chain<512, 256, 128, 64>;
int det_chain_backward(const char* who, const float* x, const gww_mlp_params* P, const gww_mlp_acts* H, const float* dz,
                       const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes, float* dx, const gww_mlp_grads* G,
                       hipStream_t s);

}  // namespace gww
