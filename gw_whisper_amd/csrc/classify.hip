// Glitch-classification head step (models.glitch_classifier: d_in -> 512 -> 256 -> 128 -> C with ReLU + Dropout between
// the layers, CrossEntropyLoss on top) and the evaluation accumulate, all exact fp32: every contraction is a
// v_mfma_f32_16x16x4_f32 chain (bit for bit a k-ordered fmaf chain), no float atomics, every reduction in a fixed order,
// so two identical calls give identical bits.  Plain launches only:
//   k_head_fwd    one workgroup per 16 rows walks the whole chain, activations in LDS, weights streamed from L2;
//                 tail: lse, row loss, argmax, dz = (softmax - onehot) / B
//   k_head_mean   one workgroup: the batch mean of the row losses (fixed order, fp64 partial sums)
//   k_head_bwd_in the same row blocks backwards: dh = dz W masked by the stored post-dropout activation, every layer's dz
//                 left in a workspace, the pooled-token gradient out
//   k_head_bwd_w  ONE launch for the four layers: a workgroup owns a 64 x 64 tile of one layer's dW = dz^T h (and the
//                 bias column sums of the same dz tile), reducing over the B rows inside the workgroup
// Dropout is Philox4x32-10 keyed by (seed, step offset, layer, element index): the mask depends on neither the launch
// geometry nor the row blocking.  The backward does not need to regenerate it: the saved activation is the POST-dropout
// one, which is positive exactly where the unit was kept AND the ReLU was open (x > 0 => x / (1 - p) > 0 in fp32).
#include "common.h"

namespace gww {

constexpr int HD_ROWS = 16;                 // rows of one workgroup (one MFMA tile)
constexpr int HD_THREADS = 512;             // 8 waves
constexpr int HD_WAVES = HD_THREADS / 64;
constexpr int HD_N1 = 512, HD_N2 = 256, HD_N3 = 128;
constexpr int HD_PAD = 4;                   // LDS row padding (floats): rows stay 16-byte aligned
constexpr int HD_CMAX = 64;

// ---- Philox4x32-10 (Salmon et al., SC'11) ------------------------------------------------------------------------
__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c = u32x4{hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// the four random words of elements 4 * idx4 .. 4 * idx4 + 3 of `layer`'s [B, width] activation (row-major element index)
__device__ __forceinline__ u32x4 drop_words(unsigned long long seed, unsigned long long offset, int layer, unsigned idx4) {
  return philox4x32_10(u32x4{idx4, (unsigned)layer, (unsigned)offset, (unsigned)(offset >> 32)}, (unsigned)seed,
                       (unsigned)(seed >> 32));
}

struct HeadDrop {
  unsigned long long seed, offset;
  unsigned thr;     // element dropped when its word < thr  (thr = p * 2^32)
  float scale;      // 1 / (1 - p)
  int on;           // train && p > 0
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// out[m][n] = act(sum_k in[m][k] W[n][k] + bias[n]) for the workgroup's 16 rows; in / out in LDS.  A wave owns 16-column
// tiles; lane (c = lane & 15, q = lane >> 4) reads W[n0 + c][k + 4 q .. + 3] and in[c][k + 4 q .. + 3] as one 16-byte
// load each and feeds four MFMAs (the k order inside a 16-block is permuted; it is the same in every call).
template <bool HIDDEN>
__device__ __forceinline__ void head_layer_fwd(const float* in, int ldi, float* out, int ldo, const float* __restrict__ W,
                                               const float* __restrict__ bias, int K, int N, int layer, const HeadDrop& dr,
                                               float* __restrict__ save, long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += HD_WAVES) {
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
      if (dr.on) {
        const u32x4 rw = drop_words(dr.seed, dr.offset, layer, (unsigned)((row * N + n) >> 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = rw[r] < dr.thr ? 0.f : v[r] * dr.scale;
      }
      const float4 o = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<float4*>(out + c * ldo + n) = o;
      if (row < B) *reinterpret_cast<float4*>(save + row * N + n) = o;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) {
          const float v = acc[r] + bias[n + r];
          out[c * ldo + n + r] = v;
          if (row < B) save[row * N + n + r] = v;
        }
    }
  }
}

// torch's argmax order: a NaN is the maximum, ties go to the lowest index
__device__ __forceinline__ bool head_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

__global__ __launch_bounds__(HD_THREADS) void k_head_fwd(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ w4,
    const float* __restrict__ b4, const long long* __restrict__ labels, int B, int d_in, int C, HeadDrop dr,
    float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ h3, float* __restrict__ logits,
    float* __restrict__ row_loss, long long* __restrict__ pred, float* __restrict__ dz4) {
  extern __shared__ __attribute__((aligned(16))) float sm_head[];
  const int ldA = (d_in > HD_N2 ? d_in : HD_N2) + HD_PAD, ldB = HD_N1 + HD_PAD;
  float* bufA = sm_head;                    // x [16][d_in], then h2 [16][256], then the logits [16][C]
  float* bufB = sm_head + HD_ROWS * ldA;    // h1 [16][512], then h3 [16][128]
  const long row0 = (long)blockIdx.x * HD_ROWS;
  const int tid = threadIdx.x;
  const int d4 = d_in >> 2;
  for (int i = tid; i < HD_ROWS * d4; i += HD_THREADS) {
    const int m = i / d4, k = (i - m * d4) * 4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + m < B) v = *reinterpret_cast<const float4*>(x + (row0 + m) * d_in + k);
    *reinterpret_cast<float4*>(bufA + m * ldA + k) = v;
  }
  __syncthreads();
  head_layer_fwd<true>(bufA, ldA, bufB, ldB, w1, b1, d_in, HD_N1, 0, dr, h1, row0, B);
  __syncthreads();
  head_layer_fwd<true>(bufB, ldB, bufA, ldA, w2, b2, HD_N1, HD_N2, 1, dr, h2, row0, B);
  __syncthreads();
  head_layer_fwd<true>(bufA, ldA, bufB, ldB, w3, b3, HD_N2, HD_N3, 2, dr, h3, row0, B);
  __syncthreads();
  head_layer_fwd<false>(bufB, ldB, bufA, ldA, w4, b4, HD_N3, C, 3, dr, logits, row0, B);
  __syncthreads();
  // tail: one wave per row, lane c holds logit c
  const int lane = tid & 63, wave = tid >> 6;
  for (int m = wave; m < HD_ROWS; m += HD_WAVES) {
    const long row = row0 + m;
    if (row >= B) break;                     // uniform per wave
    const float z = lane < C ? bufA[m * ldA + lane] : -INFINITY;
    float bv = z;
    int bi = lane < C ? lane : HD_CMAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (head_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    const float mx = wave_max(z);
    // everything relative to the row maximum (as torch's log_softmax): the rounding of lse itself never enters
    const float e = lane < C ? expf(z - mx) : 0.f;
    const float se = wave_sum(e);
    const long long y = labels[row];
    const bool yok = y >= 0 && y < C;
    const float zy = __shfl(z, yok ? (int)y : 0, 64);
    if (lane == 0) {
      row_loss[row] = yok ? logf(se) - (zy - mx) : __builtin_nanf("");   // a label outside [0, C) poisons the loss, never memory
      pred[row] = bi;
    }
    // softmax - onehot; at the label's own lane that is -(sum of the OTHER lanes' e) / se, summed as such: e / se - 1
    // would cancel to the rounding of se when the row is confident
    const bool mine = yok && lane == (int)y;
    const float others = wave_sum(mine ? 0.f : e);
    if (lane < C) dz4[row * C + lane] = (mine ? -others : e) / se / (float)B;
  }
}

// mean of the row losses: thread t sums rows t, t + 256, ... in fp64, then a fixed LDS tree
__global__ __launch_bounds__(256) void k_head_mean(const float* __restrict__ row_loss, int B, float* __restrict__ loss) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 256) s += (double)row_loss[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(part[0] / (double)B);
}

// ---- backward, input side -------------------------------------------------------------------------------------------
// out[m][k] = sum_n dz[m][n] W[n][k] for the workgroup's 16 rows (dz in LDS, its columns zero-padded to a multiple of 16).
// A wave owns 64-column strips: lane (c, q) reads W[n + q][k0 + 4 c .. + 3] as one 16-byte load (a 256-byte run per row)
// and feeds four MFMAs whose outputs are the four columns k0 + 4 c + j.  acc[j][r] = out[m = 4 q + r][k0 + 4 c + j].
// MASK: multiply by the saved post-dropout activation's sign (and 1 / (1 - p)), write the layer's dz to LDS + workspace.
template <bool MASK>
__device__ __forceinline__ void head_layer_bwd(const float* dz, int ldz, float* out, int ldo, const float* __restrict__ W,
                                               int N, int K, const float* __restrict__ hsave, float scale,
                                               float* __restrict__ gout, long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int strips = K >> 6;
  for (int t = wave; t < strips; t += HD_WAVES) {
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
        v.x = h.x > 0.f ? v.x * scale : 0.f;
        v.y = h.y > 0.f ? v.y * scale : 0.f;
        v.z = h.z > 0.f ? v.z * scale : 0.f;
        v.w = h.w > 0.f ? v.w * scale : 0.f;
        *reinterpret_cast<float4*>(out + m * ldo + k0) = v;
      }
      if (row < B) *reinterpret_cast<float4*>(gout + row * K + k0) = v;
    }
  }
}

__global__ __launch_bounds__(HD_THREADS) void k_head_bwd_in(
    const float* __restrict__ dz4_in, const float* __restrict__ gscale, const float* __restrict__ w1,
    const float* __restrict__ w2, const float* __restrict__ w3, const float* __restrict__ w4, const float* __restrict__ h1,
    const float* __restrict__ h2, const float* __restrict__ h3, int B, int d_in, int C, float scale,
    float* __restrict__ dz1, float* __restrict__ dz2, float* __restrict__ dz3, float* __restrict__ dz4, float* __restrict__ dx) {
  constexpr int ldA = HD_N2 + HD_PAD, ldB = HD_N1 + HD_PAD;
  __shared__ __attribute__((aligned(16))) float bufA[HD_ROWS * ldA];   // dz4 [16][C4], then dz2 [16][256]
  __shared__ __attribute__((aligned(16))) float bufB[HD_ROWS * ldB];   // dz3 [16][128], then dz1 [16][512]
  const long row0 = (long)blockIdx.x * HD_ROWS;
  const int tid = threadIdx.x;
  const float g = gscale ? gscale[0] : 1.f;
  const int C4 = (C + 15) & ~15;
  for (int i = tid; i < HD_ROWS * C4; i += HD_THREADS) {
    const int m = i / C4, n = i - m * C4;
    float v = 0.f;
    if (row0 + m < B && n < C) {
      v = g * dz4_in[(row0 + m) * C + n];
      dz4[(row0 + m) * C + n] = v;
    }
    bufA[m * ldA + n] = v;
  }
  __syncthreads();
  head_layer_bwd<true>(bufA, ldA, bufB, ldB, w4, C, HD_N3, h3, scale, dz3, row0, B);
  __syncthreads();
  head_layer_bwd<true>(bufB, ldB, bufA, ldA, w3, HD_N3, HD_N2, h2, scale, dz2, row0, B);
  __syncthreads();
  head_layer_bwd<true>(bufA, ldA, bufB, ldB, w2, HD_N2, HD_N1, h1, scale, dz1, row0, B);
  __syncthreads();
  head_layer_bwd<false>(bufB, ldB, nullptr, 0, w1, HD_N1, d_in, nullptr, 1.f, dx, row0, B);
}

// ---- backward, weight side ------------------------------------------------------------------------------------------
struct HeadWgradLayer {
  const float* dz;    // [B, N]
  const float* h;     // [B, K]   the layer's input
  float* dW;          // [N, K]
  float* db;          // [N]
  int N, K, tiles_k, first;   // first workgroup of the layer
};
struct HeadWgradArgs {
  HeadWgradLayer l[4];
};

// dW[n][k] = sum_b dz[b][n] h[b][k]: 64 x 64 tile per workgroup, wave w rows n0 + 16 w .. + 15.  Lane (c, q) reads
// dz[b + q][n0 + 16 w + c] and h[b + q][k0 + 4 c .. + 3]; acc[j][r] = dW[n0 + 16 w + 4 q + r][k0 + 4 c + j].  The k-tile 0
// workgroups also run the same dz operand against ones: every column of that accumulator is the bias gradient.
__global__ __launch_bounds__(256) void k_head_bwd_w(HeadWgradArgs A, int B) {
  int li = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if ((int)blockIdx.x >= A.l[i].first) li = i;
  const HeadWgradLayer L = A.l[li];
  const int tile = blockIdx.x - L.first;
  const int tn = tile / L.tiles_k, tk = tile - tn * L.tiles_k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int nb = tn * 64 + wave * 16;
  if (nb >= L.N) return;                     // uniform per wave; no barrier below
  const int na = nb + c;
  const bool nok = na < L.N;
  const int k0 = tk * 64 + 4 * c;
  const float* dzp = L.dz + (nok ? na : L.N - 1);
  const float* hp = L.h + k0;
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
      a[u] = dzp[br * L.N];
      h[u] = *reinterpret_cast<const float4*>(hp + br * L.K);
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
    if (n < L.N) {
      *reinterpret_cast<float4*>(L.dW + (long)n * L.K + k0) = float4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
      if (do_bias && c == 0) L.db[n] = accb[r];
    }
  }
}

// ---- dropout mask (for tests: rebuild the step in fp64) -------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_mask(unsigned long long seed, unsigned long long offset, int layer, long n4,
                                                   unsigned thr, float* __restrict__ mask) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const u32x4 rw = drop_words(seed, offset, layer, (unsigned)i);
  *reinterpret_cast<float4*>(mask + 4 * i) =
      float4{rw[0] < thr ? 0.f : 1.f, rw[1] < thr ? 0.f : 1.f, rw[2] < thr ? 0.f : 1.f, rw[3] < thr ? 0.f : 1.f};
}

// ---- evaluation accumulate ------------------------------------------------------------------------------------------
// one workgroup: confusion[y][argmax] += 1 (int64; the per-launch counts go through LDS integer atomics, which commute),
// loss_sum += sum of the row losses (fp64, fixed order, one writer), n += B.  Rows with a label outside [0, C) are
// counted in n and the loss but not in the matrix.
__global__ __launch_bounds__(256) void k_eval_accumulate(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                         const float* __restrict__ row_loss, int B, int C,
                                                         long long* __restrict__ confusion, double* __restrict__ loss_sum,
                                                         long long* __restrict__ n) {
  __shared__ int cnt[HD_CMAX * HD_CMAX];
  __shared__ double part[256];
  const int tid = threadIdx.x;
  for (int i = tid; i < C * C; i += 256) cnt[i] = 0;
  __syncthreads();
  double s = 0.0;
  for (int r = tid; r < B; r += 256) {
    const float* z = logits + (long)r * C;
    float bv = z[0];
    int bi = 0;
    for (int j = 1; j < C; ++j)
      if (head_better(z[j], j, bv, bi)) { bv = z[j]; bi = j; }
    const long long y = labels[r];
    if (y >= 0 && y < C) atomicAdd(&cnt[(int)y * C + bi], 1);
    s += (double)row_loss[r];
  }
  part[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  for (int i = tid; i < C * C; i += 256)
    if (cnt[i]) confusion[i] += cnt[i];
  if (tid == 0) {
    loss_sum[0] += part[0];
    n[0] += B;
  }
}

static int head_check_shape(const char* who, int B, int d_in, int C) {
  GWW_REQUIRE(B >= 1 && B <= 1024, "%s: B=%d must be 1..1024", who, B);
  GWW_REQUIRE(d_in >= 128 && d_in <= 1280 && d_in % 128 == 0, "%s: d_in=%d must be a multiple of 128 in 128..1280", who, d_in);
  GWW_REQUIRE(C >= 1 && C <= HD_CMAX, "%s: C=%d must be 1..%d", who, C, HD_CMAX);
  return GWW_OK;
}
static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace gww

using namespace gww;

extern "C" int gww_head_forward_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                    const float* w3, const float* b3, const float* w4, const float* b4,
                                    const long long* labels, int B, int d_in, int C, float p, int train,
                                    unsigned long long seed, unsigned long long offset, float* h1, float* h2, float* h3,
                                    float* logits, float* row_loss, long long* pred, float* dz, float* loss, void* stream) {
  GWW_TRY(head_check_shape("gww_head_forward_f32", B, d_in, C));
  GWW_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && w4 && b4 && labels, "gww_head_forward_f32: NULL input");
  GWW_REQUIRE(h1 && h2 && h3 && logits && row_loss && pred && dz && loss, "gww_head_forward_f32: NULL output");
  GWW_REQUIRE(p >= 0.f && p < 1.f, "gww_head_forward_f32: dropout p=%g must be in [0, 1)", (double)p);
  GWW_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(w3) && aligned16(w4) && aligned16(b1) &&
                  aligned16(b2) && aligned16(b3) && aligned16(h1) && aligned16(h2) && aligned16(h3),
              "gww_head_forward_f32: operands must be 16-byte aligned");
  HeadDrop dr;
  dr.seed = seed;
  dr.offset = offset;
  dr.on = train && p > 0.f;
  dr.thr = (unsigned)((double)p * 4294967296.0);
  dr.scale = dr.on ? 1.f / (1.f - p) : 1.f;
  const int ldA = (d_in > HD_N2 ? d_in : HD_N2) + HD_PAD, ldB = HD_N1 + HD_PAD;
  const size_t lds = (size_t)HD_ROWS * (ldA + ldB) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_head_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_head_fwd, dim3((unsigned)cdiv(B, HD_ROWS)), dim3(HD_THREADS), lds, s, x, w1, b1, w2, b2, w3, b3, w4, b4,
                     labels, B, d_in, C, dr, h1, h2, h3, logits, row_loss, pred, dz);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_head_mean, dim3(1), dim3(256), 0, s, (const float*)row_loss, B, loss);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_head_backward_f32(const float* x, const float* w1, const float* w2, const float* w3, const float* w4,
                                     const float* h1, const float* h2, const float* h3, const float* dz, const float* dloss,
                                     int B, int d_in, int C, float p, int train, float* ws, float* dx, float* dw1, float* db1,
                                     float* dw2, float* db2, float* dw3, float* db3, float* dw4, float* db4, void* stream) {
  GWW_TRY(head_check_shape("gww_head_backward_f32", B, d_in, C));
  GWW_REQUIRE(x && w1 && w2 && w3 && w4 && h1 && h2 && h3 && dz, "gww_head_backward_f32: NULL input");
  GWW_REQUIRE(ws && dx && dw1 && db1 && dw2 && db2 && dw3 && db3 && dw4 && db4, "gww_head_backward_f32: NULL output");
  GWW_REQUIRE(p >= 0.f && p < 1.f, "gww_head_backward_f32: dropout p=%g must be in [0, 1)", (double)p);
  GWW_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(w3) && aligned16(w4) && aligned16(h1) &&
                  aligned16(h2) && aligned16(h3) && aligned16(ws) && aligned16(dx) && aligned16(dw1) && aligned16(dw2) &&
                  aligned16(dw3) && aligned16(dw4),
              "gww_head_backward_f32: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // workspace: dz1 [B, 512] | dz2 [B, 256] | dz3 [B, 128] | dz4 [B, C]  (gww_head_workspace_bytes)
  float* dz1 = ws;
  float* dz2 = dz1 + (size_t)B * HD_N1;
  float* dz3 = dz2 + (size_t)B * HD_N2;
  float* dz4 = dz3 + (size_t)B * HD_N3;
  const float scale = (train && p > 0.f) ? 1.f / (1.f - p) : 1.f;
  hipLaunchKernelGGL(k_head_bwd_in, dim3((unsigned)cdiv(B, HD_ROWS)), dim3(HD_THREADS), 0, s, dz, dloss, w1, w2, w3, w4, h1, h2,
                     h3, B, d_in, C, scale, dz1, dz2, dz3, dz4, dx);
  GWW_LAUNCH_CHECK();
  HeadWgradArgs A;
  const float* dzs[4] = {dz1, dz2, dz3, dz4};
  const float* hs[4] = {x, h1, h2, h3};
  float* dws[4] = {dw1, dw2, dw3, dw4};
  float* dbs[4] = {db1, db2, db3, db4};
  const int Ns[4] = {HD_N1, HD_N2, HD_N3, C}, Ks[4] = {d_in, HD_N1, HD_N2, HD_N3};
  int first = 0;
  for (int i = 0; i < 4; ++i) {
    A.l[i] = HeadWgradLayer{dzs[i], hs[i], dws[i], dbs[i], Ns[i], Ks[i], Ks[i] / 64, first};
    first += (int)cdiv(Ns[i], 64) * (Ks[i] / 64);
  }
  hipLaunchKernelGGL(k_head_bwd_w, dim3((unsigned)first), dim3(256), 0, s, A, B);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_head_workspace_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * (HD_N1 + HD_N2 + HD_N3 + C) * sizeof(float);
}

extern "C" int gww_head_dropout_mask_f32(unsigned long long seed, unsigned long long offset, int layer, int B, int width,
                                         float p, float* mask, void* stream) {
  GWW_REQUIRE(mask, "gww_head_dropout_mask_f32: NULL output");
  GWW_REQUIRE(B >= 1 && B <= 1024 && width >= 4 && width % 4 == 0 && width <= 4096,
              "gww_head_dropout_mask_f32: B=%d must be 1..1024 and width=%d a multiple of 4 up to 4096", B, width);
  GWW_REQUIRE(layer >= 0 && layer < 3, "gww_head_dropout_mask_f32: layer=%d must be 0, 1 or 2", layer);
  GWW_REQUIRE(p >= 0.f && p < 1.f, "gww_head_dropout_mask_f32: dropout p=%g must be in [0, 1)", (double)p);
  GWW_REQUIRE(aligned16(mask), "gww_head_dropout_mask_f32: mask must be 16-byte aligned");
  const long n4 = (long)B * width / 4;
  hipLaunchKernelGGL(k_head_mask, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, seed, offset, layer, n4,
                     (unsigned)((double)p * 4294967296.0), mask);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_eval_accumulate(const float* logits, const long long* labels, const float* row_loss, int B, int C,
                                   long long* confusion, double* loss_sum, long long* n, void* stream) {
  GWW_REQUIRE(logits && labels && row_loss && confusion && loss_sum && n, "gww_eval_accumulate: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= 65536, "gww_eval_accumulate: B=%d must be 1..65536", B);
  GWW_REQUIRE(C >= 1 && C <= HD_CMAX, "gww_eval_accumulate: C=%d must be 1..%d", C, HD_CMAX);
  hipLaunchKernelGGL(k_eval_accumulate, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, row_loss, B, C, confusion,
                     loss_sum, n);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
