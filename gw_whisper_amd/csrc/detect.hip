// Detection head step (models.efficiency_classifier / GWWhisperClassifier: d_in -> 512 -> 256 -> 128 -> 64 -> C with ReLU
// between the layers, Softmax(dim=1) and the regularised BCELoss on top), its inference-only score form, and the device
// side of the evaluation / detection-efficiency statistics.  Conventions of classify.hip: exact fp32, every contraction a
// v_mfma_f32_16x16x4_f32 chain, no float atomics, every reduction in a fixed order (identical calls give identical bits),
// plain launches, nothing here synchronises.
//   k_det_fwd        one workgroup per 16 rows walks the five layers through LDS; tail (fp64 on the fp32 logits, rounded
//                    once): softmax, q = eps + (1 - C eps) p, the row's BCE sum, dz = d loss / d logits.  MODE >= 0: no
//                    saves, one score per row (inference)
//   k_det_mean       one workgroup: loss = sum(row_loss) / (B C), fp64 partial sums in a fixed tree
//   k_det_bwd_in     the same row blocks backwards, every layer's dz left in a workspace, the pooled-token gradient out
//   k_det_bwd_w      ONE launch for the five layers' dW = dz^T h and db
//   k_det_eval       one workgroup: correct += #(argmax targets == argmax probs), loss_sum += the batch's mean loss
//   k_sel_*          radix select over the order-preserving integer image of fp32: four 8-bit histogram passes for all
//                    F ranks together (integer atomics only: they commute)
//   k_det_counts     counts[f] += #{scores > thr[f]}
#include "common.h"

namespace gww {

constexpr int DT_ROWS = 16;                 // rows of one workgroup (one MFMA tile)
constexpr int DT_THREADS = 512;             // 8 waves
constexpr int DT_WAVES = DT_THREADS / 64;
constexpr int DT_N1 = 512, DT_N2 = 256, DT_N3 = 128, DT_N4 = 64;
constexpr int DT_PAD = 4;                   // LDS row padding (floats): rows stay 16-byte aligned
constexpr int DT_CMAX = 64;
constexpr int DT_FMAX = 8;                  // false-alarm ranks of one selection

// ---- forward ---------------------------------------------------------------------------------------------------------
// out[m][n] = act(sum_k in[m][k] W[n][k] + bias[n]) for the workgroup's 16 rows; in / out in LDS.  A wave owns 16-column
// tiles; lane (c = lane & 15, q = lane >> 4) reads W[n0 + c][k + 4 q .. + 3] and in[c][k + 4 q .. + 3] as one 16-byte
// load each and feeds four MFMAs (the k order inside a 16-block is permuted; it is the same in every call and in both
// kernels built from this function).  save == nullptr: nothing leaves LDS.
template <bool HIDDEN>
__device__ __forceinline__ void det_layer_fwd(const float* in, int ldi, float* out, int ldo, const float* __restrict__ W,
                                              const float* __restrict__ bias, int K, int N, float* __restrict__ save,
                                              long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += DT_WAVES) {
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
      const float4 o = {fmaxf(acc[0] + bv.x, 0.f), fmaxf(acc[1] + bv.y, 0.f), fmaxf(acc[2] + bv.z, 0.f),
                        fmaxf(acc[3] + bv.w, 0.f)};
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

// torch's argmax order: a NaN is the maximum, ties go to the lowest index
__device__ __forceinline__ bool det_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

__device__ __forceinline__ double det_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct DetWeights {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4, *w5, *b5;
};
struct DetSaves {
  float *h1, *h2, *h3, *h4, *logits, *probs, *row_loss, *dz;
};

// MODE -1: the training / evaluation forward (saves, loss tail).  MODE 0: score = probs[:, 0].  MODE 1: score = z0 - z1.
template <int MODE>
__global__ __launch_bounds__(DT_THREADS) void k_det_fwd(const float* __restrict__ x, DetWeights P,
                                                        const float* __restrict__ targets, int B, int d_in, int C, float eps,
                                                        DetSaves S, float* __restrict__ score, long score_stride) {
  extern __shared__ __attribute__((aligned(16))) float sm_det[];
  const int ldA = (d_in > DT_N2 ? d_in : DT_N2) + DT_PAD, ldB = DT_N1 + DT_PAD;
  float* bufA = sm_det;                     // x [16][d_in], then h2 [16][256], then h4 [16][64]
  float* bufB = sm_det + DT_ROWS * ldA;     // h1 [16][512], then h3 [16][128], then the logits [16][C]
  const long row0 = (long)blockIdx.x * DT_ROWS;
  const int tid = threadIdx.x;
  const int d4 = d_in >> 2;
  for (int i = tid; i < DT_ROWS * d4; i += DT_THREADS) {
    const int m = i / d4, k = (i - m * d4) * 4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + m < B) v = *reinterpret_cast<const float4*>(x + (row0 + m) * d_in + k);
    *reinterpret_cast<float4*>(bufA + m * ldA + k) = v;
  }
  constexpr bool SAVE = MODE < 0;
  __syncthreads();
  det_layer_fwd<true>(bufA, ldA, bufB, ldB, P.w1, P.b1, d_in, DT_N1, SAVE ? S.h1 : nullptr, row0, B);
  __syncthreads();
  det_layer_fwd<true>(bufB, ldB, bufA, ldA, P.w2, P.b2, DT_N1, DT_N2, SAVE ? S.h2 : nullptr, row0, B);
  __syncthreads();
  det_layer_fwd<true>(bufA, ldA, bufB, ldB, P.w3, P.b3, DT_N2, DT_N3, SAVE ? S.h3 : nullptr, row0, B);
  __syncthreads();
  det_layer_fwd<true>(bufB, ldB, bufA, ldA, P.w4, P.b4, DT_N3, DT_N4, SAVE ? S.h4 : nullptr, row0, B);
  __syncthreads();
  det_layer_fwd<false>(bufA, ldA, bufB, ldB, P.w5, P.b5, DT_N4, C, SAVE ? S.logits : nullptr, row0, B);
  __syncthreads();
  // tail: one wave per row, lane c holds logit c
  const int lane = tid & 63, wave = tid >> 6;
  for (int m = wave; m < DT_ROWS; m += DT_WAVES) {
    const long row = row0 + m;
    if (row >= B) break;                     // uniform per wave
    if (MODE == 1) {
      if (lane == 0) score[row * score_stride] = bufB[m * ldB] - bufB[m * ldB + 1];
      continue;
    }
    // Everything behind the logits is fp64, rounded to fp32 once per output: the last layer's bias gradient is a batch sum
    // of dz columns that cancel (for C = 2 the two columns are each other's negatives), which amplifies whatever rounding
    // dz carries; the tail is B x C elements, its cost does not show.
    const float z = lane < C ? bufB[m * ldB + lane] : -INFINITY;
    const float mx = wave_max(z);
    const double e = lane < C ? exp((double)z - (double)mx) : 0.0;
    const double se = det_wave_sum(e);
    const double p = e / se;
    if (MODE == 0) {
      if (lane == 0) score[row * score_stride] = (float)p;
      continue;
    }
    // 1 - p_c as (the sum of the OTHER lanes' e) / se, summed in lane order: 1 - e / se would cancel to the rounding of se
    // exactly where the loss is largest (a confident row)
    double others = 0.0;
    for (int j = 0; j < C; ++j) {
      const double ej = __shfl(e, j, 64);
      if (j != lane) others += ej;
    }
    const double omp = others / se;
    const double bc = 1.0 - (double)C * (double)eps;
    const double qv = (double)eps + bc * p;                       // q
    const double omq = (double)(C - 1) * (double)eps + bc * omp;  // 1 - q, without the subtraction
    const double t = lane < C ? (double)targets[row * C + lane] : 0.0;
    const double lq = fmax(log(qv), -100.0), lomq = fmax(log(omq), -100.0);   // nn.BCELoss clamps its logs at -100
    const double el = lane < C ? -(t * lq + (1.0 - t) * lomq) : 0.0;
    const double rl = det_wave_sum(el);
    // d loss / d q in torch's form, then through q = eps + bc p and the softmax:
    // dz_c = p_c (dp_c (1 - p_c) - sum over the other lanes of p_j dp_j)
    // (q - t = (1 - t) q - t (1 - q): no cancellation at a confident, correct lane)
    const double dq = ((1.0 - t) * qv - t * omq) / fmax(omq * qv, 1e-12) / ((double)B * (double)C);
    const double pdp = lane < C ? p * (bc * dq) : 0.0;
    double cross = 0.0;
    for (int j = 0; j < C; ++j) {
      const double pj = __shfl(pdp, j, 64);
      if (j != lane) cross += pj;
    }
    if (lane < C) {
      S.probs[row * C + lane] = (float)p;
      S.dz[row * C + lane] = (float)(pdp * omp - p * cross);
    }
    if (lane == 0) S.row_loss[row] = (float)rl;
  }
}

// sum of v[0 .. n) in fp64: thread t takes t, t + 256, ..., then a fixed LDS tree.  All 256 threads call it; the result is
// valid in thread 0.
__device__ __forceinline__ double det_block_sum(const float* __restrict__ v, int n, double* part) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(256) void k_det_mean(const float* __restrict__ row_loss, int B, int C, float* __restrict__ loss) {
  __shared__ double part[256];
  const double s = det_block_sum(row_loss, B, part);
  if (threadIdx.x == 0) loss[0] = (float)(s / ((double)B * (double)C));
}

// ---- backward, input side -------------------------------------------------------------------------------------------
// out[m][k] = sum_n dz[m][n] W[n][k] for the workgroup's 16 rows (dz in LDS, its columns zero-padded to a multiple of 16).
// A wave owns 64-column strips: lane (c, q) reads W[n + q][k0 + 4 c .. + 3] as one 16-byte load and feeds four MFMAs whose
// outputs are the four columns k0 + 4 c + j.  acc[j][r] = out[m = 4 q + r][k0 + 4 c + j].
// MASK: multiply by the saved activation's sign (the ReLU), write the layer's dz to LDS + workspace.
template <bool MASK>
__device__ __forceinline__ void det_layer_bwd(const float* dz, int ldz, float* out, int ldo, const float* __restrict__ W,
                                              int N, int K, const float* __restrict__ hsave, float* __restrict__ gout,
                                              long row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int strips = K >> 6;
  for (int t = wave; t < strips; t += DT_WAVES) {
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
        v.x = h.x > 0.f ? v.x : 0.f;
        v.y = h.y > 0.f ? v.y : 0.f;
        v.z = h.z > 0.f ? v.z : 0.f;
        v.w = h.w > 0.f ? v.w : 0.f;
        *reinterpret_cast<float4*>(out + m * ldo + k0) = v;
      }
      if (row < B) *reinterpret_cast<float4*>(gout + row * K + k0) = v;
    }
  }
}

struct DetBwdArgs {
  const float *w1, *w2, *w3, *w4, *w5, *h1, *h2, *h3, *h4;
  float *dz1, *dz2, *dz3, *dz4, *dz5, *dx;
};

__global__ __launch_bounds__(DT_THREADS) void k_det_bwd_in(const float* __restrict__ dz_in, const float* __restrict__ gscale,
                                                           DetBwdArgs A, int B, int d_in, int C) {
  constexpr int ldA = DT_N1 + DT_PAD, ldB = DT_N2 + DT_PAD;
  __shared__ __attribute__((aligned(16))) float bufA[DT_ROWS * ldA];   // dz5 [16][C16], then dz3 [16][128], then dz1 [16][512]
  __shared__ __attribute__((aligned(16))) float bufB[DT_ROWS * ldB];   // dz4 [16][64], then dz2 [16][256]
  const long row0 = (long)blockIdx.x * DT_ROWS;
  const int tid = threadIdx.x;
  const float g = gscale ? gscale[0] : 1.f;
  const int C16 = (C + 15) & ~15;
  for (int i = tid; i < DT_ROWS * C16; i += DT_THREADS) {
    const int m = i / C16, n = i - m * C16;
    float v = 0.f;
    if (row0 + m < B && n < C) {
      v = g * dz_in[(row0 + m) * C + n];
      A.dz5[(row0 + m) * C + n] = v;
    }
    bufA[m * ldA + n] = v;
  }
  __syncthreads();
  det_layer_bwd<true>(bufA, ldA, bufB, ldB, A.w5, C, DT_N4, A.h4, A.dz4, row0, B);
  __syncthreads();
  det_layer_bwd<true>(bufB, ldB, bufA, ldA, A.w4, DT_N4, DT_N3, A.h3, A.dz3, row0, B);
  __syncthreads();
  det_layer_bwd<true>(bufA, ldA, bufB, ldB, A.w3, DT_N3, DT_N2, A.h2, A.dz2, row0, B);
  __syncthreads();
  det_layer_bwd<true>(bufB, ldB, bufA, ldA, A.w2, DT_N2, DT_N1, A.h1, A.dz1, row0, B);
  __syncthreads();
  det_layer_bwd<false>(bufA, ldA, nullptr, 0, A.w1, DT_N1, d_in, nullptr, A.dx, row0, B);
}

// ---- backward, weight side ------------------------------------------------------------------------------------------
struct DetWgradLayer {
  const float* dz;    // [B, N]
  const float* h;     // [B, K]   the layer's input
  float* dW;          // [N, K]
  float* db;          // [N]
  int N, K, tiles_k, first;   // first workgroup of the layer
};
struct DetWgradArgs {
  DetWgradLayer l[5];
};

// dW[n][k] = sum_b dz[b][n] h[b][k]: 64 x 64 tile per workgroup, wave w rows n0 + 16 w .. + 15.  Lane (c, q) reads
// dz[b + q][n0 + 16 w + c] and h[b + q][k0 + 4 c .. + 3]; acc[j][r] = dW[n0 + 16 w + 4 q + r][k0 + 4 c + j].  The k-tile 0
// workgroups also run the same dz operand against ones: every column of that accumulator is the bias gradient.
__global__ __launch_bounds__(256) void k_det_bwd_w(DetWgradArgs A, int B) {
  int li = 0;
#pragma unroll
  for (int i = 1; i < 5; ++i)
    if ((int)blockIdx.x >= A.l[i].first) li = i;
  const DetWgradLayer L = A.l[li];
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

// ---- evaluation accumulate ------------------------------------------------------------------------------------------
// one workgroup: correct += #(argmax targets == argmax probs) (integer LDS atomics: they commute), loss_sum += the batch's
// mean loss as k_det_mean rounds it to fp32 (the reference sums loss.item() over batches and divides by their number),
// n += B, batches += 1; one writer.
__global__ __launch_bounds__(256) void k_det_eval(const float* __restrict__ probs, const float* __restrict__ targets,
                                                  const float* __restrict__ row_loss, int B, int C,
                                                  long long* __restrict__ correct, double* __restrict__ loss_sum,
                                                  long long* __restrict__ n, long long* __restrict__ batches) {
  __shared__ int cnt;
  __shared__ double part[256];
  const int tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int r = tid; r < B; r += 256) {
    const float* p = probs + (long)r * C;
    const float* t = targets + (long)r * C;
    float pv = p[0], tv = t[0];
    int pi = 0, ti = 0;
    for (int j = 1; j < C; ++j) {
      if (det_better(p[j], j, pv, pi)) { pv = p[j]; pi = j; }
      if (det_better(t[j], j, tv, ti)) { tv = t[j]; ti = j; }
    }
    mine += pi == ti;
  }
  if (mine) atomicAdd(&cnt, mine);
  const double s = det_block_sum(row_loss, B, part);     // its barriers also order cnt
  if (tid == 0) {
    correct[0] += cnt;
    loss_sum[0] += (double)(float)(s / ((double)B * (double)C));
    n[0] += B;
    batches[0] += 1;
  }
}

// ---- rank selection --------------------------------------------------------------------------------------------------
// order-preserving image of fp32 in uint32; every NaN is the largest key, as torch.sort orders it
__device__ __forceinline__ unsigned sel_key(float v) {
  const unsigned u = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(unsigned k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// workspace of one selection: hist [4 passes][F][256] uint32 | prefix [F] uint32 | remaining [F] int64
struct SelWs {
  unsigned* hist;
  unsigned* prefix;
  long long* remaining;
};
__host__ __device__ inline SelWs sel_carve(void* ws) {
  SelWs w;
  w.hist = reinterpret_cast<unsigned*>(ws);
  w.remaining = reinterpret_cast<long long*>(w.hist + 4 * DT_FMAX * 256);
  w.prefix = reinterpret_cast<unsigned*>(w.remaining + DT_FMAX);
  return w;
}
constexpr size_t SEL_WS_BYTES = 4 * DT_FMAX * 256 * sizeof(unsigned) + DT_FMAX * sizeof(long long) + DT_FMAX * sizeof(unsigned);

// zero the histograms, prefix = 0, remaining[f] = the 0-based ascending index N - rank (rank 0: index 0, the reference's
// noise_outputs[-0])
__global__ __launch_bounds__(256) void k_sel_init(void* ws, const long long* __restrict__ ranks, long N, int F) {
  const SelWs w = sel_carve(ws);
  for (int i = threadIdx.x; i < 4 * DT_FMAX * 256; i += 256) w.hist[i] = 0u;
  if ((int)threadIdx.x < F) {
    long long r = ranks[threadIdx.x];
    if (r < 0) r = 0;                        // validated by the caller's contract; never index outside [0, N)
    if (r > N) r = N;
    w.prefix[threadIdx.x] = 0u;
    w.remaining[threadIdx.x] = r == 0 ? 0 : N - r;
  }
}

// pass `pass` (0: the top byte): for every rank f, the histogram of this byte over the elements whose higher bytes equal
// prefix[f]
__global__ __launch_bounds__(256) void k_sel_hist(const float* __restrict__ scores, long N, int F, int pass, void* ws) {
  __shared__ unsigned h[DT_FMAX * 256];
  __shared__ unsigned pre[DT_FMAX];
  const SelWs w = sel_carve(ws);
  for (int i = threadIdx.x; i < F * 256; i += 256) h[i] = 0u;
  if ((int)threadIdx.x < F) pre[threadIdx.x] = w.prefix[threadIdx.x];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const unsigned k = sel_key(scores[i]);
    const unsigned d = (k >> shift) & 255u;
    for (int f = 0; f < F; ++f)
      if ((k & himask) == pre[f]) atomicAdd(&h[f * 256 + d], 1u);
  }
  __syncthreads();
  unsigned* g = w.hist + (size_t)pass * DT_FMAX * 256;
  for (int i = threadIdx.x; i < F * 256; i += 256)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

// one workgroup, thread f: walk rank f's 256 bins to the one that holds its index; after the last pass the key is complete
__global__ __launch_bounds__(64) void k_sel_pick(int F, int pass, void* ws, float* __restrict__ thr) {
  const SelWs w = sel_carve(ws);
  const int f = threadIdx.x;
  if (f >= F) return;
  const unsigned* g = w.hist + (size_t)pass * DT_FMAX * 256 + f * 256;
  long long rem = w.remaining[f];
  int d = 0;
  for (; d < 255; ++d) {
    const long long cnt = g[d];
    if (rem < cnt) break;
    rem -= cnt;
  }
  const unsigned p = w.prefix[f] | ((unsigned)d << (24 - 8 * pass));
  w.prefix[f] = p;
  w.remaining[f] = rem;
  if (pass == 3) thr[f] = sel_value(p);
}

// counts[f] += #{scores[i] > thr[f]} (strict; a NaN on either side compares false)
__global__ __launch_bounds__(256) void k_det_counts(const float* __restrict__ scores, long n, const float* __restrict__ thr,
                                                    int F, unsigned long long* __restrict__ counts) {
  __shared__ unsigned cnt[DT_FMAX];
  float t[DT_FMAX];
  unsigned mine[DT_FMAX];
#pragma unroll
  for (int f = 0; f < DT_FMAX; ++f) {
    t[f] = f < F ? thr[f] : __uint_as_float(0x7FC00000u);
    mine[f] = 0u;
  }
  if (threadIdx.x < DT_FMAX) cnt[threadIdx.x] = 0u;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float s = scores[i];
#pragma unroll
    for (int f = 0; f < DT_FMAX; ++f) mine[f] += s > t[f] ? 1u : 0u;
  }
#pragma unroll
  for (int f = 0; f < DT_FMAX; ++f)
    if (mine[f]) atomicAdd(&cnt[f], mine[f]);
  __syncthreads();
  if ((int)threadIdx.x < F && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

static int det_check_shape(const char* who, int B, int d_in, int C) {
  GWW_REQUIRE(B >= 1 && B <= 65536, "%s: B=%d must be 1..65536", who, B);
  GWW_REQUIRE(d_in >= 128 && d_in <= 1280 && d_in % 128 == 0, "%s: d_in=%d must be a multiple of 128 in 128..1280", who, d_in);
  GWW_REQUIRE(C >= 2 && C <= DT_CMAX, "%s: C=%d must be 2..%d", who, C, DT_CMAX);
  return GWW_OK;
}
static bool det_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static size_t det_lds_bytes(int d_in) {
  const int ldA = (d_in > DT_N2 ? d_in : DT_N2) + DT_PAD, ldB = DT_N1 + DT_PAD;
  return (size_t)DT_ROWS * (ldA + ldB) * sizeof(float);
}

}  // namespace gww

using namespace gww;

extern "C" int gww_det_head_forward_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                        const float* w3, const float* b3, const float* w4, const float* b4, const float* w5,
                                        const float* b5, const float* targets, int B, int d_in, int C, float epsilon,
                                        float* h1, float* h2, float* h3, float* h4, float* logits, float* probs,
                                        float* row_loss, float* dz, float* loss, void* stream) {
  GWW_TRY(det_check_shape("gww_det_head_forward_f32", B, d_in, C));
  GWW_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && w4 && b4 && w5 && b5 && targets, "gww_det_head_forward_f32: NULL input");
  GWW_REQUIRE(h1 && h2 && h3 && h4 && logits && probs && row_loss && dz && loss, "gww_det_head_forward_f32: NULL output");
  GWW_REQUIRE(epsilon >= 0.f && epsilon * (float)C < 1.f, "gww_det_head_forward_f32: epsilon=%g must be in [0, 1/C)", (double)epsilon);
  GWW_REQUIRE(det_aligned16(x) && det_aligned16(w1) && det_aligned16(w2) && det_aligned16(w3) && det_aligned16(w4) &&
                  det_aligned16(w5) && det_aligned16(b1) && det_aligned16(b2) && det_aligned16(b3) && det_aligned16(b4) &&
                  det_aligned16(h1) && det_aligned16(h2) && det_aligned16(h3) && det_aligned16(h4),
              "gww_det_head_forward_f32: operands must be 16-byte aligned");
  const size_t lds = det_lds_bytes(d_in);
  hipStream_t s = (hipStream_t)stream;
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_det_fwd<-1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const DetWeights P{w1, b1, w2, b2, w3, b3, w4, b4, w5, b5};
  const DetSaves S{h1, h2, h3, h4, logits, probs, row_loss, dz};
  hipLaunchKernelGGL(k_det_fwd<-1>, dim3((unsigned)cdiv(B, DT_ROWS)), dim3(DT_THREADS), lds, s, x, P, targets, B, d_in, C, epsilon,
                     S, (float*)nullptr, 0L);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_det_mean, dim3(1), dim3(256), 0, s, (const float*)row_loss, B, C, loss);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_det_head_workspace_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * (DT_N1 + DT_N2 + DT_N3 + DT_N4 + C) * sizeof(float);
}

extern "C" int gww_det_head_backward_f32(const float* x, const float* w1, const float* w2, const float* w3, const float* w4,
                                         const float* w5, const float* h1, const float* h2, const float* h3, const float* h4,
                                         const float* dz, const float* dloss, int B, int d_in, int C, float* ws,
                                         size_t ws_bytes, float* dx, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                         float* db3, float* dw4, float* db4, float* dw5, float* db5, void* stream) {
  GWW_TRY(det_check_shape("gww_det_head_backward_f32", B, d_in, C));
  GWW_REQUIRE(x && w1 && w2 && w3 && w4 && w5 && h1 && h2 && h3 && h4 && dz, "gww_det_head_backward_f32: NULL input");
  GWW_REQUIRE(ws && dx && dw1 && db1 && dw2 && db2 && dw3 && db3 && dw4 && db4 && dw5 && db5,
              "gww_det_head_backward_f32: NULL output");
  GWW_REQUIRE(ws_bytes >= gww_det_head_workspace_bytes(B, C), "gww_det_head_backward_f32: workspace of %zu bytes, %zu needed",
              ws_bytes, gww_det_head_workspace_bytes(B, C));
  GWW_REQUIRE(det_aligned16(x) && det_aligned16(w1) && det_aligned16(w2) && det_aligned16(w3) && det_aligned16(w4) &&
                  det_aligned16(w5) && det_aligned16(h1) && det_aligned16(h2) && det_aligned16(h3) && det_aligned16(h4) &&
                  det_aligned16(ws) && det_aligned16(dx) && det_aligned16(dw1) && det_aligned16(dw2) && det_aligned16(dw3) &&
                  det_aligned16(dw4) && det_aligned16(dw5),
              "gww_det_head_backward_f32: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // workspace: dz1 [B, 512] | dz2 [B, 256] | dz3 [B, 128] | dz4 [B, 64] | dz5 [B, C]
  float* dz1 = ws;
  float* dz2 = dz1 + (size_t)B * DT_N1;
  float* dz3 = dz2 + (size_t)B * DT_N2;
  float* dz4 = dz3 + (size_t)B * DT_N3;
  float* dz5 = dz4 + (size_t)B * DT_N4;
  const DetBwdArgs A{w1, w2, w3, w4, w5, h1, h2, h3, h4, dz1, dz2, dz3, dz4, dz5, dx};
  hipLaunchKernelGGL(k_det_bwd_in, dim3((unsigned)cdiv(B, DT_ROWS)), dim3(DT_THREADS), 0, s, dz, dloss, A, B, d_in, C);
  GWW_LAUNCH_CHECK();
  DetWgradArgs W;
  const float* dzs[5] = {dz1, dz2, dz3, dz4, dz5};
  const float* hs[5] = {x, h1, h2, h3, h4};
  float* dws[5] = {dw1, dw2, dw3, dw4, dw5};
  float* dbs[5] = {db1, db2, db3, db4, db5};
  const int Ns[5] = {DT_N1, DT_N2, DT_N3, DT_N4, C}, Ks[5] = {d_in, DT_N1, DT_N2, DT_N3, DT_N4};
  int first = 0;
  for (int i = 0; i < 5; ++i) {
    W.l[i] = DetWgradLayer{dzs[i], hs[i], dws[i], dbs[i], Ns[i], Ks[i], Ks[i] / 64, first};
    first += (int)cdiv(Ns[i], 64) * (Ks[i] / 64);
  }
  hipLaunchKernelGGL(k_det_bwd_w, dim3((unsigned)first), dim3(256), 0, s, W, B);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_det_head_scores_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                       const float* w3, const float* b3, const float* w4, const float* b4, const float* w5,
                                       const float* b5, int B, int d_in, int C, int mode, float* out, long out_stride,
                                       void* stream) {
  GWW_TRY(det_check_shape("gww_det_head_scores_f32", B, d_in, C));
  GWW_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && w4 && b4 && w5 && b5 && out, "gww_det_head_scores_f32: NULL argument");
  GWW_REQUIRE(mode == 0 || mode == 1, "gww_det_head_scores_f32: mode=%d must be 0 (probs[:, 0]) or 1 (z0 - z1)", mode);
  GWW_REQUIRE(mode == 0 || C == 2, "gww_det_head_scores_f32: mode 1 (z0 - z1) needs C = 2, not %d", C);
  GWW_REQUIRE(out_stride >= 1, "gww_det_head_scores_f32: out_stride=%ld must be >= 1", out_stride);
  GWW_REQUIRE(det_aligned16(x) && det_aligned16(w1) && det_aligned16(w2) && det_aligned16(w3) && det_aligned16(w4) &&
                  det_aligned16(w5) && det_aligned16(b1) && det_aligned16(b2) && det_aligned16(b3) && det_aligned16(b4),
              "gww_det_head_scores_f32: operands must be 16-byte aligned");
  const size_t lds = det_lds_bytes(d_in);
  hipStream_t s = (hipStream_t)stream;
  const DetWeights P{w1, b1, w2, b2, w3, b3, w4, b4, w5, b5};
  const DetSaves S{};
  const dim3 grid((unsigned)cdiv(B, DT_ROWS));
  if (mode == 0) {
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_det_fwd<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_det_fwd<0>, grid, dim3(DT_THREADS), lds, s, x, P, (const float*)nullptr, B, d_in, C, 0.f, S, out, out_stride);
  } else {
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_det_fwd<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_det_fwd<1>, grid, dim3(DT_THREADS), lds, s, x, P, (const float*)nullptr, B, d_in, C, 0.f, S, out, out_stride);
  }
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_det_eval_accumulate(const float* probs, const float* targets, const float* row_loss, int B, int C,
                                       long long* correct, double* loss_sum, long long* n, long long* batches, void* stream) {
  GWW_REQUIRE(probs && targets && row_loss && correct && loss_sum && n && batches, "gww_det_eval_accumulate: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= 65536, "gww_det_eval_accumulate: B=%d must be 1..65536", B);
  GWW_REQUIRE(C >= 2 && C <= DT_CMAX, "gww_det_eval_accumulate: C=%d must be 2..%d", C, DT_CMAX);
  hipLaunchKernelGGL(k_det_eval, dim3(1), dim3(256), 0, (hipStream_t)stream, probs, targets, row_loss, B, C, correct, loss_sum, n,
                     batches);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_score_thresholds_workspace_bytes(void) { return SEL_WS_BYTES; }

extern "C" int gww_score_thresholds_f32(const float* scores, long N, const long long* ranks, int F, float* thr, void* ws,
                                        size_t ws_bytes, void* stream) {
  GWW_REQUIRE(scores && ranks && thr && ws, "gww_score_thresholds_f32: NULL argument");
  GWW_REQUIRE(N >= 1 && N <= 2147483647L, "gww_score_thresholds_f32: N=%ld must be 1..2^31-1", N);
  GWW_REQUIRE(F >= 1 && F <= DT_FMAX, "gww_score_thresholds_f32: F=%d must be 1..%d", F, DT_FMAX);
  GWW_REQUIRE(ws_bytes >= SEL_WS_BYTES, "gww_score_thresholds_f32: workspace of %zu bytes, %zu needed", ws_bytes, SEL_WS_BYTES);
  GWW_REQUIRE((((uintptr_t)ws) & 7) == 0, "gww_score_thresholds_f32: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(256), 0, s, ws, ranks, N, F);
  GWW_LAUNCH_CHECK();
  const unsigned blocks = (unsigned)(cdiv(N, 256 * 8) < 1024 ? cdiv(N, 256 * 8) : 1024);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(k_sel_hist, dim3(blocks), dim3(256), 0, s, scores, N, F, pass, ws);
    GWW_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(64), 0, s, F, pass, ws, thr);
    GWW_LAUNCH_CHECK();
  }
  return GWW_OK;
}

extern "C" int gww_detection_counts_f32(const float* scores, long n, const float* thr, int F, long long* counts, void* stream) {
  GWW_REQUIRE(scores && thr && counts, "gww_detection_counts_f32: NULL argument");
  GWW_REQUIRE(n >= 1 && n <= 2147483647L, "gww_detection_counts_f32: n=%ld must be 1..2^31-1", n);
  GWW_REQUIRE(F >= 1 && F <= DT_FMAX, "gww_detection_counts_f32: F=%d must be 1..%d", F, DT_FMAX);
  const unsigned blocks = (unsigned)(cdiv(n, 256 * 8) < 1024 ? cdiv(n, 256 * 8) : 1024);
  hipLaunchKernelGGL(k_det_counts, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scores, n, thr, F,
                     reinterpret_cast<unsigned long long*>(counts));
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
