// Detection head step (models.efficiency_classifier / GWWhisperClassifier: d_in -> 512 -> 256 -> 128 -> 64 -> C with ReLU
// between the layers, Softmax(dim=1) and the regularised BCELoss on top), its inference-only score form, and the device
// side of the evaluation / detection-efficiency statistics.  Conventions of classify.hip: exact fp32, every contraction a
// v_mfma_f32_16x16x4_f32 chain, no float atomics, every reduction in a fixed order (identical calls give identical bits),
// plain launches, nothing here synchronises.
//   k_det_fwd        one workgroup per 16 rows walks the five layers through LDS; tail (fp64 on the fp32 logits, rounded
//                    once): softmax, q = eps + (1 - C eps) p, the row's BCE sum, dz = d loss / d logits.  MODE >= 0: no
//                    saves, one score per row (inference)
//   k_chain_mean, k_chain_bwd_in<DetChain, false, false>, k_chain_bwd_w<5>: head_chain.h
//   k_det_eval       one workgroup: correct += #(argmax targets == argmax probs), loss_sum += the batch's mean loss
//   k_sel_*          radix select over the order-preserving integer image of fp32: four 8-bit histogram passes for all
//                    F ranks together (integer atomics only: they commute)
//   k_det_counts     counts[f] += #{scores > thr[f]}
#include "device_sort.h"
#include "head_chain.h"

namespace gww {

static_assert(DetChain::fwd_w(0) == 256 && DetChain::fwd_w(1) == 512 && DetChain::bwd_lds_bytes() == 49664,
              "LDS layout of the detection head (DESIGN.md section 21)");
constexpr int DT_FMAX = 8;                  // false-alarm ranks of one selection

struct DetTail {
  float *probs, *row_loss, *dz;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// MODE -1: the training / evaluation forward (saves, loss tail).  MODE 0: score = probs[:, 0].  MODE 1: score = z0 - z1.
// MODE 2: every column of probs, MODE 3: (z0 - z1, z1 - z0) -- score [B, C] with row pitch score_stride (the efficiency
// study's test stage writes both outputs of the network, test_network.py:89-99).
// LDS: buffer 0 x [16][d_in], then h2 [16][256], then h4 [16][64]; buffer 1 h1 [16][512], then h3 [16][128], then the
// logits [16][C]
template <int MODE>
__global__ __launch_bounds__(CH_THREADS) void k_det_fwd(const float* __restrict__ x, ChainFwdArgs<DetChain::L> P,
                                                        const float* __restrict__ targets, int B, int d_in, int C, float eps,
                                                        DetTail S, float* __restrict__ score, long score_stride) {
  extern __shared__ __attribute__((aligned(16))) float sm_det[];
  const ChainRows Z = chain_fwd<DetChain, (MODE < 0), false>(sm_det, x, P, B, d_in, C, NoDrop{});
  // tail: one wave per row, lane c holds logit c
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = wave; m < CH_ROWS; m += CH_WAVES) {
    const long row = row0 + m;
    if (row >= B) break;                     // uniform per wave
    if (MODE == 1) {
      if (lane == 0) score[row * score_stride] = Z.p[m * Z.ld] - Z.p[m * Z.ld + 1];
      continue;
    }
    if (MODE == 3) {
      if (lane < 2) score[row * score_stride + lane] = Z.p[m * Z.ld + lane] - Z.p[m * Z.ld + 1 - lane];
      continue;
    }
    // Everything behind the logits is fp64, rounded to fp32 once per output: the last layer's bias gradient is a batch sum
    // of dz columns that cancel (for C = 2 the two columns are each other's negatives), which amplifies whatever rounding
    // dz carries; the tail is B x C elements, its cost does not show.
    const float z = lane < C ? Z.p[m * Z.ld + lane] : -INFINITY;
    const float mx = wave_max(z);
    const double e = lane < C ? exp((double)z - (double)mx) : 0.0;
    const double se = wave_sum_f64(e);
    const double p = e / se;
    if (MODE == 0) {
      if (lane == 0) score[row * score_stride] = (float)p;
      continue;
    }
    if (MODE == 2) {
      if (lane < C) score[row * score_stride + lane] = (float)p;
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
    const double rl = wave_sum_f64(el);
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

// ---- backward ----------------------------------------------------------------------------------------------------------
// LDS: buffer 0 dz5 [16][C16], then dz3 [16][128], then dz1 [16][512]; buffer 1 dz4 [16][64], then dz2 [16][256]
int det_chain_backward(const char* who, const float* x, const gww_mlp_params* P, const gww_mlp_acts* H, const float* dz,
                       const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes, float* dx, const gww_mlp_grads* G,
                       hipStream_t s) {
  return chain_backward<DetChain, false, false>(who, x, P, H, dz, dloss, B, d_in, C, 1.f, ws, ws_bytes, dx, G, s);
}

// ---- evaluation accumulate ------------------------------------------------------------------------------------------
// one workgroup: correct += #(argmax targets == argmax probs) (integer LDS atomics: they commute), loss_sum += the batch's
// mean loss as k_chain_mean rounds it to fp32 (the reference sums loss.item() over batches and divides by their number),
// n += B, batches += 1; one writer.
__global__ __launch_bounds__(256) void k_det_eval(const float* __restrict__ probs, const float* __restrict__ targets,
                                                  const float* __restrict__ row_loss, int B, int C,
                                                  long long* __restrict__ correct, double* __restrict__ loss_sum,
                                                  long long* __restrict__ n, long long* __restrict__ batches) {
  __shared__ int cnt;
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
      if (argmax_better(p[j], j, pv, pi)) { pv = p[j]; pi = j; }
      if (argmax_better(t[j], j, tv, ti)) { tv = t[j]; ti = j; }
    }
    mine += pi == ti;
  }
  if (mine) atomicAdd(&cnt, mine);
  const double s = block_sum_f64(row_loss, B);           // its barriers also order cnt
  if (tid == 0) {
    correct[0] += cnt;
    loss_sum[0] += (double)(float)(s / ((double)B * (double)C));
    n[0] += B;
    batches[0] += 1;
  }
}

// ---- rank selection --------------------------------------------------------------------------------------------------
// keys: the order-preserving image of the score (device_sort.h); every NaN is the largest key, 0xFFFFFFFF, as torch.sort
// orders it, and comes back as the canonical NaN

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
    const float v = scores[i];
    const unsigned k = v != v ? 0xFFFFFFFFu : ordered_u32(v);
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
  if (pass == 3) thr[f] = p == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : from_ordered_u32(p);
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

}  // namespace gww

using namespace gww;

extern "C" int gww_det_head_forward_f32(const float* x, const gww_mlp_params* params, const float* targets, int B, int d_in,
                                        int C, float epsilon, const gww_mlp_acts* acts, float* probs, float* row_loss, float* dz,
                                        float* loss, void* stream) {
  const char* who = "gww_det_head_forward_f32";
  GWW_TRY(chain_check_shape(who, B, 65536, d_in, C, 2));
  GWW_REQUIRE(targets && acts && probs && row_loss && dz && loss, "%s: NULL argument", who);
  GWW_TRY(chain_check_operands(who, DetChain::L, x, params, acts, nullptr));
  GWW_REQUIRE(epsilon >= 0.f && epsilon * (float)C < 1.f, "%s: epsilon=%g must be in [0, 1/C)", who, (double)epsilon);
  return chain_launch_fwd(k_det_fwd<-1>, chain_lds_bytes<DetChain>(d_in), B, row_loss, (double)B * (double)C, loss,
                          (hipStream_t)stream, x, chain_fwd_args<DetChain::L>(params, acts->h, acts->logits), targets, B, d_in, C,
                          epsilon, DetTail{probs, row_loss, dz}, (float*)nullptr, 0L);
}

extern "C" size_t gww_det_head_workspace_bytes(int B, int C) { return chain_workspace_bytes<DetChain>(B, C); }

extern "C" int gww_det_head_backward_f32(const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts, const float* dz,
                                         const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes, float* dx,
                                         const gww_mlp_grads* grads, void* stream) {
  GWW_TRY(chain_check_shape("gww_det_head_backward_f32", B, 65536, d_in, C, 2));
  return det_chain_backward("gww_det_head_backward_f32", x, params, acts, dz, dloss, B, d_in, C, ws, ws_bytes, dx, grads,
                            (hipStream_t)stream);
}

// The two score entries: one value per row (k_det_fwd<0 / 1>) or all C of them (`both`, k_det_fwd<2 / 3>).
template <int MODE>
static int det_launch_scores(const float* x, const gww_mlp_params* P, int B, int d_in, int C, float* out, long out_stride,
                             void* stream) {
  return chain_launch_fwd(k_det_fwd<MODE>, chain_lds_bytes<DetChain>(d_in), B, nullptr, 0.0, nullptr, (hipStream_t)stream, x,
                          chain_fwd_args<DetChain::L>(P, nullptr, nullptr), (const float*)nullptr, B, d_in, C, 0.f, DetTail{}, out,
                          out_stride);
}
static int det_scores(const char* who, bool both, const float* x, const gww_mlp_params* P, int B, int d_in, int C, int mode,
                      float* out, long out_stride, void* stream) {
  GWW_TRY(chain_check_shape(who, B, 65536, d_in, C, 2));
  GWW_REQUIRE(out, "%s: NULL argument", who);
  GWW_TRY(chain_check_operands(who, DetChain::L, x, P, nullptr, nullptr));
  GWW_REQUIRE(mode == 0 || mode == 1, "%s: mode=%d must be 0 (%s) or 1 (%s)", who, mode, both ? "probs" : "probs[:, 0]",
              both ? "z0 - z1, z1 - z0" : "z0 - z1");
  GWW_REQUIRE(mode == 0 || C == 2, "%s: mode 1 (%s) needs C = 2, not %d", who, both ? "z0 - z1, z1 - z0" : "z0 - z1", C);
  GWW_REQUIRE(out_stride >= (both ? C : 1), "%s: out_stride=%ld must be >= %d", who, out_stride, both ? C : 1);
  switch (2 * both + mode) {
    case 0: return det_launch_scores<0>(x, P, B, d_in, C, out, out_stride, stream);
    case 1: return det_launch_scores<1>(x, P, B, d_in, C, out, out_stride, stream);
    case 2: return det_launch_scores<2>(x, P, B, d_in, C, out, out_stride, stream);
    default: return det_launch_scores<3>(x, P, B, d_in, C, out, out_stride, stream);
  }
}

extern "C" int gww_det_head_scores_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, int mode, float* out,
                                       long out_stride, void* stream) {
  return det_scores("gww_det_head_scores_f32", false, x, params, B, d_in, C, mode, out, out_stride, stream);
}

extern "C" int gww_det_head_scores2_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, int mode,
                                        float* out, long out_stride, void* stream) {
  return det_scores("gww_det_head_scores2_f32", true, x, params, B, d_in, C, mode, out, out_stride, stream);
}

extern "C" int gww_det_eval_accumulate(const float* probs, const float* targets, const float* row_loss, int B, int C,
                                       long long* correct, double* loss_sum, long long* n, long long* batches, void* stream) {
  GWW_REQUIRE(probs && targets && row_loss && correct && loss_sum && n && batches, "gww_det_eval_accumulate: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= 65536, "gww_det_eval_accumulate: B=%d must be 1..65536", B);
  GWW_REQUIRE(C >= 2 && C <= CH_CMAX, "gww_det_eval_accumulate: C=%d must be 2..%d", C, CH_CMAX);
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
