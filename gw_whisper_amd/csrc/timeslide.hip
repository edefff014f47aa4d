// Search background from time slides: the detectors of GWWhisperClassifier only meet in the head,
// whose first Linear splits over the concatenated tokens as W1 = [W1_0 | W1_1 | ...].  With the per-detector partial
// products P[g] = tok_g W1_g^T (+ b1 in detector 0) computed once per window, the score of the pair (detector-0 window i,
// detector-g window (i + g o) mod N) is relu(sum_g P[g][.]) through layers 2..5 of the head.
//   k_slide_scores   one workgroup per 16 consecutive windows i of ONE slide: gathers and sums the D partial rows into the
//                    chain's first LDS buffer (the circular wrap may fall inside the tile), walks 512 -> 256 -> 128 -> 64
//                    -> C with head_chain.h's chain_layer_fwd, writes one score per row.  Exact fp32, every contraction
//                    a v_mfma_f32_16x16x4_f32 chain, no atomics: two calls give identical bits, and a slide's row does
//                    not depend on which other slides share the launch.
//   k_cluster_slides one wave per slide: cluster_wave.h over row s of the scores, the times shared
#include "cluster_wave.h"
#include "head_chain.h"

namespace gww {

using SlideChain = Chain<256, 128, 64>;     // layers 2..5 of the search head; layer 1 is the partials
constexpr int SL_DIN = 512;                 // width of the partials
constexpr int SL_LD0 = SL_DIN + CH_PAD, SL_LD1 = SlideChain::fwd_w(1) + CH_PAD;
static_assert(SlideChain::L == 4 && SlideChain::fwd_w(0) == 128 && SlideChain::fwd_w(1) == 256 && SL_DIN >= SlideChain::fwd_w(0),
              "LDS layout of the slide head (DESIGN.md section 26)");
constexpr int SL_DMAX = 4;

// MODE 0: score = z[0] (the head without its Softmax).  MODE 1: score = softmax(z)[0].
// LDS: buffer 0 relu(sum of partials) [16][512], then h3 [16][128], then the logits [16][C]; buffer 1 h2 [16][256], then
// h4 [16][64]
template <int MODE>
__global__ __launch_bounds__(CH_THREADS) void k_slide_scores(const float* __restrict__ P, ChainFwdArgs<SlideChain::L> A,
                                                             const long long* __restrict__ offsets, long N, int D, int C,
                                                             float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float sm[CH_ROWS * (SL_LD0 + SL_LD1)];
  float* const buf[2] = {sm, sm + CH_ROWS * SL_LD0};
  constexpr int ld[2] = {SL_LD0, SL_LD1};
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int slide = blockIdx.y;
  long o = offsets[slide] % N;               // the wrapper checked 0 <= o < N; whatever arrives, no index leaves [0, N)
  if (o < 0) o += N;
  constexpr int d4 = SL_DIN / 4;
  for (int i = threadIdx.x; i < CH_ROWS * d4; i += CH_THREADS) {
    const int m = i / d4, k = (i - m * d4) * 4;
    const long row = row0 + m;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      v = *reinterpret_cast<const float4*>(P + row * SL_DIN + k);          // detector 0 is never moved
      long j = row;
      for (int g = 1; g < D; ++g) {
        j += o;
        if (j >= N) j -= N;                  // j, o < N: one subtraction is the modulus
        const float4 p = *reinterpret_cast<const float4*>(P + ((long)g * N + j) * SL_DIN + k);
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
      }
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    *reinterpret_cast<float4*>(buf[0] + m * ld[0] + k) = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SlideChain::L - 1; ++i) {
    chain_layer_fwd<true, false>(buf[i & 1], ld[i & 1], buf[(i + 1) & 1], ld[(i + 1) & 1], A.W[i], A.b[i],
                                 SlideChain::in(i, SL_DIN), SlideChain::out(i), i, NoDrop{}, (float*)nullptr, row0, 0);
    __syncthreads();
  }
  constexpr int l = SlideChain::L - 1;
  chain_layer_fwd<false, false>(buf[l & 1], ld[l & 1], buf[(l + 1) & 1], ld[(l + 1) & 1], A.W[l], A.b[l],
                                SlideChain::in(l, SL_DIN), C, l, NoDrop{}, (float*)nullptr, row0, 0);
  __syncthreads();
  const float* Z = buf[(l + 1) & 1];
  constexpr int ldz = ld[(l + 1) & 1];
  // tail: one wave per row, lane c holds logit c
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* out = scores + (long)slide * N;
  for (int m = wave; m < CH_ROWS; m += CH_WAVES) {
    const long row = row0 + m;
    if (row >= N) break;                     // uniform per wave
    if (MODE == 0) {
      if (lane == 0) out[row] = Z[m * ldz];
      continue;
    }
    // as k_det_fwd: fp64 on the fp32 logits, rounded once
    const float z = lane < C ? Z[m * ldz + lane] : -INFINITY;
    const float mx = wave_max(z);
    const double e = lane < C ? exp((double)z - (double)mx) : 0.0;
    const double se = wave_sum_f64(e);
    if (lane == 0) out[row] = (float)(e / se);
  }
}

__global__ __launch_bounds__(64) void k_cluster_slides(const double* __restrict__ times, const float* __restrict__ scores,
                                                       long n, float trigger_threshold, double cluster_threshold,
                                                       double* __restrict__ out_t, float* __restrict__ out_v,
                                                       int* __restrict__ out_count, int max_clusters) {
  const long s = blockIdx.x;
  cluster_wave(times, scores + s * n, n, trigger_threshold, cluster_threshold, out_t + s * max_clusters,
               out_v + s * max_clusters, out_count + s, max_clusters);
}

}  // namespace gww

using namespace gww;

extern "C" int gww_slide_scores_f32(const float* P, const float* w2, const float* b2, const float* w3, const float* b3,
                                    const float* w4, const float* b4, const float* w5, const float* b5,
                                    const long long* offsets, long N, int D, int S, int C, int mode, float* scores,
                                    void* stream) {
  GWW_REQUIRE(P && w2 && b2 && w3 && b3 && w4 && b4 && w5 && b5 && offsets && scores, "gww_slide_scores_f32: NULL argument");
  GWW_REQUIRE(N >= 1 && N <= 2147483647L, "gww_slide_scores_f32: N=%ld must be 1..2^31-1", N);
  GWW_REQUIRE(D >= 2 && D <= SL_DMAX, "gww_slide_scores_f32: D=%d detectors, must be 2..%d", D, SL_DMAX);
  GWW_REQUIRE(S >= 1 && S <= 65535, "gww_slide_scores_f32: S=%d slides, must be 1..65535", S);
  GWW_REQUIRE(C >= 1 && C <= CH_CMAX, "gww_slide_scores_f32: C=%d must be 1..%d", C, CH_CMAX);
  GWW_REQUIRE(mode == 0 || mode == 1, "gww_slide_scores_f32: mode=%d must be 0 (z[0]) or 1 (softmax(z)[0])", mode);
  GWW_REQUIRE(mode == 0 || C >= 2, "gww_slide_scores_f32: mode 1 (softmax) needs C >= 2, not %d", C);
  GWW_REQUIRE(aligned16({P, w2, w3, w4, w5, b2, b3, b4}), "gww_slide_scores_f32: operands must be 16-byte aligned");
  const ChainFwdArgs<SlideChain::L> A{{w2, w3, w4, w5}, {b2, b3, b4, b5}, {}};
  const dim3 grid((unsigned)cdiv(N, CH_ROWS), (unsigned)S);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL(k_slide_scores<0>, grid, dim3(CH_THREADS), 0, s, P, A, offsets, N, D, C, scores);
  else
    hipLaunchKernelGGL(k_slide_scores<1>, grid, dim3(CH_THREADS), 0, s, P, A, offsets, N, D, C, scores);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_cluster_slides_f64(const double* times, const float* scores, long N, int S, float trigger_threshold,
                                      double cluster_threshold, double* out_times, float* out_vals, int* out_count,
                                      int max_clusters, void* stream) {
  GWW_REQUIRE(times && scores && out_count && (max_clusters == 0 || (out_times && out_vals)),
              "gww_cluster_slides_f64: NULL argument");
  GWW_REQUIRE(N >= 1 && N <= 2147483647L, "gww_cluster_slides_f64: N=%ld must be 1..2^31-1", N);
  GWW_REQUIRE(S >= 1 && S <= 65535, "gww_cluster_slides_f64: S=%d slides, must be 1..65535", S);
  GWW_REQUIRE(max_clusters >= 0, "gww_cluster_slides_f64: max_clusters=%d is negative", max_clusters);
  hipLaunchKernelGGL(k_cluster_slides, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, times, scores, N, trigger_threshold,
                     cluster_threshold, out_times, out_vals, out_count, max_clusters);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
