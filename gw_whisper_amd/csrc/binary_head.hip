// Binary head step of the signal-vs-noise trainers (models.one_channel_ligo_binary_classifier: d_in -> 512 -> 256 -> 128 ->
// 64 -> C, models.two_channel_ligo_binary_classifier: d_in -> 1024 -> 512 -> 256 -> C, ReLU between the layers,
// BCEWithLogitsLoss on top) and its inference-only score form.  Conventions of detect.hip: exact fp32, every contraction a
// v_mfma_f32_16x16x4_f32 chain (head_chain.h), no float atomics, every reduction in a fixed order (identical calls give
// identical bits), plain launches, nothing here synchronises.
//   k_bh_fwd         one workgroup per 16 rows walks the layers through LDS; tail (fp64 on the fp32 logits, rounded once):
//                    sigmoid, the row's BCE-with-logits sum, dz = d loss / d logits.  TRAIN false: the logits only
//   k_bh_mean        one workgroup: loss = sum(row_loss) / (B C), fp64 partial sums in a fixed tree
//   k_bh_bwd_in      the same row blocks backwards, every layer's dz left in a workspace, the pooled-token gradient out
//   k_bh_bwd_w       ONE launch for all the layers' dW = dz^T h and db
// Layout 1 is the detection head's chain, walked by the same chain_fwd / chain_bwd: at equal weights its logits are the
// bits of k_det_fwd's.  Layout 2 keeps a 1024-wide row in LDS, next to which x fits only up to d_in = 1280: its first
// layer walks x in 512-column chunks (chain_fwd_chunked, the k order of chain_fwd) at every d_in, and its backward takes its
// 98 816 bytes of LDS from the launch (chain_bwd_at).
#include "head_chain.h"

namespace gww {

template <int LAYOUT>
struct BinHead;
template <>
struct BinHead<GWW_BIN_HEAD_ONE> {
  using CH = Chain<512, 256, 128, 64>;
};
template <>
struct BinHead<GWW_BIN_HEAD_TWO> {
  using CH = Chain<1024, 512, 256>;
};
using BinOne = BinHead<GWW_BIN_HEAD_ONE>::CH;
using BinTwo = BinHead<GWW_BIN_HEAD_TWO>::CH;
static_assert(BinOne::L == 5 && BinOne::bwd_lds_bytes() == 49664, "layout 1 is the detection head's chain");
static_assert(BinTwo::L == 4 && BinTwo::fwd_w(0) == 512 && BinTwo::fwd_w(1) == 1024 && BinTwo::bwd_lds_bytes() == 98816,
              "LDS layout of the two-detector head");
constexpr int BH_LMAX = 5;

struct BinTail {
  const float* targets;
  float *probs, *row_loss, *dz;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int LAYOUT, bool TRAIN>
__global__ __launch_bounds__(CH_THREADS) void k_bh_fwd(const float* __restrict__ x, ChainFwdArgs<BinHead<LAYOUT>::CH::L> P,
                                                       int B, int d_in, int C, BinTail S) {
  using CH = typename BinHead<LAYOUT>::CH;
  extern __shared__ __attribute__((aligned(16))) float sm_bh[];
  ChainRows Z;
  if constexpr (LAYOUT == GWW_BIN_HEAD_ONE)
    Z = chain_fwd<CH, true, false>(sm_bh, x, P, B, d_in, C, NoDrop{});
  else
    Z = chain_fwd_chunked<CH, true>(sm_bh, x, P, B, d_in, C);
  if constexpr (TRAIN) {
    // tail: one wave per row, lane c holds logit c.  Everything behind the logits is fp64, rounded to fp32 once per output
    // (detect.hip: the last layer's bias gradient is a batch sum of dz columns that cancel).
    const long row0 = (long)blockIdx.x * CH_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inv = 1.0 / ((double)B * (double)C);
    for (int m = wave; m < CH_ROWS; m += CH_WAVES) {
      const long row = row0 + m;
      if (row >= B) break;                     // uniform per wave
      const bool on = lane < C;
      const double z = on ? (double)Z.p[m * Z.ld + lane] : 0.0;
      const double t = on ? (double)S.targets[row * C + lane] : 0.0;
      // sigmoid and 1 - sigmoid from e = exp(-|z|), neither by subtraction: p - t = (1 - t) p - t (1 - p) keeps the digits
      // of a confident, correct lane
      const double e = exp(-fabs(z));
      const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
      const double p = z >= 0.0 ? big : small, omp = z >= 0.0 ? small : big;
      const double el = on ? fmax(z, 0.0) - z * t + log1p(e) : 0.0;      // torch's BCEWithLogitsLoss form
      const double rl = wave_sum_f64(el);
      if (on) {
        S.probs[row * C + lane] = (float)p;
        S.dz[row * C + lane] = (float)(((1.0 - t) * p - t * omp) * inv);
      }
      if (lane == 0) S.row_loss[row] = (float)rl;
    }
  }
}

__global__ __launch_bounds__(256) void k_bh_mean(const float* __restrict__ row_loss, int B, int C, float* __restrict__ loss) {
  const double s = block_sum_f64(row_loss, B);
  if (threadIdx.x == 0) loss[0] = (float)(s / ((double)B * (double)C));
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <int LAYOUT>
__global__ __launch_bounds__(CH_THREADS) void k_bh_bwd_in(const float* __restrict__ dz_in, const float* __restrict__ gscale,
                                                          ChainBwdArgs<BinHead<LAYOUT>::CH::L> A, int B, int d_in, int C) {
  using CH = typename BinHead<LAYOUT>::CH;
  if constexpr (LAYOUT == GWW_BIN_HEAD_ONE) {
    chain_bwd<CH, false>(dz_in, gscale, A, B, d_in, C, 1.f);
  } else {
    extern __shared__ __attribute__((aligned(16))) float sm_bh[];
    chain_bwd_at<CH>(sm_bh, dz_in, gscale, A, B, d_in, C);
  }
}

template <int L>
__global__ __launch_bounds__(256) void k_bh_bwd_w(ChainWgradArgs<L> A, int B) {
  chain_bwd_w(A, B);
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int bh_check_shape(const char* who, int layout, int B, int d_in, int C) {
  GWW_REQUIRE(layout == GWW_BIN_HEAD_ONE || layout == GWW_BIN_HEAD_TWO, "%s: layout=%d must be %d (d_in -> 512 -> 256 -> 128 "
              "-> 64 -> C) or %d (d_in -> 1024 -> 512 -> 256 -> C)", who, layout, GWW_BIN_HEAD_ONE, GWW_BIN_HEAD_TWO);
  if (layout == GWW_BIN_HEAD_ONE) return chain_check_shape(who, B, 65536, d_in, C, 1);
  GWW_REQUIRE(B >= 1 && B <= 65536, "%s: B=%d must be 1..65536", who, B);
  GWW_REQUIRE(d_in >= 256 && d_in <= 2560 && d_in % 256 == 0, "%s: d_in=%d must be a multiple of 256 in 256..2560", who, d_in);
  GWW_REQUIRE(C >= 1 && C <= CH_CMAX, "%s: C=%d must be 1..%d", who, C, CH_CMAX);
  return GWW_OK;
}

// the pointers of the layers a layout has (w, b, h of the others are ignored): non-NULL and 16-byte aligned; the last
// layer's bias is read by elements and needs no alignment
static bool bh_layers_ok(int L, const float* const* w, const float* const* b, const float* const* h) {
  for (int i = 0; i < L; ++i) {
    if (!w[i] || (((uintptr_t)w[i]) & 15)) return false;
    if (b && (!b[i] || (i < L - 1 && (((uintptr_t)b[i]) & 15)))) return false;
    if (h && i < L - 1 && (!h[i] || (((uintptr_t)h[i]) & 15))) return false;
  }
  return true;
}

template <int LAYOUT, bool TRAIN>
static int bh_launch_fwd(const float* x, const float* const* w, const float* const* b, float* const* h, float* logits, int B,
                         int d_in, int C, const BinTail& S, hipStream_t s) {
  using CH = typename BinHead<LAYOUT>::CH;
  const size_t lds = LAYOUT == GWW_BIN_HEAD_ONE ? chain_lds_bytes<CH>(d_in) : chain_chunked_lds_bytes<CH>();
  ChainFwdArgs<CH::L> P;
  for (int i = 0; i < CH::L; ++i) {
    P.W[i] = w[i];
    P.b[i] = b[i];
    P.save[i] = i < CH::L - 1 ? (TRAIN ? h[i] : nullptr) : logits;
  }
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bh_fwd<LAYOUT, TRAIN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  hipLaunchKernelGGL((k_bh_fwd<LAYOUT, TRAIN>), dim3((unsigned)cdiv(B, CH_ROWS)), dim3(CH_THREADS), lds, s, x, P, B, d_in, C, S);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

template <int LAYOUT>
static int bh_launch_bwd(const float* x, const float* const* w, const float* const* h, const float* dz, const float* dloss, int B,
                         int d_in, int C, float* ws, float* dx, float* const* dw, float* const* db, hipStream_t s) {
  using CH = typename BinHead<LAYOUT>::CH;
  ChainBwdArgs<CH::L> A;
  for (int i = 0; i < CH::L; ++i) A.W[i] = w[i];
  for (int i = 0; i < CH::L - 1; ++i) A.h[i] = h[i];
  A.dx = dx;
  chain_carve<CH>(ws, B, A.dz);
  const size_t lds = LAYOUT == GWW_BIN_HEAD_ONE ? 0 : CH::bwd_lds_bytes();
  if (lds)
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bh_bwd_in<LAYOUT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  hipLaunchKernelGGL(k_bh_bwd_in<LAYOUT>, dim3((unsigned)cdiv(B, CH_ROWS)), dim3(CH_THREADS), lds, s, dz, dloss, A, B, d_in, C);
  GWW_LAUNCH_CHECK();
  ChainWgradArgs<CH::L> T;
  float* gw[CH::L];
  float* gb[CH::L];
  for (int i = 0; i < CH::L; ++i) {
    gw[i] = dw[i];
    gb[i] = db[i];
  }
  const int grid = chain_wgrad_table<CH>(T, x, A, gw, gb, d_in, C);
  hipLaunchKernelGGL(k_bh_bwd_w<CH::L>, dim3((unsigned)grid), dim3(256), 0, s, T, B);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" int gww_bin_head_forward_f32(int layout, const float* x, const float* w1, const float* b1, const float* w2,
                                        const float* b2, const float* w3, const float* b3, const float* w4, const float* b4,
                                        const float* w5, const float* b5, const float* targets, int B, int d_in, int C,
                                        float* h1, float* h2, float* h3, float* h4, float* logits, float* probs,
                                        float* row_loss, float* dz, float* loss, void* stream) {
  GWW_TRY(bh_check_shape("gww_bin_head_forward_f32", layout, B, d_in, C));
  const int L = layout == GWW_BIN_HEAD_ONE ? BinOne::L : BinTwo::L;
  const float* const w[BH_LMAX] = {w1, w2, w3, w4, w5};
  const float* const b[BH_LMAX] = {b1, b2, b3, b4, b5};
  float* const h[BH_LMAX - 1] = {h1, h2, h3, h4};
  GWW_REQUIRE(x && targets && logits && probs && row_loss && dz && loss, "gww_bin_head_forward_f32: NULL argument");
  GWW_REQUIRE(bh_layers_ok(L, w, b, h) && aligned16({x}),
              "gww_bin_head_forward_f32: x and the %d layers' w, b and h must be non-NULL and 16-byte aligned", L);
  hipStream_t s = (hipStream_t)stream;
  const BinTail S{targets, probs, row_loss, dz};
  if (layout == GWW_BIN_HEAD_ONE)
    GWW_TRY((bh_launch_fwd<GWW_BIN_HEAD_ONE, true>(x, w, b, h, logits, B, d_in, C, S, s)));
  else
    GWW_TRY((bh_launch_fwd<GWW_BIN_HEAD_TWO, true>(x, w, b, h, logits, B, d_in, C, S, s)));
  hipLaunchKernelGGL(k_bh_mean, dim3(1), dim3(256), 0, s, (const float*)row_loss, B, C, loss);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_bin_head_workspace_bytes(int layout, int B, int C) {
  if (layout == GWW_BIN_HEAD_ONE) return chain_workspace_bytes<BinOne>(B, C);
  if (layout == GWW_BIN_HEAD_TWO) return chain_workspace_bytes<BinTwo>(B, C);
  return 0;
}

extern "C" int gww_bin_head_backward_f32(int layout, const float* x, const float* w1, const float* w2, const float* w3,
                                         const float* w4, const float* w5, const float* h1, const float* h2, const float* h3,
                                         const float* h4, const float* dz, const float* dloss, int B, int d_in, int C, float* ws,
                                         size_t ws_bytes, float* dx, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                         float* db3, float* dw4, float* db4, float* dw5, float* db5, void* stream) {
  GWW_TRY(bh_check_shape("gww_bin_head_backward_f32", layout, B, d_in, C));
  const int L = layout == GWW_BIN_HEAD_ONE ? BinOne::L : BinTwo::L;
  const float* const w[BH_LMAX] = {w1, w2, w3, w4, w5};
  const float* const h[BH_LMAX - 1] = {h1, h2, h3, h4};
  float* const dw[BH_LMAX] = {dw1, dw2, dw3, dw4, dw5};
  float* const db[BH_LMAX] = {db1, db2, db3, db4, db5};
  GWW_REQUIRE(x && dz && ws && dx, "gww_bin_head_backward_f32: NULL argument");
  GWW_REQUIRE(bh_layers_ok(L, w, nullptr, h) && bh_layers_ok(L, dw, nullptr, nullptr) && aligned16({x, ws, dx}),
              "gww_bin_head_backward_f32: x, ws, dx and the %d layers' w, h and dw must be non-NULL and 16-byte aligned", L);
  for (int i = 0; i < L; ++i) GWW_REQUIRE(db[i], "gww_bin_head_backward_f32: NULL bias gradient of layer %d", i + 1);
  GWW_REQUIRE(ws_bytes >= gww_bin_head_workspace_bytes(layout, B, C), "gww_bin_head_backward_f32: workspace of %zu bytes, %zu needed",
              ws_bytes, gww_bin_head_workspace_bytes(layout, B, C));
  hipStream_t s = (hipStream_t)stream;
  if (layout == GWW_BIN_HEAD_ONE) return bh_launch_bwd<GWW_BIN_HEAD_ONE>(x, w, h, dz, dloss, B, d_in, C, ws, dx, dw, db, s);
  return bh_launch_bwd<GWW_BIN_HEAD_TWO>(x, w, h, dz, dloss, B, d_in, C, ws, dx, dw, db, s);
}

extern "C" int gww_bin_head_scores_f32(int layout, const float* x, const float* w1, const float* b1, const float* w2,
                                       const float* b2, const float* w3, const float* b3, const float* w4, const float* b4,
                                       const float* w5, const float* b5, int B, int d_in, int C, float* logits, void* stream) {
  GWW_TRY(bh_check_shape("gww_bin_head_scores_f32", layout, B, d_in, C));
  const int L = layout == GWW_BIN_HEAD_ONE ? BinOne::L : BinTwo::L;
  const float* const w[BH_LMAX] = {w1, w2, w3, w4, w5};
  const float* const b[BH_LMAX] = {b1, b2, b3, b4, b5};
  GWW_REQUIRE(x && logits, "gww_bin_head_scores_f32: NULL argument");
  GWW_REQUIRE(bh_layers_ok(L, w, b, nullptr) && aligned16({x}),
              "gww_bin_head_scores_f32: x and the %d layers' w and b must be non-NULL and 16-byte aligned", L);
  hipStream_t s = (hipStream_t)stream;
  const BinTail S{};
  if (layout == GWW_BIN_HEAD_ONE) return bh_launch_fwd<GWW_BIN_HEAD_ONE, false>(x, w, b, nullptr, logits, B, d_in, C, S, s);
  return bh_launch_fwd<GWW_BIN_HEAD_TWO, false>(x, w, b, nullptr, logits, B, d_in, C, S, s);
}
