// Binary head step of the signal-vs-noise trainers (models.one_channel_ligo_binary_classifier: d_in -> 512 -> 256 -> 128 ->
// 64 -> C, models.two_channel_ligo_binary_classifier: d_in -> 1024 -> 512 -> 256 -> C, ReLU between the layers,
// BCEWithLogitsLoss on top) and its inference-only score form.  Conventions of detect.hip: exact fp32, every contraction a
// v_mfma_f32_16x16x4_f32 chain (head_chain.h), no float atomics, every reduction in a fixed order (identical calls give
// identical bits), plain launches, nothing here synchronises.
//   k_bh_fwd         one workgroup per 16 rows walks the layers through LDS; tail (fp64 on the fp32 logits, rounded once):
//                    sigmoid, the row's BCE-with-logits sum, dz = d loss / d logits.  TRAIN false: the logits only
//   k_chain_mean, k_chain_bwd_in<BinTwo, false, true>, k_chain_bwd_w<4>: head_chain.h
// Layout 1 is the detection head's chain, walked by the same chain_fwd: at equal weights its logits are the bits of
// k_det_fwd's, and its backward IS the detection head's (det_chain_backward, detect.hip).  Layout 2 keeps a 1024-wide row in
// LDS, next to which x fits only up to d_in = 1280: its first layer walks x in 512-column chunks (chain_fwd_chunked, the k
// order of chain_fwd) at every d_in, and its backward takes its 98 816 bytes of LDS from the launch.
#include "head_chain.h"

namespace gww {

template <int LAYOUT>
struct BinHead;
template <>
struct BinHead<GWW_BIN_HEAD_ONE> {
  using CH = DetChain;
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

// forward (TRAIN: H and the loss) or scores (H == NULL, loss == NULL, S empty) of one layout
template <int LAYOUT, bool TRAIN>
static int bh_forward(const char* who, const float* x, const gww_mlp_params* P, const gww_mlp_acts* H, float* logits, int B,
                      int d_in, int C, const BinTail& S, float* loss, void* stream) {
  using CH = typename BinHead<LAYOUT>::CH;
  GWW_TRY(chain_check_operands(who, CH::L, x, P, H, nullptr));
  const size_t lds = LAYOUT == GWW_BIN_HEAD_ONE ? chain_lds_bytes<CH>(d_in) : chain_chunked_lds_bytes<CH>();
  return chain_launch_fwd(k_bh_fwd<LAYOUT, TRAIN>, lds, B, S.row_loss, (double)B * (double)C, loss, (hipStream_t)stream, x,
                          chain_fwd_args<CH::L>(P, H ? H->h : nullptr, logits), B, d_in, C, S);
}

}  // namespace gww

using namespace gww;

extern "C" int gww_bin_head_forward_f32(int layout, const float* x, const gww_mlp_params* params, const float* targets, int B,
                                        int d_in, int C, const gww_mlp_acts* acts, float* probs, float* row_loss, float* dz,
                                        float* loss, void* stream) {
  const char* who = "gww_bin_head_forward_f32";
  GWW_TRY(bh_check_shape(who, layout, B, d_in, C));
  GWW_REQUIRE(targets && acts && probs && row_loss && dz && loss, "%s: NULL argument", who);
  const BinTail S{targets, probs, row_loss, dz};
  if (layout == GWW_BIN_HEAD_ONE) return bh_forward<GWW_BIN_HEAD_ONE, true>(who, x, params, acts, acts->logits, B, d_in, C, S, loss, stream);
  return bh_forward<GWW_BIN_HEAD_TWO, true>(who, x, params, acts, acts->logits, B, d_in, C, S, loss, stream);
}

extern "C" size_t gww_bin_head_workspace_bytes(int layout, int B, int C) {
  if (layout == GWW_BIN_HEAD_ONE) return chain_workspace_bytes<BinOne>(B, C);
  if (layout == GWW_BIN_HEAD_TWO) return chain_workspace_bytes<BinTwo>(B, C);
  return 0;
}

extern "C" int gww_bin_head_backward_f32(int layout, const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts,
                                         const float* dz, const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes,
                                         float* dx, const gww_mlp_grads* grads, void* stream) {
  const char* who = "gww_bin_head_backward_f32";
  GWW_TRY(bh_check_shape(who, layout, B, d_in, C));
  hipStream_t s = (hipStream_t)stream;
  if (layout == GWW_BIN_HEAD_ONE) return det_chain_backward(who, x, params, acts, dz, dloss, B, d_in, C, ws, ws_bytes, dx, grads, s);
  return chain_backward<BinTwo, false, true>(who, x, params, acts, dz, dloss, B, d_in, C, 1.f, ws, ws_bytes, dx, grads, s);
}

extern "C" int gww_bin_head_scores_f32(int layout, const float* x, const gww_mlp_params* params, int B, int d_in, int C,
                                       float* logits, void* stream) {
  const char* who = "gww_bin_head_scores_f32";
  GWW_TRY(bh_check_shape(who, layout, B, d_in, C));
  GWW_REQUIRE(logits, "%s: NULL argument", who);
  if (layout == GWW_BIN_HEAD_ONE)
    return bh_forward<GWW_BIN_HEAD_ONE, false>(who, x, params, nullptr, logits, B, d_in, C, BinTail{}, nullptr, stream);
  return bh_forward<GWW_BIN_HEAD_TWO, false>(who, x, params, nullptr, logits, B, d_in, C, BinTail{}, nullptr, stream);
}
