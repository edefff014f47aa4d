// Glitch-classification head step (models.glitch_classifier: d_in -> 512 -> 256 -> 128 -> C with ReLU + Dropout between
// the layers, CrossEntropyLoss on top) and the evaluation accumulate, all exact fp32: every contraction is a
// v_mfma_f32_16x16x4_f32 chain (bit for bit a k-ordered fmaf chain), no float atomics, every reduction in a fixed order,
// so two identical calls give identical bits.  Plain launches only:
//   k_head_fwd    one workgroup per 16 rows walks the whole chain, activations in LDS, weights streamed from L2;
//                 tail: lse, row loss, argmax, dz = (softmax - onehot) / B
//   k_chain_mean, k_chain_bwd_in<HeadChain, true, false>, k_chain_bwd_w<4>: head_chain.h.  The backward masks dh = dz W by
//                 the stored post-dropout activation
// Dropout is Philox4x32-10 keyed by (seed, step offset, layer, element index): the mask depends on neither the launch
// geometry nor the row blocking.  The backward does not need to regenerate it: the saved activation is the POST-dropout
// one, which is positive exactly where the unit was kept AND the ReLU was open (x > 0 => x / (1 - p) > 0 in fp32).
#include "head_chain.h"

namespace gww {

using HeadChain = Chain<512, 256, 128>;
static_assert(HeadChain::fwd_w(0) == 256 && HeadChain::fwd_w(1) == 512 && HeadChain::bwd_lds_bytes() == 49664,
              "LDS layout of the glitch head (DESIGN.md section 15)");

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

  __device__ __forceinline__ void apply(float (&v)[4], int layer, unsigned idx4) const {
    if (!on) return;
    const u32x4 rw = drop_words(seed, offset, layer, idx4);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = rw[r] < thr ? 0.f : v[r] * scale;
  }
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// LDS: buffer 0 x [16][d_in], then h2 [16][256], then the logits [16][C]; buffer 1 h1 [16][512], then h3 [16][128]
__global__ __launch_bounds__(CH_THREADS) void k_head_fwd(const float* __restrict__ x, ChainFwdArgs<HeadChain::L> P,
                                                         const long long* __restrict__ labels, int B, int d_in, int C,
                                                         HeadDrop dr, float* __restrict__ row_loss,
                                                         long long* __restrict__ pred, float* __restrict__ dz4) {
  extern __shared__ __attribute__((aligned(16))) float sm_head[];
  const ChainRows Z = chain_fwd<HeadChain, true, true>(sm_head, x, P, B, d_in, C, dr);
  // tail: one wave per row, lane c holds logit c
  const long row0 = (long)blockIdx.x * CH_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = wave; m < CH_ROWS; m += CH_WAVES) {
    const long row = row0 + m;
    if (row >= B) break;                     // uniform per wave
    const float z = lane < C ? Z.p[m * Z.ld + lane] : -INFINITY;
    float bv = z;
    int bi = lane < C ? lane : CH_CMAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
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
  __shared__ int cnt[CH_CMAX * CH_CMAX];
  const int tid = threadIdx.x;
  for (int i = tid; i < C * C; i += 256) cnt[i] = 0;
  __syncthreads();
  double s = 0.0;
  for (int r = tid; r < B; r += 256) {
    const float* z = logits + (long)r * C;
    float bv = z[0];
    int bi = 0;
    for (int j = 1; j < C; ++j)
      if (argmax_better(z[j], j, bv, bi)) { bv = z[j]; bi = j; }
    const long long y = labels[r];
    if (y >= 0 && y < C) atomicAdd(&cnt[(int)y * C + bi], 1);
    s += (double)row_loss[r];
  }
  s = block_sum_f64(s);                      // its barriers also order cnt
  for (int i = tid; i < C * C; i += 256)
    if (cnt[i]) confusion[i] += cnt[i];
  if (tid == 0) {
    loss_sum[0] += s;
    n[0] += B;
  }
}

}  // namespace gww

using namespace gww;

extern "C" int gww_head_forward_f32(const float* x, const gww_mlp_params* params, const long long* labels, int B, int d_in,
                                    int C, float p, int train, unsigned long long seed, unsigned long long offset,
                                    const gww_mlp_acts* acts, float* row_loss, long long* pred, float* dz, float* loss,
                                    void* stream) {
  const char* who = "gww_head_forward_f32";
  GWW_TRY(chain_check_shape(who, B, 1024, d_in, C, 1));
  GWW_REQUIRE(labels && acts && row_loss && pred && dz && loss, "%s: NULL argument", who);
  GWW_TRY(chain_check_operands(who, HeadChain::L, x, params, acts, nullptr));
  GWW_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p=%g must be in [0, 1)", who, (double)p);
  HeadDrop dr;
  dr.seed = seed;
  dr.offset = offset;
  dr.on = train && p > 0.f;
  dr.thr = (unsigned)((double)p * 4294967296.0);
  dr.scale = dr.on ? 1.f / (1.f - p) : 1.f;
  return chain_launch_fwd(k_head_fwd, chain_lds_bytes<HeadChain>(d_in), B, row_loss, (double)B, loss, (hipStream_t)stream, x,
                          chain_fwd_args<HeadChain::L>(params, acts->h, acts->logits), labels, B, d_in, C, dr, row_loss, pred, dz);
}

extern "C" int gww_head_backward_f32(const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts, const float* dz,
                                     const float* dloss, int B, int d_in, int C, float p, int train, float* ws, size_t ws_bytes,
                                     float* dx, const gww_mlp_grads* grads, void* stream) {
  const char* who = "gww_head_backward_f32";
  GWW_TRY(chain_check_shape(who, B, 1024, d_in, C, 1));
  GWW_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p=%g must be in [0, 1)", who, (double)p);
  const float scale = (train && p > 0.f) ? 1.f / (1.f - p) : 1.f;
  return chain_backward<HeadChain, true, false>(who, x, params, acts, dz, dloss, B, d_in, C, scale, ws, ws_bytes, dx, grads,
                                                (hipStream_t)stream);
}

extern "C" size_t gww_head_workspace_bytes(int B, int C) { return chain_workspace_bytes<HeadChain>(B, C); }

extern "C" int gww_head_dropout_mask_f32(unsigned long long seed, unsigned long long offset, int layer, int B, int width,
                                         float p, float* mask, void* stream) {
  GWW_REQUIRE(mask, "gww_head_dropout_mask_f32: NULL output");
  GWW_REQUIRE(B >= 1 && B <= 1024 && width >= 4 && width % 4 == 0 && width <= 4096,
              "gww_head_dropout_mask_f32: B=%d must be 1..1024 and width=%d a multiple of 4 up to 4096", B, width);
  GWW_REQUIRE(layer >= 0 && layer < 3, "gww_head_dropout_mask_f32: layer=%d must be 0, 1 or 2", layer);
  GWW_REQUIRE(p >= 0.f && p < 1.f, "gww_head_dropout_mask_f32: dropout p=%g must be in [0, 1)", (double)p);
  GWW_REQUIRE(aligned16({mask}), "gww_head_dropout_mask_f32: mask must be 16-byte aligned");
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
  GWW_REQUIRE(C >= 1 && C <= CH_CMAX, "gww_eval_accumulate: C=%d must be 1..%d", C, CH_CMAX);
  hipLaunchKernelGGL(k_eval_accumulate, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, row_loss, B, C, confusion,
                     loss_sum, n);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
