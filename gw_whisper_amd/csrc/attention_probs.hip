// Attention probabilities as an output: P[b, h, i, j] = softmax_j(q_i . k_j), fp32 [B, H, T, T] -- HF's eager
// `attn_weights` (HF:modeling_whisper.py eager_attention_forward, before dropout).  The flash-style forward kernels
// (attention.hip) never form P; this kernel recomputes it from the same qkv buffer [B*T, 3d] the forward has just read.
//
// One workgroup = 4 waves = 128 query rows of one (b, h); one wave = 32 query rows, self-contained:
//   pass 1: S^T = K Q^T tile by tile over all T keys, per-lane running max / sum over the lane's 16 keys of each tile,
//           then the lane pair (l, l ^ 32) that shares a query column combines its two partial (max, sum);
//   pass 2: the same S^T tiles again (same instructions, same bits), p = exp(s - max) / sum, stored.
// The "swapped" product puts the query on the lane and 4 consecutive keys in 4 consecutive accumulator registers
// (C/D layout row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col = lane & 31), so each lane stores 16 B of one
// probability row per register group: per key tile a wave writes 32 rows x 128 contiguous bytes.
// K is read straight from global memory into the MFMA operand registers (the 4 waves of a workgroup read the same
// K rows close together in time: L1 / L2 hits), with the next tile's fragment requested before the current MFMAs.
//
// bf16: v_mfma_f32_32x32x16_bf16 on the bf16 q / k the forward used; q carries 1/8 (times log2(e) when q_log2, then
// p = exp2(s - max)).  fp32: v_mfma_f32_32x32x2_f32, q carries 1/8, expf.
// The key index k of the 64-wide dot product is assigned the same way to both operands (lane half hh supplies
// k = 32 hh + ...), which is all the MFMA sum needs.
// Tails: query rows >= T are loaded clamped and not stored; keys >= T are -inf in pass 1 and not stored.  T % 4 == 0
// keeps every 16-byte store inside the row and aligned (T = 1500 at every Whisper size).
// The kernel is bound by its HBM writes (B H T^2 4 bytes); DESIGN.md section 12 has the measured rate.
#include "common.h"

#include <type_traits>

namespace gww {

namespace {

constexpr int PDH = 64;    // head_dim at every Whisper size
constexpr int PQB = 128;   // query rows per workgroup (4 waves x 32)

// bf16: the bare v_exp_f32 (exp2f / expf wrap it in denormal range fix-ups: ~5 instructions per probability; a result
// below 2^-126 flushes to 0 here).  fp32, the parity path: expf.
template <bool BF, bool LOG2>
__device__ __forceinline__ float p_exp(float x) {
  if constexpr (LOG2) return __builtin_amdgcn_exp2f(x);
  else if constexpr (BF) return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
  else return expf(x);
}

// K fragment of one 32-key tile for this lane: key row `key`, dot-product columns [32 hh, 32 hh + 32)
template <bool BF> struct KFrag;
template <> struct KFrag<true> {
  bf16x8 v[4];
  __device__ __forceinline__ void load(const unsigned short* kp, long key, long row_stride, int hh) {
    const u32x4* src = reinterpret_cast<const u32x4*>(kp + key * row_stride + 32 * hh);
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = __builtin_bit_cast(bf16x8, src[s]);
  }
};
template <> struct KFrag<false> {
  float v[32];
  __device__ __forceinline__ void load(const float* kp, long key, long row_stride, int hh) {
    const f32x4* src = reinterpret_cast<const f32x4*>(kp + key * row_stride + 32 * hh);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const f32x4 t = src[s];
      v[4 * s] = t[0]; v[4 * s + 1] = t[1]; v[4 * s + 2] = t[2]; v[4 * s + 3] = t[3];
    }
  }
};

template <bool BF, bool LOG2>
__global__ __launch_bounds__(256) void k_attention_probs(const void* __restrict__ qkv_v, float* __restrict__ probs,
                                                         int T, int H, int q_tiles) {
  using E = typename std::conditional<BF, unsigned short, float>::type;
  const E* qkv = (const E*)qkv_v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qt = blockIdx.x % q_tiles;
  const int bh = blockIdx.x / q_tiles;
  const int b = bh / H, h = bh - b * H;
  const int d = H * PDH;
  const long row_stride = 3L * d;
  const E* base = qkv + (long)b * T * row_stride;
  const E* qp = base + h * PDH;
  const E* kp = base + d + h * PDH;
  const int r = lane & 31, hh = lane >> 5;
  const int q_row = qt * PQB + wave * 32 + r;
  const long q_ld = q_row < T ? q_row : T - 1;

  KFrag<BF> qf;   // Q[q_row][32 hh + ...]: the B operand (same loader as K)
  qf.load(qp, q_ld, row_stride, hh);

  const int n_kt = (T + 31) / 32;
  auto scores = [&](const KFrag<BF>& kf) -> f32x16 {
    f32x16 st;
#pragma unroll
    for (int j = 0; j < 16; ++j) st[j] = 0.f;
    if constexpr (BF) {
#pragma unroll
      for (int s = 0; s < 4; ++s) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.v[s], qf.v[s], st, 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < 32; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.v[s], qf.v[s], st, 0, 0, 0);
    }
    return st;
  };
  auto key_of = [&](int kt, int j) { return kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh; };
  auto kclamp = [&](int kt) -> long { const int k = kt * 32 + r; return k < T ? k : T - 1; };

  // ---- pass 1: per-lane running max / sum over the lane's keys
  float m_run = -INFINITY, l_run = 0.f;
  KFrag<BF> kf, kn;
  kf.load(kp, kclamp(0), row_stride, hh);
  for (int kt = 0; kt < n_kt; ++kt) {
    if (kt + 1 < n_kt) kn.load(kp, kclamp(kt + 1), row_stride, hh);
    f32x16 st = scores(kf);
    if (kt == n_kt - 1 && (T & 31) != 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (key_of(kt, j) >= T) st[j] = -INFINITY;
    }
    float tmax = st[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) tmax = fmaxf(tmax, st[j]);
    const float m_new = fmaxf(m_run, tmax);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;   // a lane with no valid key yet: keep everything 0, not NaN
    float ps[4] = {0.f, 0.f, 0.f, 0.f};   // four independent chains, not one 16-deep one
#pragma unroll
    for (int j = 0; j < 16; ++j) ps[j & 3] += p_exp<BF, LOG2>(st[j] - m_use);
    l_run = l_run * p_exp<BF, LOG2>(m_run - m_use) + ((ps[0] + ps[1]) + (ps[2] + ps[3]));
    m_run = m_new;
    kf = kn;
  }
  // the lane pair (l, l ^ 32) holds the same query column with disjoint keys
  const float m_o = __shfl_xor(m_run, 32, 64), l_o = __shfl_xor(l_run, 32, 64);
  const float m_row = fmaxf(m_run, m_o);
  const float l_row = l_run * p_exp<BF, LOG2>(m_run - m_row) + l_o * p_exp<BF, LOG2>(m_o - m_row);
  const float inv = 1.0f / l_row;

  // ---- pass 2: recompute, normalise, store 16 B per register group
  const bool q_ok = q_row < T;
  float* prow = probs + ((size_t)bh * T + (q_ok ? q_row : 0)) * (size_t)T;
  kf.load(kp, kclamp(0), row_stride, hh);
  for (int kt = 0; kt < n_kt; ++kt) {
    if (kt + 1 < n_kt) kn.load(kp, kclamp(kt + 1), row_stride, hh);
    const f32x16 st = scores(kf);
    if (q_ok) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int key = key_of(kt, 4 * g);
        if (key < T) {   // T % 4 == 0: the 4 keys of a group are all valid or all past the end
          f32x4 p;
#pragma unroll
          for (int c = 0; c < 4; ++c) p[c] = p_exp<BF, LOG2>(st[4 * g + c] - m_row) * inv;
          *reinterpret_cast<f32x4*>(prow + key) = p;
        }
      }
    }
    kf = kn;
  }
}

}  // namespace

int launch_attention_probs(const void* qkv, bool bf16, bool q_log2, float* probs, int B, int T, int H, hipStream_t s) {
  GWW_REQUIRE(B >= 0 && T > 0 && H > 0, "attention_probs: bad shape B=%d T=%d H=%d", B, T, H);
  GWW_REQUIRE(T % 4 == 0, "attention_probs: T=%d must be a multiple of 4 (16-byte row stores)", T);
  GWW_REQUIRE(bf16 || !q_log2, "attention_probs: q in log2 units is a bf16-path convention");
  if (B == 0) return GWW_OK;   // an empty batch has no storage: its pointers may be NULL
  GWW_REQUIRE(qkv && probs, "attention_probs: NULL operand");
  GWW_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)probs) & 15) == 0, "attention_probs: 16-byte alignment");
  const int q_tiles = (T + PQB - 1) / PQB;
  const long blocks = (long)q_tiles * B * H;
  GWW_REQUIRE(blocks < 2147483647L, "attention_probs: grid too large");
  if (bf16 && q_log2)
    hipLaunchKernelGGL((k_attention_probs<true, true>), dim3((unsigned)blocks), dim3(256), 0, s, qkv, probs, T, H, q_tiles);
  else if (bf16)
    hipLaunchKernelGGL((k_attention_probs<true, false>), dim3((unsigned)blocks), dim3(256), 0, s, qkv, probs, T, H, q_tiles);
  else
    hipLaunchKernelGGL((k_attention_probs<false, false>), dim3((unsigned)blocks), dim3(256), 0, s, qkv, probs, T, H, q_tiles);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" int gww_attention_probs_bf16(const void* qkv, int q_log2, float* probs, int B, int T, int n_heads, void* stream) {
  return launch_attention_probs(qkv, true, q_log2 != 0, probs, B, T, n_heads, (hipStream_t)stream);
}
extern "C" int gww_attention_probs_f32(const float* qkv, float* probs, int B, int T, int n_heads, void* stream) {
  return launch_attention_probs(qkv, false, false, probs, B, T, n_heads, (hipStream_t)stream);
}
