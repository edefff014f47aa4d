// Attention backward, exact fp32 (the training twin of k_attention_f32 in attention.hip): every contraction on
// v_mfma_f32_32x32x2_f32, which is a k-ordered fmaf chain, so the result matches an fp32 CPU reference to
// accumulation-order noise.  head_dim 64, any H, any T (1, 77, 1500: key / query tails masked).
//
// Layout as the bf16 backward: qkv [B, T, 3 d] (q | k | v, q as stored: pre-scaled by 1/8), ctx / dctx [B, T, d],
// lse [B, H, T] (natural log), dqkv [B, T, 3 d]: the gradient with respect to the STORED q, k, v (the dX GEMM against
// the packed [3 d, d] panel, which carries the 1/8, then gives the gradient of the layer input).
//
// Three launches, no atomics, so two identical calls give identical bits:
//   rowdot   D = rowsum(dO o O) per query row, and a live flag per 32-row query tile (dO not all zero): the pooled last
//            layer's dctx is zero except at row T-1, and its dead tiles (whose lse rows the forward never wrote) are
//            skipped below.
//   dkv      per workgroup 128 keys of one (b, h), 4 waves x 32 keys with K and V in registers; loop over the live
//            32-row query tiles:  S = Q K^T,  P = exp(S - lse),  dV^T += dO^T P,  dP = dO V^T,  dS = P (dP - D),
//            dK^T += Q^T dS.  128 MFMAs per tile and wave.
//   dq       per workgroup 128 queries, 4 waves x 32 queries with Q and dO in registers; loop over 32-key tiles:
//            S^T = K Q^T,  P^T = exp(S^T - lse),  dP^T = V dO^T,  dS^T = P^T (dP^T - D),  dQ^T += (K - kbar)^T dS^T
//            (kbar: the mean key, see the kernel).  96 MFMAs per tile and wave.  Dead waves store zeros.
// v_mfma_f32_32x32x2_f32: A[i = lane&31][k = lane>>5], B[k = lane>>5][j = lane&31]; D register v of lane l holds
// row i = (v&3) + 8 (v>>2) + 4 (l>>5), column j = l&31.
#include "common.h"

namespace gww {

namespace {
constexpr int BDH = 64;          // head_dim
constexpr int BLD = BDH + 1;     // padded fp32 LDS row
constexpr int BQT = 32;          // query rows per tile of the dkv loop / per flag
constexpr int BKB = 128;         // keys (dkv) or queries (dq) per workgroup

__device__ __forceinline__ int mrow(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }
}  // namespace

// D[bh][t] = sum_dh dctx o ctx; flags[bh][t / 32] = 1 when a dctx row of the tile is non-zero.  One workgroup per
// (b, h, 32-row tile): thread = (row tid >> 3, eight columns (tid & 7) * 8).
__global__ __launch_bounds__(256) void k_attn_rowdot_f32(const float* __restrict__ ctx, const float* __restrict__ dctx,
                                                         float* __restrict__ D, int* __restrict__ flags, int T, int H,
                                                         int n_qt) {
  const int qt = blockIdx.x % n_qt;
  const int bh = blockIdx.x / n_qt;
  const int b = bh / H, h = bh - b * H;
  const int d = H * BDH;
  const int tid = threadIdx.x;
  const int t = qt * BQT + (tid >> 3);
  const int c = (tid & 7) * 8;
  float s = 0.f;
  int nz = 0;
  if (t < T) {
    const float* o = ctx + ((long)b * T + t) * d + h * BDH + c;
    const float* g = dctx + ((long)b * T + t) * d + h * BDH + c;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 ov = *reinterpret_cast<const float4*>(o + 4 * i);
      const float4 gv = *reinterpret_cast<const float4*>(g + 4 * i);
      s = fmaf(gv.x, ov.x, s); s = fmaf(gv.y, ov.y, s); s = fmaf(gv.z, ov.z, s); s = fmaf(gv.w, ov.w, s);
      nz |= (gv.x != 0.f) | (gv.y != 0.f) | (gv.z != 0.f) | (gv.w != 0.f);
    }
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  if (t < T && (tid & 7) == 0) D[(long)bh * T + t] = s;
  const int any = __syncthreads_or(nz);
  if (tid == 0) flags[(long)bh * n_qt + qt] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_attn_bwd_dkv_f32(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          const int* __restrict__ flags, float* __restrict__ dqkv, int T,
                                                          int H, int k_blocks, int n_qt) {
  __shared__ float Qs[BQT][BLD];
  __shared__ float Gs[BQT][BLD];   // dO rows
  __shared__ float Ls[BQT], Ds[BQT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kb = blockIdx.x % k_blocks;
  const int bh = blockIdx.x / k_blocks;
  const int b = bh / H, h = bh - b * H;
  const int d = H * BDH;
  const long rs = 3L * d;
  const float* base = qkv + (long)b * T * rs;
  const float* qp = base + h * BDH;
  const float* kp = base + d + h * BDH;
  const float* vp = base + 2 * d + h * BDH;
  const float* gp = dctx + (long)b * T * d + h * BDH;
  const int r = lane & 31, hh = lane >> 5;
  const int key = kb * BKB + wave * 32 + r;
  const int key_ld = key < T ? key : T - 1;
  float kf[32], vf[32];   // K[key = r][dh = 2 s + hh], V likewise
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    kf[s] = kp[(long)key_ld * rs + 2 * s + hh];
    vf[s] = vp[(long)key_ld * rs + 2 * s + hh];
  }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < 16; ++j) dk[n][j] = dv[n][j] = 0.f;

  for (int qt = 0; qt < n_qt; ++qt) {
    if (!flags[(long)bh * n_qt + qt]) continue;   // uniform over the workgroup
    // stage 32 query rows of q and dO (rows past T: zero, lse +inf -> P = 0)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, row = c >> 4, col = (c & 15) * 4;
      const int q = qt * BQT + row;
      float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), gv = qv;
      if (q < T) {
        qv = *reinterpret_cast<const float4*>(qp + (long)q * rs + col);
        gv = *reinterpret_cast<const float4*>(gp + (long)q * d + col);
      }
      Qs[row][col] = qv.x; Qs[row][col + 1] = qv.y; Qs[row][col + 2] = qv.z; Qs[row][col + 3] = qv.w;
      Gs[row][col] = gv.x; Gs[row][col + 1] = gv.y; Gs[row][col + 2] = gv.z; Gs[row][col + 3] = gv.w;
    }
    if (tid < BQT) {
      const int q = qt * BQT + tid;
      Ls[tid] = q < T ? lse[(long)bh * T + q] : INFINITY;
      Ds[tid] = q < T ? D[(long)bh * T + q] : 0.f;
    }
    __syncthreads();
    // S[q][key] = sum_dh Q[q][dh] K[key][dh]
    f32x16 p, dp;
#pragma unroll
    for (int j = 0; j < 16; ++j) p[j] = dp[j] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      p = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[r][2 * s + hh], kf[s], p, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[r][2 * s + hh], vf[s], dp, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int q = mrow(v, hh);
      p[v] = expf(p[v] - Ls[q]);
      dp[v] = p[v] * (dp[v] - Ds[q]);   // dS
    }
    // dV^T[dh][key] += dO^T[dh][q] P[q][key];  dK^T[dh][key] += Q^T[dh][q] dS[q][key]
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int q = mrow(v, hh);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        dv[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[q][32 * n + r], p[v], dv[n], 0, 0, 0);
        dk[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[q][32 * n + r], dp[v], dk[n], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (key < T) {
    float* krow = dqkv + ((long)b * T + key) * rs + d + h * BDH;
    float* vrow = krow + d;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int dh = 32 * n + 8 * c + 4 * hh;
        *reinterpret_cast<float4*>(krow + dh) = make_float4(dk[n][4 * c], dk[n][4 * c + 1], dk[n][4 * c + 2], dk[n][4 * c + 3]);
        *reinterpret_cast<float4*>(vrow + dh) = make_float4(dv[n][4 * c], dv[n][4 * c + 1], dv[n][4 * c + 2], dv[n][4 * c + 3]);
      }
  }
}

__global__ __launch_bounds__(256) void k_attn_bwd_dq_f32(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                         const float* __restrict__ lse, const float* __restrict__ D,
                                                         const int* __restrict__ flags, float* __restrict__ dqkv, int T,
                                                         int H, int q_blocks, int n_qt) {
  __shared__ float Ks[32][BLD];
  __shared__ float Vs[32][BLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qb = blockIdx.x % q_blocks;
  const int bh = blockIdx.x / q_blocks;
  const int b = bh / H, h = bh - b * H;
  const int d = H * BDH;
  const long rs = 3L * d;
  const float* base = qkv + (long)b * T * rs;
  const float* qp = base + h * BDH;
  const float* kp = base + d + h * BDH;
  const float* vp = base + 2 * d + h * BDH;
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * BKB + wave * 32;   // a 32-row flag tile
  const int q = q0 + r;
  const int q_ld = q < T ? q : T - 1;
  const bool live = q0 < T && flags[(long)bh * n_qt + q0 / BQT] != 0;   // uniform over the wave
  int any_live = __syncthreads_or(live ? 1 : 0);

  f32x16 dq[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < 16; ++j) dq[n][j] = 0.f;
  if (any_live) {
    // dQ is accumulated against the CENTRED keys, dQ = sum_k dS_k (K_k - kbar): sum_k dS_k is zero in exact arithmetic, so
    // any kbar gives the same gradient, but in fp32 that sum is rounding noise (P is recomputed from the stored lse, D comes
    // from the forward's O) and the product kbar * noise stays in dQ.  With pretrained weights the keys of a head share a
    // component several times their spread (LayerNorm bias through W_k), which made that term the whole error of dQ (6.7e-5
    // of |dQ| on such keys where the other contractions hold 3e-6).  kbar = the mean key of this (b, h), summed here: one more
    // read of K (L2 resident), no MFMA.  Thread = (rows tid >> 4, tid >> 4 + 16, ...; float4 column tid & 15); Vs is free until
    // the first tile is staged.
    {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = tid >> 4; k < T; k += 16) {
        const float4 kv = *reinterpret_cast<const float4*>(kp + (long)k * rs + (tid & 15) * 4);
        a.x += kv.x; a.y += kv.y; a.z += kv.z; a.w += kv.w;
      }
      const int row = tid >> 4, col = (tid & 15) * 4;
      Vs[row][col] = a.x; Vs[row][col + 1] = a.y; Vs[row][col + 2] = a.z; Vs[row][col + 3] = a.w;
    }
    __syncthreads();
    float kbar[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) a += Vs[i][32 * n + r];
      kbar[n] = a * (1.0f / (float)T);
    }
    __syncthreads();   // (the first tile overwrites Vs)
    float qf[32], gf[32];   // Q[q = r][dh = 2 s + hh], dO likewise
    const float* grow = dctx + ((long)b * T + q_ld) * d + h * BDH;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      qf[s] = qp[(long)q_ld * rs + 2 * s + hh];
      gf[s] = grow[2 * s + hh];
    }
    const float lq = live ? lse[(long)bh * T + q_ld] : 0.f;
    const float Dq = live ? D[(long)bh * T + q_ld] : 0.f;
    const int n_kt = (T + 31) / 32;
    for (int kt = 0; kt < n_kt; ++kt) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i, row = c >> 4, col = (c & 15) * 4;
        int k = kt * 32 + row;
        if (k >= T) k = T - 1;
        const float4 kv = *reinterpret_cast<const float4*>(kp + (long)k * rs + col);
        const float4 vv = *reinterpret_cast<const float4*>(vp + (long)k * rs + col);
        Ks[row][col] = kv.x; Ks[row][col + 1] = kv.y; Ks[row][col + 2] = kv.z; Ks[row][col + 3] = kv.w;
        Vs[row][col] = vv.x; Vs[row][col + 1] = vv.y; Vs[row][col + 2] = vv.z; Vs[row][col + 3] = vv.w;
      }
      __syncthreads();
      if (live) {
        f32x16 p, dp;
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = dp[j] = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          p = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[r][2 * s + hh], qf[s], p, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[r][2 * s + hh], gf[s], dp, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const bool in = kt * 32 + mrow(v, hh) < T;
          const float pv = in ? expf(p[v] - lq) : 0.f;
          dp[v] = pv * (dp[v] - Dq);   // dS^T
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int k = mrow(v, hh);
#pragma unroll
          for (int n = 0; n < 2; ++n)
            dq[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[k][32 * n + r] - kbar[n], dp[v], dq[n], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  if (q < T) {
    float* orow = dqkv + ((long)b * T + q) * rs + h * BDH;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int dh = 32 * n + 8 * c + 4 * hh;
        *reinterpret_cast<float4*>(orow + dh) = make_float4(dq[n][4 * c], dq[n][4 * c + 1], dq[n][4 * c + 2], dq[n][4 * c + 3]);
      }
  }
}

size_t attention_bwd_f32_scratch_words(int B, int T, int H) {
  return (size_t)B * H * (T + (T + BQT - 1) / BQT);
}

int launch_attention_bwd_f32(const float* qkv, const float* ctx, const float* dctx, const float* lse, float* scratch,
                             float* dqkv, int B, int T, int H, hipStream_t s) {
  GWW_REQUIRE(qkv && ctx && dctx && lse && scratch && dqkv, "attention_bwd_f32: NULL operand");
  GWW_REQUIRE(B >= 0 && T > 0 && H > 0, "attention_bwd_f32: bad shape B=%d T=%d H=%d", B, T, H);
  GWW_REQUIRE(((((uintptr_t)qkv) | ((uintptr_t)ctx) | ((uintptr_t)dctx) | ((uintptr_t)dqkv)) & 15) == 0 &&
                  (((uintptr_t)scratch) & 3) == 0,
              "attention_bwd_f32: qkv / ctx / dctx / dqkv must be 16-byte aligned");
  if (B == 0) return GWW_OK;
  const int n_qt = (T + BQT - 1) / BQT, n_b = (T + BKB - 1) / BKB;
  const long bh = (long)B * H;
  GWW_REQUIRE(bh * n_qt < 2147483647L, "attention_bwd_f32: grid too large");
  float* D = scratch;
  int* flags = reinterpret_cast<int*>(scratch + (size_t)bh * T);
  hipLaunchKernelGGL(k_attn_rowdot_f32, dim3((unsigned)(bh * n_qt)), dim3(256), 0, s, ctx, dctx, D, flags, T, H, n_qt);
  hipLaunchKernelGGL(k_attn_bwd_dkv_f32, dim3((unsigned)(bh * n_b)), dim3(256), 0, s, qkv, dctx, lse, D, flags, dqkv, T,
                     H, n_b, n_qt);
  hipLaunchKernelGGL(k_attn_bwd_dq_f32, dim3((unsigned)(bh * n_b)), dim3(256), 0, s, qkv, dctx, lse, D, flags, dqkv, T, H,
                     n_b, n_qt);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" size_t gww_attention_bwd_f32_scratch_bytes(int B, int T, int n_heads) {
  return (B > 0 && T > 0 && n_heads > 0) ? attention_bwd_f32_scratch_words(B, T, n_heads) * 4 : 0;
}

extern "C" int gww_attention_bwd_f32(const float* qkv, const float* ctx, const float* dctx, const float* lse,
                                     float* d_scratch, float* dqkv, int B, int T, int n_heads, void* stream) {
  return launch_attention_bwd_f32(qkv, ctx, dctx, lse, d_scratch, dqkv, B, T, n_heads, (hipStream_t)stream);
}
