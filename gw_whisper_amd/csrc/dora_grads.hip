// DoRA parameter gradients on the matrix cores (d = 384 / 512, r = 8), up to three projections that share
// their input in ONE pass -- q, k and v of a layer all read h1 = LN1(x) (peft 0.12.0 tuners/lora/dora.py; the
// reference adapts q/k/v [+ out_proj]: Signal_vs_Noise/src/train.py:230-237, MLGWSC-1/train.py:695).
//
// Per projection p (x [M, d], dy_p, y_p [M, d] bf16; g_p[c] = yscale_p mag_p[c] / nrm_p[c]):
//   u      = x A_p^T                       [M, 8]
//   v_p    = dy_p (g_p . B_p)              [M, 8]
//   dB_p  += scaling g_p[c] (dy_p^T u)     [d, 8]
//   dA_p  += scaling (v_p^T x)             [8, d]
//   dm_p  += (sum_rows dy_p y_p - b_p sum_rows dy_p) / mag_p
// The rank-8 factors make this 2.4 GFLOP per projection against 220 MB of operands: the kernel is HBM-bound
// (x + 2 NP operand matrices, read once) as long as the contractions stay off the VALU, which is where the
// register-blocked kernel of train_ops.hip spends its time.
//
// One workgroup (4 waves) streams 32-row tiles:
//   staging   x, dy_p -> LDS as ONE dual-use image each (row reads AND ds_read_b64_tr_b16 transposed reads,
//             256-byte rows with the chunk XOR of cdna_hip_programming.md T10 (b)); sum dy_p y_p on the fly in the
//             staging threads (a thread keeps one 8-column chunk for the whole kernel)
//   phase A   wave 0: u_all[32 rows][n = 8 p + r] = x A_all^T ; wave 1 + p: v_p -> columns 8 p .. 8 p + 7 of v_all.
//             The weights (bf16) live in registers as B operands for the whole kernel.  u_all / v_all go to LDS
//             as bf16 [n][row].
//   phase B   each wave owns D / 128 column blocks of 32:  dA_all^T[j][n] += x^T[j][rows] v_all[rows][n]   (1 MFMA
//             chain for all projections) and dB_all[c][n] += sum_p dy_p^T[c][rows] u_p*[rows][n], where u_p* is
//             u_all with the lanes outside 8 p .. 8 p + 7 zeroed and lane 24 + p set to 1 -- so column 24 + p of
//             the same accumulator collects sum_rows dy_p (the bias term of dm).
// Accumulators stay in registers over all tiles of the workgroup; each workgroup then stores its partial sums to a
// slab of scratch memory and k_dora_reduce adds the (at most 256) slabs into the gradients.
#include <algorithm>

#include "common.h"

namespace gww {

namespace {
struct DoraProj {
  const float* A;      // [8, d]
  const float* Bm;     // [d, 8]
  const float* mag;    // [d]
  const float* nrm;    // [d]
  const float* bias;   // [d] (of the stored y)
  float* dA;
  float* dB;
  float* dm;
  float yscale, scaling;
  long col_off;        // column offset of this projection inside dY / Y rows
};
struct DoraProjs {
  DoraProj p[3];
};

// byte offset of 16-byte chunk ch (0..15) of row `row` inside a [32][128] bf16 sub-image (256-byte rows)
__device__ __forceinline__ int dual_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4_p;

// A operand (32x32x16) = transposed block: M = column 32 jb + (lane & 31), K = rows row0 + {4 hh + (j & 3) + 8 (j >> 2)}
__device__ __forceinline__ bf16x8 tr_frag_dual(const unsigned char* img, int row0, int jb, int lane) {
  const int hh = lane >> 5, g16 = (lane & 31) >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const unsigned char* sub = img + (jb >> 2) * (32 * 256);
  const int ch = 4 * (jb & 3) + 2 * g16 + (p >> 1);
  const int r = row0 + 4 * hh + q;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_p)(sub + dual_off(r, ch) + 8 * (p & 1)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_p)(sub + dual_off(r + 8, ch) + 8 * (p & 1)));
  bf16x8 f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

__device__ __forceinline__ float bf_lo(unsigned int w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned int w) { return __uint_as_float(w & 0xffff0000u); }
}  // namespace

// WLDS: the phase-A weights live in LDS instead of registers (d = 768: 192 registers of weights beside 192 of
// accumulators would spill)
template <int D, int NP, bool WLDS = false>
__global__ __launch_bounds__(256) void k_dora_grads_mfma(const unsigned short* __restrict__ X, long ldx,
                                                         const unsigned short* __restrict__ dY,
                                                         const unsigned short* __restrict__ Y, long ldy,
                                                         const DoraProjs pr, long M, float* __restrict__ scratch) {
  constexpr int R = 32, CH = D / 8, IMG = R * D * 2, KS = D / 16, JB = D / 128;
  constexpr int RP = D <= 512 ? 4 : 2;   // staging row phases: RP * CH threads load, each its chunk of R / RP rows
  static_assert(D % 128 == 0 && RP * CH <= 256 && NP >= 1 && NP <= 3, "shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* Us = lds + (1 + NP) * IMG;   // [32 n][32 rows] bf16
  unsigned char* Vs = Us + 2048;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, hh = lane >> 5;

  // ---- phase-A weights of this wave as B operands: lane (n, hh), k-step s holds W[k = 16 s + 8 hh + j][n]
  constexpr int WROW = D * 2 + 16;              // LDS weight row (bytes), padded against bank conflicts
  unsigned char* Wl = Vs + 2048;                // WLDS: [8 NP rows of A_all | NP x 8 rows of (g . B)^T], bf16 [row][k]
  bf16x8 wf[WLDS ? 1 : KS];
  const bool w_lane = wave == 0 ? n < 8 * NP : (n >> 3) == wave - 1;          // lanes with a non-zero weight column
  const int w_row = wave == 0 ? (n < 8 * NP ? n : 0) : 8 * NP + 8 * (wave - 1) + (n & 7);
  if constexpr (WLDS) {
    for (int i = tid; i < 8 * NP * D; i += 256) {
      const int row = i / D, k = i - row * D;
      const DoraProj& P = pr.p[row >> 3];
      const int r = row & 7;
      *reinterpret_cast<__bf16*>(Wl + row * WROW + 2 * k) = (__bf16)P.A[(long)r * D + k];
      *reinterpret_cast<__bf16*>(Wl + (8 * NP + row) * WROW + 2 * k) =
          (__bf16)(P.yscale * (P.mag[k] / P.nrm[k]) * P.Bm[(long)k * 8 + r]);
    }
  } else {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) wf[s][j] = (__bf16)0.f;
    if (wave == 0) {
      if (n < 8 * NP) {
        const float* a = pr.p[n >> 3].A + (long)(n & 7) * D + 8 * hh;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(a + 16 * s), hi = *reinterpret_cast<const f32x4*>(a + 16 * s + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { wf[s][j] = (__bf16)lo[j]; wf[s][4 + j] = (__bf16)hi[j]; }
        }
      }
    } else if (wave <= NP) {
      const DoraProj& P = pr.p[wave - 1];
      if ((n >> 3) == wave - 1) {
        const int r = n & 7;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = 16 * s + 8 * hh + j;
            wf[s][j] = (__bf16)(P.yscale * (P.mag[k] / P.nrm[k]) * P.Bm[(long)k * 8 + r]);
          }
      }
    }
  }

  // ---- staging role: 16-byte chunk c8 of rows ph, ph + RP, ... (threads past RP CH idle: D = 384, 768 -> wave 3)
  const bool stager = tid < RP * CH;
  const int c8 = tid % CH, ph = tid / CH;
  const int st_sub = (c8 >> 4) * (32 * 256), st_ch = c8 & 15;
  float dyy[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) dyy[p][j] = 0.f;

  // ---- phase-B role: column blocks jb = wave * JB + i; per-lane selectors of the masked u operand
  f32x16 accA[JB], accB[JB];
#pragma unroll
  for (int i = 0; i < JB; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) { accA[i][j] = 0.f; accB[i][j] = 0.f; }
  unsigned int fill[NP];
  bool own[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    own[p] = (n >> 3) == p;
    fill[p] = n == 24 + p ? 0x3f803f80u : 0u;   // bf16 1.0 pairs
  }
  // lanes of v_all nobody writes only feed ignored output columns, but keep them finite (U and V: 4 KB)
  for (int i = tid; i < 1024; i += 256) reinterpret_cast<unsigned int*>(Us)[i] = 0u;

  const long n_tiles = (M + R - 1) / R;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long r0 = t * R;
    // ---------------- staging
    if (stager) {
      // 2 rows per trip and no unrolling: the compiler would otherwise hoist all 8 rows' loads (7 x 32 registers)
#pragma unroll 1
      for (int qq = 0; qq < R / RP / 2; ++qq) {
        u32x4 vx[2], vd[NP][2], vy[NP][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const long row = r0 + RP * (2 * qq + i) + ph;
          const bool ok = row < M;
          vx[i] = ok ? *reinterpret_cast<const u32x4*>(X + row * ldx + 8 * c8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            const long o = row * ldy + pr.p[p].col_off + 8 * c8;
            vd[p][i] = ok ? *reinterpret_cast<const u32x4*>(dY + o) : u32x4{0u, 0u, 0u, 0u};
            vy[p][i] = ok ? *reinterpret_cast<const u32x4*>(Y + o) : u32x4{0u, 0u, 0u, 0u};
          }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = RP * (2 * qq + i) + ph;
          const int off = st_sub + dual_off(row, st_ch);
          *reinterpret_cast<u32x4*>(lds + off) = vx[i];
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            *reinterpret_cast<u32x4*>(lds + (1 + p) * IMG + off) = vd[p][i];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              dyy[p][2 * w] = fmaf(bf_lo(vd[p][i][w]), bf_lo(vy[p][i][w]), dyy[p][2 * w]);
              dyy[p][2 * w + 1] = fmaf(bf_hi(vd[p][i][w]), bf_hi(vy[p][i][w]), dyy[p][2 * w + 1]);
            }
          }
        }
      }
    }
    __syncthreads();
    // ---------------- phase A: u_all (wave 0) / v_p (wave 1 + p), rows on M, n on the lane
    if (wave <= NP) {
      const unsigned char* img = lds + wave * IMG;
      f32x16 acc;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(img + (s >> 3) * (32 * 256) + dual_off(n, 2 * (s & 7) + hh));
        if constexpr (WLDS) {
          u32x4 wv = *reinterpret_cast<const u32x4*>(Wl + w_row * WROW + (16 * s + 8 * hh) * 2);
          if (!w_lane) wv = u32x4{0u, 0u, 0u, 0u};
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, wv), acc, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, wf[s], acc, 0, 0, 0);
        }
      }
      // acc[4 c + e] = out[row 8 c + 4 hh + e][n]  ->  [n][row] bf16
      if (wave == 0 || (n >> 3) == wave - 1) {
        unsigned char* dst = (wave == 0 ? Us : Vs) + n * 64 + 8 * hh;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          *reinterpret_cast<u32x2*>(dst + 16 * c) = u32x2{pack2bf(acc[4 * c], acc[4 * c + 1]), pack2bf(acc[4 * c + 2], acc[4 * c + 3])};
      }
    }
    __syncthreads();
    // ---------------- phase B
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // B operands: rows 16 ks + {4 hh + (j & 3) + 8 (j >> 2)} of column n
      u32x4 uf, vf;
      {
        const u32x2 u0 = *reinterpret_cast<const u32x2*>(Us + n * 64 + 32 * ks + 8 * hh);
        const u32x2 u1 = *reinterpret_cast<const u32x2*>(Us + n * 64 + 32 * ks + 16 + 8 * hh);
        const u32x2 v0 = *reinterpret_cast<const u32x2*>(Vs + n * 64 + 32 * ks + 8 * hh);
        const u32x2 v1 = *reinterpret_cast<const u32x2*>(Vs + n * 64 + 32 * ks + 16 + 8 * hh);
        uf = u32x4{u0[0], u0[1], u1[0], u1[1]};
        vf = u32x4{v0[0], v0[1], v1[0], v1[1]};
      }
      bf16x8 ub[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        u32x4 m;
#pragma unroll
        for (int w = 0; w < 4; ++w) m[w] = own[p] ? uf[w] : fill[p];
        ub[p] = __builtin_bit_cast(bf16x8, m);
      }
      const bf16x8 vb = __builtin_bit_cast(bf16x8, vf);
#pragma unroll
      for (int i = 0; i < JB; ++i) {
        const int jb = wave * JB + i;
        accA[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_dual(lds, 16 * ks, jb, lane), vb, accA[i], 0, 0, 0);
#pragma unroll
        for (int p = 0; p < NP; ++p)
          accB[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_dual(lds + (1 + p) * IMG, 16 * ks, jb, lane), ub[p],
                                                            accB[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---------------- epilogue: acc[4 c + e] = out[column 32 jb + 8 c + 4 hh + e][n].  Every workgroup leaves its
  // partial sums in its own slab of `scratch` (plain 16-byte stores); k_dora_reduce adds the slabs up.  (fp32
  // atomics straight into dA / dB / dm cost ~300 us per call: 6 M device-scope atomics on 20 k addresses.)
  //   slab: PA [NP][8][D] | PB [NP][8][D] | PS [NP][D] | PY [NP][RP][D]
  float* slab = scratch + (long)blockIdx.x * (NP * D * (17 + RP));
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (own[p] || n == 24 + p) {
      const int r = n & 7;
#pragma unroll
      for (int i = 0; i < JB; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int col = 32 * (wave * JB + i) + 8 * c + 4 * hh;
          const f32x4 va = {accA[i][4 * c], accA[i][4 * c + 1], accA[i][4 * c + 2], accA[i][4 * c + 3]};
          const f32x4 vb = {accB[i][4 * c], accB[i][4 * c + 1], accB[i][4 * c + 2], accB[i][4 * c + 3]};
          if (own[p]) {
            *reinterpret_cast<f32x4*>(slab + (p * 8 + r) * D + col) = va;
            *reinterpret_cast<f32x4*>(slab + NP * 8 * D + (p * 8 + r) * D + col) = vb;
          } else {
            *reinterpret_cast<f32x4*>(slab + 2 * NP * 8 * D + p * D + col) = vb;   // sum_rows dy_p
          }
        }
    }
    if (stager) {
      float* py = slab + 2 * NP * 8 * D + NP * D + (p * RP + ph) * D + 8 * c8;
      *reinterpret_cast<f32x4*>(py) = f32x4{dyy[p][0], dyy[p][1], dyy[p][2], dyy[p][3]};
      *reinterpret_cast<f32x4*>(py + 4) = f32x4{dyy[p][4], dyy[p][5], dyy[p][6], dyy[p][7]};
    }
  }
}

// element e of the slab layout, summed over the nb workgroup slabs, scaled and added to its gradient
template <int D, int NP>
__global__ __launch_bounds__(256) void k_dora_reduce(const float* __restrict__ scratch, int nb, const DoraProjs pr) {
  constexpr int RP = D <= 512 ? 4 : 2;
  constexpr int E = NP * D * (17 + RP);
  __shared__ float part[4][64];
  const int tid = threadIdx.x, el = tid & 63, sl = tid >> 6;
  const int e = blockIdx.x * 64 + el;
  float sum = 0.f;
  if (e < E)
    for (int w = sl; w < nb; w += 4) sum += scratch[(long)w * E + e];
  part[sl][el] = sum;
  __syncthreads();
  if (sl != 0 || e >= E) return;
  sum = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
  if (e < 2 * NP * 8 * D) {
    const bool isB = e >= NP * 8 * D;
    const int q = isB ? e - NP * 8 * D : e;
    const int p = q / (8 * D), r = (q - p * 8 * D) / D, col = q % D;
    const DoraProj& P = pr.p[p];
    if (isB) atomicAdd(P.dB + (long)col * 8 + r, P.scaling * P.yscale * (P.mag[col] / P.nrm[col]) * sum);
    else atomicAdd(P.dA + (long)r * D + col, P.scaling * sum);
  } else {
    const int q = e - 2 * NP * 8 * D;
    if (q < NP * D) {
      const int p = q / D, col = q % D;
      atomicAdd(pr.p[p].dm + col, -pr.p[p].bias[col] * sum / pr.p[p].mag[col]);   // - b sum_rows dy
    } else {
      const int q2 = q - NP * D;
      const int p = q2 / (RP * D), col = q2 % D;
      atomicAdd(pr.p[p].dm + col, sum / pr.p[p].mag[col]);                        // sum_rows dy y
    }
  }
}

// scratch the multi-projection kernel wants: one slab of partial sums per workgroup (at most 256 workgroups)
size_t dora_grads_scratch_bytes(int np, int d) { return (size_t)256 * np * d * 21 * sizeof(float); }   // >= 17 + RP

// np projections (1..3) that read the same X; d in {384, 512}.  Gradients are ACCUMULATED.  scratch (optional):
// dora_grads_scratch_bytes(np, d) bytes of device memory; without it the slabs come from hipMallocAsync.
int launch_dora_grads_multi(const void* X, long ldx, const void* dY, const void* Y, long ldy, int np,
                            const long* col_off, const float* const* bias_st, const float* yscale,
                            const float* scaling, const float* const* A, const float* const* Bm,
                            const float* const* mag, const float* const* nrm, float* const* dA, float* const* dB,
                            float* const* dm, long M, int d, hipStream_t s, void* scratch, size_t scratch_bytes) {
  GWW_REQUIRE(np >= 1 && np <= 3 && (d == 384 || d == 512 || (d == 768 && np == 1)),
              "dora_grads_multi: np=%d d=%d unsupported (d 384 / 512 with up to 3 projections, d 768 with one)", np, d);
  GWW_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0, "dora_grads_multi: row strides must be multiples of 8 elements");
  if (M == 0) return GWW_OK;
  DoraProjs pr{};
  for (int p = 0; p < np; ++p) {
    GWW_REQUIRE(A[p] && Bm[p] && mag[p] && nrm[p] && bias_st[p] && dA[p] && dB[p] && dm[p] && col_off[p] % 8 == 0,
                "dora_grads_multi: bad projection %d", p);
    pr.p[p] = DoraProj{A[p], Bm[p], mag[p], nrm[p], bias_st[p], dA[p], dB[p], dm[p], yscale[p], scaling[p], col_off[p]};
  }
  static const long nb_env = lab_int("GWW_DORA_BLOCKS", 0);   // tuning aid (lab build)
  long nb = cdiv(M, 32);
  const long nb_max = nb_env > 0 && nb_env < 256 ? nb_env : 256;   // one workgroup per CU (LDS); one slab each
  if (nb > nb_max) nb = nb_max;
  const size_t lds = (size_t)(1 + np) * 32 * d * 2 + 4096 + (d > 512 ? (size_t)16 * np * (d * 2 + 16) : 0);
  // per-workgroup partial sums: the caller's scratch (encoder workspace) or a stream-ordered allocation
  const size_t need = dora_grads_scratch_bytes(np, d);
  float* slabs = (float*)scratch;
  bool own_alloc = false;
  if (!slabs || scratch_bytes < need) {
    GWW_HIP(hipMallocAsync((void**)&slabs, need, s));
    own_alloc = true;
  }
  const int n_el = np * d * (17 + (d <= 512 ? 4 : 2));
#define GWW_DGM(DD, NPP)                                                                                            \
  do {                                                                                                              \
    GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dora_grads_mfma<DD, NPP, (DD > 512)>),             \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                             \
    hipLaunchKernelGGL((k_dora_grads_mfma<DD, NPP, (DD > 512)>), dim3((unsigned)nb), dim3(256), lds, s,             \
                       (const unsigned short*)X, ldx, (const unsigned short*)dY, (const unsigned short*)Y, ldy, pr, \
                       M, slabs);                                                                                   \
    hipLaunchKernelGGL((k_dora_reduce<DD, NPP>), dim3((unsigned)cdiv(n_el, 64)), dim3(256), 0, s, slabs, (int)nb,   \
                       pr);                                                                                         \
  } while (0)
  if (d == 768) {
    GWW_DGM(768, 1);
  } else if (d == 384) {
    if (np == 1) GWW_DGM(384, 1); else if (np == 2) GWW_DGM(384, 2); else GWW_DGM(384, 3);
  } else {
    if (np == 1) GWW_DGM(512, 1); else if (np == 2) GWW_DGM(512, 2); else GWW_DGM(512, 3);
  }
#undef GWW_DGM
  GWW_LAUNCH_CHECK();
  if (own_alloc) GWW_HIP(hipFreeAsync(slabs, s));
  return GWW_OK;
}


// ---------------------------------------------------------------------------------------------------------------
// Adapter gradients of any adapted linear layer: rectangular projections (fc1 [4d, d], fc2 [d, 4d]) and every rank
// 1..64 (the kernels above serve r = 8 on [d, d] only).  Same contract as k_dora_grads (x [M, d_in], dy / y [M, d_out]
// bf16 with row strides, bias in stored units, g = yscale mag / nrm, gradients ACCUMULATED), in three launches:
//   prep    Wu = bf16 A [RP][d_in], Wv = bf16 (g . B)^T [RP][d_out]; ranks r .. RP - 1 zero (RP = 32 or 64)
//   uv      u = x Wu^T, v = dy Wv^T  [RP][Mp] bf16, rank-major; 32 rows per wave on the 32x32x16 MFMA: each lane
//           streams 64 contiguous bytes of its row per 64-column step (the contraction's k order is permuted alike
//           in both operands, so a half-wave covers 128 contiguous bytes of a row)
//   outer   one workgroup per (128-column block of x or of dy, row split): the 32-row tile goes through ONE LDS
//           image in the dual layout above and is read transposed (ds_read_b64_tr_b16) as the A operand of
//           dA^T[col][rank] += x^T v  or  dB[col][rank] += dy^T u; the column sums of dy y and dy (dm) ride on the
//           staging threads.  Each workgroup stores its partial sums to the slab of its row split
//   reduce  sums the slabs in a fixed order and adds the scaled sums to dA / dB / dm (one thread per element: no
//           float atomics, two identical calls give identical bits)
// The row-wise contractions need the whole row, the outer products want the columns split across workgroups
// (r (d_in + d_out) fp32 accumulators do not fit one workgroup at r = 64, d = 1280): x and dy are read twice,
// y once.
namespace {
struct AdapterPlan {
  int RP, n_cb, n_rs;
  long Mp, E;                                   // padded rows; floats per slab
  size_t wu, wv, u, v, slab, total;             // byte offsets inside the scratch
};
AdapterPlan adapter_plan(long M, int d_in, int d_out, int r) {
  AdapterPlan p{};
  p.RP = r <= 32 ? 32 : 64;
  p.Mp = (M + 31) / 32 * 32;
  p.n_cb = (d_in + d_out) / 128;
  long rs = cdiv(1024, p.n_cb);                 // ~4 workgroups per CU in the outer-product pass
  rs = std::min(rs, std::min(std::max(p.Mp / 32, 1L), 128L));
  p.n_rs = (int)std::max(rs, 1L);
  p.E = (long)p.RP * (d_in + d_out) + 2L * d_out;
  Arena a;
  p.wu = a.take((size_t)p.RP * d_in * 2);
  p.wv = a.take((size_t)p.RP * d_out * 2);
  p.u = a.take((size_t)p.RP * p.Mp * 2);
  p.v = a.take((size_t)p.RP * p.Mp * 2);
  p.slab = a.take((size_t)p.n_rs * p.E * 4);
  p.total = a.total();
  return p;
}
}  // namespace

__global__ __launch_bounds__(256) void k_adapter_prep(const float* __restrict__ A, const float* __restrict__ Bm,
                                                      const float* __restrict__ mag, const float* __restrict__ nrm,
                                                      float yscale, int r, int RP, int d_in, int d_out,
                                                      __bf16* __restrict__ Wu, __bf16* __restrict__ Wv) {
  const long n_u = (long)RP * d_in, n = n_u + (long)RP * d_out;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    if (i < n_u) {
      const int j = (int)(i / d_in);
      Wu[i] = (__bf16)(j < r ? A[i] : 0.f);
    } else {
      const long q = i - n_u;
      const int j = (int)(q / d_out), c = (int)(q - (long)j * d_out);
      Wv[q] = (__bf16)(j < r ? yscale * (mag[c] / nrm[c]) * Bm[(long)c * r + j] : 0.f);
    }
  }
}

// blockIdx.y = 0: u from x, 1: v from dy.  Rows M .. Mp - 1 come out zero.
template <int NB>
__global__ __launch_bounds__(256) void k_adapter_uv(const unsigned short* __restrict__ X, long ldx,
                                                    const unsigned short* __restrict__ dY, long ldy,
                                                    const __bf16* __restrict__ Wu, const __bf16* __restrict__ Wv,
                                                    int d_in, int d_out, long M, long Mp, unsigned short* __restrict__ U,
                                                    unsigned short* __restrict__ V) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, hh = lane >> 5;
  const long row0 = (long)blockIdx.x * 128 + 32 * wave;
  if (row0 >= Mp) return;
  const bool isv = blockIdx.y == 1;
  const int K = isv ? d_out : d_in;
  const long row = row0 + n;
  const bool ok = row < M;
  const unsigned short* a_ptr = (isv ? dY : X) + (ok ? row : 0L) * (isv ? ldy : ldx) + 32 * hh;
  const __bf16* b_ptr = (isv ? Wv : Wu) + (long)n * K + 32 * hh;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[nb][j] = 0.f;
  // k-step s of the 64-column group k0 holds columns k0 + 32 hh + 8 s .. + 7 in BOTH operands; the next group's
  // operands are loaded before this group's MFMAs (two groups, 128 bytes of the row per lane, in flight)
  u32x4 a[4], b[NB][4];
  auto load = [&](int k0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a[s] = ok ? *reinterpret_cast<const u32x4*>(a_ptr + k0 + 8 * s) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) b[nb][s] = *reinterpret_cast<const u32x4*>(b_ptr + (long)nb * 32 * K + k0 + 8 * s);
    }
  };
  load(0);
  for (int k0 = 0; k0 < K; k0 += 64) {
    u32x4 ac[4], bc[NB][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      ac[s] = a[s];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bc[nb][s] = b[nb][s];
    }
    if (k0 + 64 < K) load(k0 + 64);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ac[s]),
                                                          __builtin_bit_cast(bf16x8, bc[nb][s]), acc[nb], 0, 0, 0);
  }
  // acc[4 c + e] = out[row 8 c + 4 hh + e][rank n]  ->  [rank][row]
  unsigned short* out = isv ? V : U;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<u32x2*>(out + (long)(32 * nb + n) * Mp + row0 + 8 * c + 4 * hh) =
          u32x2{pack2bf(acc[nb][4 * c], acc[nb][4 * c + 1]), pack2bf(acc[nb][4 * c + 2], acc[nb][4 * c + 3])};
}

// blockIdx.x < d_in / 128: column block of x (dA); otherwise of dy / y (dB, dm).  blockIdx.y: row split.
//   slab (floats): dA^T-blocks [RP][d_in] | dB [RP][d_out] | sum dy y [d_out] | sum dy [d_out]
template <int NB>
__global__ __launch_bounds__(256) void k_adapter_outer(const unsigned short* __restrict__ X, long ldx,
                                                       const unsigned short* __restrict__ dY,
                                                       const unsigned short* __restrict__ Y, long ldy,
                                                       const unsigned short* __restrict__ U,
                                                       const unsigned short* __restrict__ V, int d_in, int d_out,
                                                       long M, long Mp, long E, float* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char img[32 * 256];
  __shared__ float red[2][16][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hh = lane >> 5;
  const int nbx = d_in / 128;
  const bool isx = (int)blockIdx.x < nbx;
  const int col0 = 128 * (isx ? (int)blockIdx.x : (int)blockIdx.x - nbx);
  const unsigned short* src = isx ? X : dY;
  const long ld = isx ? ldx : ldy;
  const unsigned short* opB = isx ? V : U;      // dA^T = x^T v,  dB = dy^T u
  const int c8 = tid & 15, ph = tid >> 4;       // staging: chunk c8 of rows ph and ph + 16
  float sy[8], sd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sy[j] = sd[j] = 0.f;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[nb][j] = 0.f;

  const long n_tiles = Mp / 32;
  u32x4 pa[2], py[2], pb[NB][2];
  // the next tile's operands are in flight while the current one is on the matrix cores
  auto fetch = [&](long t) {
    const long r0 = t * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long row = r0 + ph + 16 * i;
      const bool ok = row < M;
      pa[i] = ok ? *reinterpret_cast<const u32x4*>(src + row * ld + col0 + 8 * c8) : u32x4{0u, 0u, 0u, 0u};
      py[i] = (ok && !isx) ? *reinterpret_cast<const u32x4*>(Y + row * ldy + col0 + 8 * c8) : u32x4{0u, 0u, 0u, 0u};
    }
    // B operand rows r0 + 16 ks + {4 hh + (j & 3) + 8 (j >> 2)}: the K order of tr_frag_dual
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const unsigned short* p = opB + (long)(32 * nb + n) * Mp + r0 + 16 * ks + 4 * hh;
        const u32x2 lo = *reinterpret_cast<const u32x2*>(p), hi = *reinterpret_cast<const u32x2*>(p + 8);
        pb[nb][ks] = u32x4{lo[0], lo[1], hi[0], hi[1]};
      }
  };
  long t = blockIdx.y;
  if (t < n_tiles) fetch(t);
  for (; t < n_tiles; t += gridDim.y) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(img + dual_off(ph + 16 * i, c8)) = pa[i];
      if (!isx) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float d0 = bf_lo(pa[i][w]), d1 = bf_hi(pa[i][w]);
          sy[2 * w] = fmaf(d0, bf_lo(py[i][w]), sy[2 * w]);
          sy[2 * w + 1] = fmaf(d1, bf_hi(py[i][w]), sy[2 * w + 1]);
          sd[2 * w] += d0;
          sd[2 * w + 1] += d1;
        }
      }
    }
    u32x4 b[NB][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { b[nb][0] = pb[nb][0]; b[nb][1] = pb[nb][1]; }
    __syncthreads();
    if (t + gridDim.y < n_tiles) fetch(t + gridDim.y);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 a = tr_frag_dual(img, 16 * ks, wave, lane);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, b[nb][ks]), acc[nb], 0, 0, 0);
    }
  }

  // acc[4 c + e] = out[column 32 wave + 8 c + 4 hh + e][rank n]
  float* slab = scratch + (long)blockIdx.y * E;
  float* dst = slab + (isx ? 0L : (long)NB * 32 * d_in);
  const int ldo = isx ? d_in : d_out;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<f32x4*>(dst + (long)(32 * nb + n) * ldo + col0 + 32 * wave + 8 * c + 4 * hh) =
          f32x4{acc[nb][4 * c], acc[nb][4 * c + 1], acc[nb][4 * c + 2], acc[nb][4 * c + 3]};
  if (!isx) {   // column sums of the 16 row phases, in a fixed order
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][ph][8 * c8 + j] = sy[j];
      red[1][ph][8 * c8 + j] = sd[j];
    }
    __syncthreads();
    const int which = tid >> 7, col = tid & 127;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += red[which][q][col];
    slab[(long)NB * 32 * (d_in + d_out) + (long)which * d_out + col0 + col] = sum;
  }
}

// element i of the output (dA | dB | dm), its partial sums of the n_rs slabs: 64 elements per workgroup, four slab
// phases per element (eight loads in flight each), combined in a fixed order
__global__ __launch_bounds__(256) void k_adapter_reduce(const float* __restrict__ scratch, int n_rs, long E, int RP,
                                                        int r, int d_in, int d_out, const float* __restrict__ bias,
                                                        float yscale, float scaling, const float* __restrict__ mag,
                                                        const float* __restrict__ nrm, float* dA, float* dB, float* dm) {
  __shared__ float part[2][4][64];
  const int tid = threadIdx.x, el = tid & 63, sl = tid >> 6;
  const long nA = (long)r * d_in, nBv = (long)r * d_out, n_out = nA + nBv + d_out;
  const long i = (long)blockIdx.x * 64 + el;
  long o = -1, o2 = -1;   // slab offsets of the element (dm: the two column sums)
  if (i < nA) o = i;                                          // slab index j * d_in + c == dA index
  else if (i < nA + nBv) o = (long)RP * d_in + (i - nA);      // [rank][d_out]
  else if (i < n_out) {
    o = (long)RP * (d_in + d_out) + (i - nA - nBv);
    o2 = o + d_out;
  }
  float s1 = 0.f, s2 = 0.f;
  if (o >= 0) {
#pragma unroll 8
    for (int w = sl; w < n_rs; w += 4) {
      s1 += scratch[(long)w * E + o];
      if (o2 >= 0) s2 += scratch[(long)w * E + o2];
    }
  }
  part[0][sl][el] = s1;
  part[1][sl][el] = s2;
  __syncthreads();
  if (sl != 0 || i >= n_out) return;
  const float s = (part[0][0][el] + part[0][1][el]) + (part[0][2][el] + part[0][3][el]);
  if (i < nA) {
    dA[i] += scaling * s;
  } else if (i < nA + nBv) {
    const long q = i - nA;
    const int j = (int)(q / d_out), c = (int)(q - (long)j * d_out);
    dB[(long)c * r + j] += scaling * yscale * (mag[c] / nrm[c]) * s;
  } else {
    const int c = (int)(i - nA - nBv);
    const float sdd = (part[1][0][el] + part[1][1][el]) + (part[1][2][el] + part[1][3][el]);
    dm[c] += (s - bias[c] * sdd) / mag[c];   // (sum dy y - b sum dy) / m
  }
}

size_t adapter_grads_scratch_bytes(long M, int d_in, int d_out, int r) {
  if (M <= 0 || d_in <= 0 || d_out <= 0 || r < 1 || r > 64) return 0;
  return adapter_plan(M, d_in, d_out, r).total;
}

int launch_adapter_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                         float yscale, float scaling, const float* A, const float* Bm, const float* mag,
                         const float* nrm, float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r,
                         hipStream_t s, void* scratch, size_t scratch_bytes) {
  GWW_REQUIRE(r >= 1 && r <= 64, "adapter_grads: rank r=%d is outside 1..64 (the limit of the adapter-gradient kernel)",
              r);
  GWW_REQUIRE(d_in > 0 && d_out > 0 && d_in % 128 == 0 && d_out % 128 == 0,
              "adapter_grads: d_in=%d and d_out=%d must be positive multiples of 128", d_in, d_out);
  GWW_REQUIRE(M >= 0 && ldx >= d_in && ldy >= d_out && ldx % 8 == 0 && ldy % 8 == 0 &&
                  ((((uintptr_t)X) | ((uintptr_t)dY) | ((uintptr_t)Y)) & 15) == 0,
              "adapter_grads: row strides (ldx=%ld ldy=%ld) must be multiples of 8 elements >= d_in / d_out and X / dY / "
              "Y 16-byte aligned", ldx, ldy);
  if (M == 0) return GWW_OK;
  const AdapterPlan p = adapter_plan(M, d_in, d_out, r);
  char* ws = (char*)scratch;
  bool own_alloc = false;
  if (!ws || scratch_bytes < p.total) {
    GWW_HIP(hipMallocAsync((void**)&ws, p.total, s));
    own_alloc = true;
  }
  __bf16* Wu = (__bf16*)(ws + p.wu);
  __bf16* Wv = (__bf16*)(ws + p.wv);
  unsigned short* U = (unsigned short*)(ws + p.u);
  unsigned short* V = (unsigned short*)(ws + p.v);
  float* slabs = (float*)(ws + p.slab);
  const long n_w = (long)p.RP * (d_in + d_out);
  hipLaunchKernelGGL(k_adapter_prep, dim3((unsigned)std::min(cdiv(n_w, 256), 2048L)), dim3(256), 0, s, A, Bm, mag, nrm,
                     yscale, r, p.RP, d_in, d_out, Wu, Wv);
  const dim3 g_uv((unsigned)cdiv(p.Mp, 128), 2), g_out((unsigned)p.n_cb, (unsigned)p.n_rs);
  const auto* x = (const unsigned short*)X;
  const auto* dy = (const unsigned short*)dY;
  const auto* y = (const unsigned short*)Y;
  if (p.RP == 32) {
    hipLaunchKernelGGL(k_adapter_uv<1>, g_uv, dim3(256), 0, s, x, ldx, dy, ldy, Wu, Wv, d_in, d_out, M, p.Mp, U, V);
    hipLaunchKernelGGL(k_adapter_outer<1>, g_out, dim3(256), 0, s, x, ldx, dy, y, ldy, U, V, d_in, d_out, M, p.Mp, p.E,
                       slabs);
  } else {
    hipLaunchKernelGGL(k_adapter_uv<2>, g_uv, dim3(256), 0, s, x, ldx, dy, ldy, Wu, Wv, d_in, d_out, M, p.Mp, U, V);
    hipLaunchKernelGGL(k_adapter_outer<2>, g_out, dim3(256), 0, s, x, ldx, dy, y, ldy, U, V, d_in, d_out, M, p.Mp, p.E,
                       slabs);
  }
  const long n_out = (long)r * (d_in + d_out) + d_out;
  hipLaunchKernelGGL(k_adapter_reduce, dim3((unsigned)cdiv(n_out, 64)), dim3(256), 0, s, slabs, p.n_rs, p.E, p.RP, r,
                     d_in, d_out, bias_st, yscale, scaling, mag, nrm, dA, dB, dm);
  GWW_LAUNCH_CHECK();
  if (own_alloc) GWW_HIP(hipFreeAsync(ws, s));
  return GWW_OK;
}

}  // namespace gww

using namespace gww;

extern "C" int gww_dora_grads_multi(const void* X, long ldx, const void* dY, const void* Y, long ldy, int np,
                                    const long* col_off, const float* const* bias_st, const float* yscale,
                                    const float* scaling, const float* const* A, const float* const* B,
                                    const float* const* mag, const float* const* nrm, float* const* dA,
                                    float* const* dB, float* const* dm, long M, int d, void* stream) {
  GWW_REQUIRE(X && dY && Y && col_off && bias_st && yscale && scaling && A && B && mag && nrm && dA && dB && dm,
              "gww_dora_grads_multi: NULL argument");
  return launch_dora_grads_multi(X, ldx, dY, Y, ldy, np, col_off, bias_st, yscale, scaling, A, B, mag, nrm, dA, dB, dm,
                                 M, d, (hipStream_t)stream, nullptr, 0);
}

extern "C" size_t gww_adapter_grads_scratch_bytes(long M, int d_in, int d_out, int r) {
  return adapter_grads_scratch_bytes(M, d_in, d_out, r);
}

extern "C" int gww_adapter_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                                 float yscale, float scaling, const float* A, const float* B, const float* mag,
                                 const float* nrm, float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r,
                                 void* scratch, size_t scratch_bytes, void* stream) {
  GWW_REQUIRE(X && dY && Y && bias_st && A && B && mag && nrm && dA && dB && dm, "gww_adapter_grads: NULL argument");
  return launch_adapter_grads(X, ldx, dY, Y, ldy, bias_st, yscale, scaling, A, B, mag, nrm, dA, dB, dm, M, d_in, d_out,
                              r, (hipStream_t)stream, scratch, scratch_bytes);
}
