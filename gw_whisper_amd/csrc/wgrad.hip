// Weight-gradient GEMM of the full fine-tuning step:
//     dW[N, K] += alpha * sum_m dY[m, n] X[m, k]          db[N] += alpha * sum_m dY[m, n]
// dY, X bf16 row-major with row strides ldy / ldx; dW, db fp32, ACCUMULATED into (the backward's contract).
//
// Unlike every other GEMM here the reduction index is the ROW index of both operands.  Both tiles are staged in
// LDS as they lie in HBM ([m][n] and [m][k], 16-byte loads) and both MFMA operands are read column-wise with
// ds_read_b64_tr_b16, which delivers 4 consecutive m of one column per lane.  The LDS image of a 64-row chunk is
// [column block of 32][64 rows][32 columns] bf16 (64-byte rows): the four rows one 32-lane half reads with a
// transposed read cover the 64 banks exactly once, so the reads are conflict-free without a swizzle.
//
// Tiling: a 256-thread workgroup owns a 128 (n) x 128 (k) tile of dW and one slice of M; its four waves own 64 x 64
// each (2 x 2 v_mfma_f32_32x32x16_bf16 accumulators).  M is split across workgroups so that the grid fills the
// chip; every slice writes an fp32 partial slab, and a second launch sums the slabs in slice order (deterministic:
// no float atomics, two identical calls give identical bits) and adds alpha * sum into dW / db.  Ragged rows,
// n >= N and k >= K are zero-filled in LDS (the transposed read needs EXEC all ones: pad, don't mask).
//
// Strided im2col views: conv2 = dz2^T view(c1, ldx = 2 d, K = 3 d), conv1 = dz1^T view(melT, ldx = C, K = 256).  The
// reducer then maps the tap-major column k = tap * cin + c to HF's [out, in, 3] layout and drops k >= 3 cin.
#include "common.h"

namespace gww {

namespace {
constexpr int WG_BN = 128, WG_BK = 128, WG_CM = 64, WG_THREADS = 256;
constexpr int WG_OP_BYTES = 4 * WG_CM * 64;            // one operand's image of a chunk: 4 column blocks x 64 rows x 64 B
constexpr int WG_STAGE_BYTES = 2 * WG_OP_BYTES;        // dY image | X image
constexpr int WG_LDS_BYTES = 2 * WG_STAGE_BYTES;       // double buffered: 64 KiB

struct WgradPlan {
  int tiles_n, tiles_k, slices;
  long rows_per_slice;
};

WgradPlan wgrad_plan(long M, int N, int K) {
  WgradPlan p{};
  p.tiles_n = (int)cdiv(N, WG_BN);
  p.tiles_k = (int)cdiv(K, WG_BK);
  const long tiles = (long)p.tiles_n * p.tiles_k;
  // about two workgroups per CU (256 CUs), each slice at least 256 rows, at most 64 slices
  long s = cdiv(512, tiles);
  const long smax = cdiv(M > 0 ? M : 1, 256);
  if (s > smax) s = smax;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  p.rows_per_slice = cdiv(cdiv(M > 0 ? M : 1, s), WG_CM) * WG_CM;
  p.slices = (int)cdiv(M > 0 ? M : 1, p.rows_per_slice);
  return p;
}
}  // namespace

size_t wgrad_workspace_bytes(long M, int N, int K) {
  const WgradPlan p = wgrad_plan(M, N, K);
  return ((size_t)p.slices * N * K + (size_t)p.slices * N) * 4 + 256;
}

typedef bf16x4 __attribute__((address_space(3)))* lds_bf16x4_ptr;

// grid (tiles_k, tiles_n, slices).  part: [slices][N][K] fp32; dbpart (or null): [slices][N] fp32
__global__ __launch_bounds__(WG_THREADS) void k_wgrad_bf16(const unsigned short* __restrict__ dY, long ldy,
                                                           const unsigned short* __restrict__ X, long ldx, long M, int N,
                                                           int K, long rows_per_slice, float* __restrict__ part,
                                                           float* __restrict__ dbpart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int n0 = blockIdx.y * WG_BN, k0 = blockIdx.x * WG_BK;
  const long m_beg = (long)blockIdx.z * rows_per_slice;
  long m_end = m_beg + rows_per_slice;
  if (m_end > M) m_end = M;
  const bool want_db = dbpart != nullptr && blockIdx.x == 0;

  // staging: chunk of 64 rows x 128 columns per operand = 1024 pieces of 8 columns; thread owns pieces tid + 256 i
  // (row = piece >> 4, 8-column chunk c = piece & 15)
  u32x4 ry[4], rx[4];
  auto load = [&](long m0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = tid + WG_THREADS * i;
      const int r = piece >> 4, c = piece & 15;
      const long m = m0 + r;
      const int n = n0 + 8 * c, k = k0 + 8 * c;
      ry[i] = (m < m_end && n < N) ? *reinterpret_cast<const u32x4*>(dY + m * ldy + n) : u32x4{0u, 0u, 0u, 0u};
      rx[i] = (m < m_end && k < K) ? *reinterpret_cast<const u32x4*>(X + m * ldx + k) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto store = [&](int buf) {
    unsigned char* st = smem + buf * WG_STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = tid + WG_THREADS * i;
      const int r = piece >> 4, c = piece & 15;
      const int off = (c >> 2) * (WG_CM * 64) + r * 64 + (c & 3) * 16;
      *reinterpret_cast<u32x4*>(st + off) = ry[i];
      *reinterpret_cast<u32x4*>(st + WG_OP_BYTES + off) = rx[i];
    }
  };

  // transposed-read address of this lane inside one column block: group g = lane / 16 takes columns 16 (g & 1) ..
  // + 15 and rows 8 (g >> 1) + 4 h + q of a 16-row k step; lane 4 q + p of the group addresses row q, columns 4 p .. 4 p + 3
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int tr_off = (8 * (g >> 1) + q) * 64 + (16 * (g & 1) + 4 * p) * 2;

  f32x16 acc[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
  // bias: thread owns column pair 2 (tid & 63) + {0, 1} and rows 16 (tid >> 6) .. + 15 of each chunk
  float bs0 = 0.f, bs1 = 0.f;

  const long n_chunks = m_end > m_beg ? (m_end - m_beg + WG_CM - 1) / WG_CM : 0;
  if (n_chunks > 0) {
    load(m_beg);
    store(0);
    __syncthreads();
  }
  for (long it = 0; it < n_chunks; ++it) {
    const int buf = (int)(it & 1);
    if (it + 1 < n_chunks) load(m_beg + (it + 1) * WG_CM);
    const unsigned char* st = smem + buf * WG_STAGE_BYTES;
#pragma unroll
    for (int s = 0; s < WG_CM / 16; ++s) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned char* a = st + (2 * wn + j) * (WG_CM * 64) + 16 * s * 64 + tr_off;
        const unsigned char* b = st + WG_OP_BYTES + (2 * wk + j) * (WG_CM * 64) + 16 * s * 64 + tr_off;
        const bf16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)a);
        const bf16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(a + 4 * 64));
        const bf16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)b);
        const bf16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(b + 4 * 64));
        af[j] = bf16x8{alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
        bf[j] = bf16x8{blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[j], bf[i], acc[j][i], 0, 0, 0);
    }
    if (want_db) {   // column sums of the dY image already in LDS (zero-filled rows add nothing)
      const int col = 2 * (tid & 63);
      const unsigned char* a = st + (col >> 5) * (WG_CM * 64) + (col & 31) * 2;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned int v = *reinterpret_cast<const unsigned int*>(a + (16 * (tid >> 6) + r) * 64);
        bs0 += bf2f((unsigned short)(v & 0xffff));
        bs1 += bf2f((unsigned short)(v >> 16));
      }
    }
    if (it + 1 < n_chunks) store(buf ^ 1);
    __syncthreads();
  }

  // partial slab: lane holds column k = l % 32 and rows n = 8 (r / 4) + 4 (l / 32) + r % 4 of each 32 x 32 block
  float* slab = part + (size_t)blockIdx.z * N * K;
  const int h = lane >> 5, cl = lane & 31;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = k0 + 64 * wk + 32 * i + cl;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + 64 * wn + 32 * j + 8 * (r >> 2) + 4 * h + (r & 3);
        if (n < N && k < K) slab[(size_t)n * K + k] = acc[j][i][r];
      }
    }
  if (want_db) {   // the four row groups of a column pair, in fixed order, through LDS
    float* red = reinterpret_cast<float*>(smem);
    red[tid * 2] = bs0;
    red[tid * 2 + 1] = bs1;
    __syncthreads();
    if (tid < 64) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        s0 += red[(tid + 64 * w) * 2];
        s1 += red[(tid + 64 * w) * 2 + 1];
      }
      const int n = n0 + 2 * tid;
      if (n < N) {
        dbpart[(size_t)blockIdx.z * N + n] = s0;
        dbpart[(size_t)blockIdx.z * N + n + 1] = s1;
      }
    }
  }
}

// dW[dst(n, k)] += alpha * sum_s part[s][n][k] (s = 0, 1, ... in order); dst = n K + k, or with cin > 0 the conv
// layout n (3 cin) + (k % cin) 3 + k / cin for k < 3 cin (k >= 3 cin is the K padding: dropped)
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ part, const float* __restrict__ dbpart,
                                                      int slices, int N, int K, float alpha, int cin, float* dW,
                                                      float* db) {
  const long NK = (long)N * K;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < NK) {
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += part[(size_t)z * NK + i];
    const int n = (int)(i / K), k = (int)(i - (long)n * K);
    if (!dW) {
    } else if (cin == 0) {
      dW[i] += alpha * s;
    } else if (k < 3 * cin) {
      const int tap = k / cin, c = k - tap * cin;
      dW[(size_t)n * 3 * cin + c * 3 + tap] += alpha * s;
    }
  }
  if (db && i < N) {
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += dbpart[(size_t)z * N + i];
    db[i] += alpha * s;
  }
}

int launch_wgrad(const void* dY, long ldy, const void* X, long ldx, long M, int N, int K, float alpha, float* dW,
                 float* db, int conv_cin, void* workspace, size_t ws_bytes, hipStream_t s) {
  GWW_REQUIRE(dY && X && (dW || db), "gemm_wgrad: NULL operand");
  GWW_REQUIRE(M >= 0 && N > 0 && K > 0, "gemm_wgrad: bad shape M=%ld N=%d K=%d", M, N, K);
  GWW_REQUIRE(N % 64 == 0, "gemm_wgrad: N=%d must be a multiple of 64", N);
  GWW_REQUIRE(K % 16 == 0, "gemm_wgrad: K=%d must be a multiple of 16", K);
  GWW_REQUIRE(ldy % 8 == 0 && ldx % 8 == 0, "gemm_wgrad: row strides ldy=%ld / ldx=%ld must be multiples of 8 elements",
              ldy, ldx);
  GWW_REQUIRE(ldy >= N && ldx >= 8, "gemm_wgrad: ldy=%ld < N=%d", ldy, N);
  GWW_REQUIRE(conv_cin == 0 || (3 * conv_cin <= K && conv_cin > 0), "gemm_wgrad: conv layout needs 3 cin <= K");
  GWW_REQUIRE((((uintptr_t)dY) & 15) == 0 && (((uintptr_t)X) & 15) == 0,
              "gemm_wgrad: dY and X must be 16-byte aligned");
  if (M == 0) return GWW_OK;
  const WgradPlan p = wgrad_plan(M, N, K);
  const size_t need = wgrad_workspace_bytes(M, N, K);
  if (!workspace || ws_bytes < need)
    return fail(GWW_ERR_WORKSPACE, "gemm_wgrad: workspace %zu bytes < required %zu", ws_bytes, need);
  float* part = (float*)workspace;
  float* dbpart = db ? part + (size_t)p.slices * N * K : nullptr;
  hipLaunchKernelGGL(k_wgrad_bf16, dim3(p.tiles_k, p.tiles_n, p.slices), dim3(WG_THREADS), WG_LDS_BYTES, s,
                     (const unsigned short*)dY, ldy, (const unsigned short*)X, ldx, M, N, K, p.rows_per_slice, part,
                     dbpart);
  GWW_LAUNCH_CHECK();
  const long NK = (long)N * K;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)cdiv(NK, 256)), dim3(256), 0, s, part, dbpart, p.slices, N, K,
                     alpha, conv_cin, dW, db);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

}  // namespace gww

extern "C" size_t gww_gemm_wgrad_workspace_bytes(long M, int N, int K) {
  return (M >= 0 && N > 0 && K > 0) ? gww::wgrad_workspace_bytes(M, N, K) : 0;
}

extern "C" int gww_gemm_wgrad_bf16(const void* dY, long ldy, const void* X, long ldx, long M, int N, int K, float alpha,
                                   float* dW, float* db_or_null, void* workspace, size_t ws_bytes, void* stream) {
  GWW_REQUIRE(dW, "gww_gemm_wgrad_bf16: NULL dW");
  return gww::launch_wgrad(dY, ldy, X, ldx, M, N, K, alpha, dW, db_or_null, 0, workspace, ws_bytes,
                           (hipStream_t)stream);
}
