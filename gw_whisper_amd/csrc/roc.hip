// Signal-vs-noise evaluation on the device (Signal_vs_Noise/src/evaluation.py): the ROC curve at every distinct score, its
// AUC, and the bootstrap band of the TPR at a grid of FPRs.  Everything here is integer counting plus a few fp64 divisions
// in a fixed order, so identical calls give identical bits and the results equal sklearn's / numpy's operation for
// operation.  No float atomics, no cross-workgroup flags, nothing here synchronises.
//   k_roc_keys       key = the complement of the order-preserving image of the score: ascending keys = descending scores;
//                    then the shared stable radix sort of (key, index) pairs, four 8-bit digits (device_sort.h:
//                    radix_hist / radix_scan / radix_scatter on 32-bit keys)
//   k_roc_finish     order, rank (its inverse), pos (the label at each sorted position)
//   k_roc_groups     one workgroup: gend[g] = the last sorted position of the g-th run of equal scores, G
//   k_roc_curve      one workgroup: fps / tps / fpr / tpr at every run end, P, Nneg, the AUC from an int64 sum
//   k_roc_bootstrap  THE HOT PATH: one workgroup per replicate.  Multiplicities of the sorted positions in LDS tiles, a block
//                    scan of (c pos, c (1 - pos)) with the previous tile's carry, the running (tps, fps) at every position
//                    into the replicate's private workspace row, then np.interp's search and expression per grid point
//   k_roc_band       one thread per grid point: mean and population std over the valid replicates, rows in index order
//   k_bin_eval       one workgroup: scores = sigmoid(logits), loss_sum, batches, the 2 x 2 confusion matrix
// This file is compiled with -ffp-contract=off (Makefile): a fused multiply-add in the interpolation or in the band would
// lose the bit match with numpy.
#include "common.h"
#include "device_sort.h"

namespace gww {

constexpr int RC_TILE = GWW_ROC_TILE;       // sorted positions of one LDS tile: 64 KiB of uint32 multiplicities
constexpr int RC_THREADS = 1024;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_PER = RC_TILE / RC_THREADS;  // consecutive positions of one thread in the scan
constexpr int RC_QMAX = 1024;
constexpr long RC_NMAX = 1L << 24;

static_assert(RC_PER * RC_THREADS == RC_TILE && RC_PER % 4 == 0, "a thread scans whole uint4 groups");

// ---- sort -------------------------------------------------------------------------------------------------------------
// ascending key = descending score; -0.0 and +0.0 are one value; every NaN gets key 0 (in front, counted by the caller)
__device__ __forceinline__ unsigned roc_key(float v) {
  if (v != v) return 0u;
  if (v == 0.f) v = 0.f;
  return ~ordered_u32(v);
}

__global__ __launch_bounds__(64) void k_roc_init(int* __restrict__ G, int* __restrict__ n_nan) {
  if (threadIdx.x == 0) {
    G[0] = 0;
    n_nan[0] = 0;
  }
}

__global__ __launch_bounds__(256) void k_roc_keys(const float* __restrict__ scores, int N, unsigned* __restrict__ key,
                                                  int* __restrict__ idx, int* __restrict__ n_nan) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float v = scores[i];
  key[i] = roc_key(v);
  idx[i] = i;
  if (v != v) atomicAdd(n_nan, 1);            // an integer count: the order of the adds does not matter
}

__global__ __launch_bounds__(256) void k_roc_finish(const int* __restrict__ idx, const float* __restrict__ labels, int N,
                                                    int* __restrict__ order, int* __restrict__ rank,
                                                    unsigned char* __restrict__ pos) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  int i = idx[p];
  if ((unsigned)i >= (unsigned)N) i = 0;     // a permutation by construction
  order[p] = i;
  rank[i] = p;
  pos[p] = labels[i] > 0.5f ? 1 : 0;
}

// one workgroup walks the sorted keys 1024 at a time: a position ends a run when the next key differs
__global__ __launch_bounds__(RC_THREADS) void k_roc_groups(const unsigned* __restrict__ key, int N, int* __restrict__ gend,
                                                           int* __restrict__ G) {
  __shared__ unsigned long long part[RC_WAVES];
  unsigned long long carry = 0ull;
  for (int t0 = 0; t0 < N; t0 += RC_THREADS) {
    const int p = t0 + threadIdx.x;
    const bool end = p < N && (p == N - 1 || key[p] != key[p + 1]);
    unsigned long long tot;
    const unsigned long long incl = block_scan<unsigned long long, RC_WAVES>(end ? 1ull : 0ull, part, &tot);
    if (end) gend[(int)(carry + incl) - 1] = p;
    carry += tot;
  }
  if (threadIdx.x == 0) G[0] = (int)carry;
}

// ---- curve ------------------------------------------------------------------------------------------------------------
// one workgroup.  cum[p] = the positives among the sorted positions 0..p (workspace, written and read by this workgroup
// only: the barrier between the phases is the whole protocol); vertex 0 = (0, 0), vertex g + 1 sits at gend[g].
__global__ __launch_bounds__(RC_THREADS) void k_roc_curve(const unsigned char* __restrict__ pos, const int* __restrict__ gend,
                                                          const int* __restrict__ Gp, int N, unsigned* __restrict__ cum,
                                                          long long* __restrict__ fps, long long* __restrict__ tps,
                                                          double* __restrict__ fpr, double* __restrict__ tpr,
                                                          long long* __restrict__ counts, double* __restrict__ auc) {
  __shared__ unsigned long long part[RC_WAVES];
  unsigned long long carry = 0ull;
  for (int t0 = 0; t0 < N; t0 += RC_THREADS) {
    const int p = t0 + threadIdx.x;
    unsigned long long tot;
    const unsigned long long incl = block_scan<unsigned long long, RC_WAVES>(p < N && pos[p] ? 1ull : 0ull, part, &tot);
    if (p < N) cum[p] = (unsigned)(carry + incl);
    carry += tot;
  }
  __syncthreads();
  int G = Gp[0];
  if (G < 0) G = 0;
  if (G > N) G = N;
  const long long P = (long long)carry, Nn = (long long)N - P;
  unsigned long long acc = 0ull;
  for (int g = (int)threadIdx.x; g <= G; g += RC_THREADS) {
    long long tp = 0, fp = 0, tp0 = 0, fp0 = 0;
    if (g > 0) {
      int e = gend[g - 1];
      if ((unsigned)e >= (unsigned)N) e = N - 1;
      tp = cum[e];
      fp = (long long)e + 1 - tp;
      if (g > 1) {
        int e0 = gend[g - 2];
        if ((unsigned)e0 >= (unsigned)N) e0 = N - 1;
        tp0 = cum[e0];
        fp0 = (long long)e0 + 1 - tp0;
      }
      acc += (unsigned long long)((fp - fp0) * (tp + tp0));
    }
    fps[g] = fp;
    tps[g] = tp;
    fpr[g] = (double)fp / (double)Nn;
    tpr[g] = (double)tp / (double)P;
  }
  unsigned long long tot;
  block_scan<unsigned long long, RC_WAVES>(acc, part, &tot);           // an integer sum: exact in any order
  if (threadIdx.x == 0) {
    counts[0] = P;
    counts[1] = Nn;
    auc[0] = (double)tot / (double)(2ull * (unsigned long long)P * (unsigned long long)Nn);
  }
}

// ---- bootstrap --------------------------------------------------------------------------------------------------------
// vertex j of the replicate's curve: (0, 0) for j = 0, else the running counts at the end of run j - 1
__device__ __forceinline__ uint2 roc_vertex(const uint2* __restrict__ row, const int* __restrict__ gend, int j, int N) {
  if (j == 0) return uint2{0u, 0u};
  int e = gend[j - 1];
  if ((unsigned)e >= (unsigned)N) e = N - 1;
  return row[e];
}

__global__ __launch_bounds__(RC_THREADS) void k_roc_bootstrap(const int* __restrict__ rank, const unsigned char* __restrict__ pos,
                                                              const int* __restrict__ gend, const int* __restrict__ Gp,
                                                              const int* __restrict__ idx, int N, const double* __restrict__ grid,
                                                              int Q, uint2* __restrict__ ws, double* __restrict__ tpr,
                                                              unsigned char* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned sm_roc[];
  unsigned* mult = sm_roc;                                                      // [RC_TILE]
  unsigned long long* part = reinterpret_cast<unsigned long long*>(sm_roc + RC_TILE);   // [RC_WAVES]
  int* bad = reinterpret_cast<int*>(part + RC_WAVES);
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  const int* draws = idx + r * (size_t)N;
  uint2* row = ws + r * (size_t)N;            // x = tps, y = fps at every sorted position
  if (tid == 0) bad[0] = 0;
  unsigned long long carry = 0ull;            // (tps << 32) | fps behind the previous tile: each at most N <= 2^24
  for (int t0 = 0; t0 < N; t0 += RC_TILE) {
    for (int i = tid; i < RC_TILE; i += RC_THREADS) mult[i] = 0u;
    __syncthreads();
    for (int j = tid; j < N; j += RC_THREADS) {
      const int s = draws[j];
      if ((unsigned)s >= (unsigned)N) {       // not a draw from 0..N-1: the replicate is marked invalid
        bad[0] = 1;
        continue;
      }
      const unsigned q = (unsigned)(rank[s] - t0);
      if (q < (unsigned)RC_TILE) atomicAdd(&mult[q], 1u);
    }
    __syncthreads();
    const int q0 = tid * RC_PER, p0 = t0 + q0;
    unsigned c[RC_PER];
    unsigned char y[RC_PER];
#pragma unroll
    for (int u = 0; u < RC_PER; u += 4) {
      const uint4 m = *reinterpret_cast<const uint4*>(mult + q0 + u);
      c[u] = m.x; c[u + 1] = m.y; c[u + 2] = m.z; c[u + 3] = m.w;
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int u = 0; u < RC_PER; ++u) {
      y[u] = p0 + u < N ? pos[p0 + u] : 0;
      mine += y[u] ? (unsigned long long)c[u] << 32 : (unsigned long long)c[u];
    }
    unsigned long long tot;
    unsigned long long run = carry + block_scan<unsigned long long, RC_WAVES>(mine, part, &tot) - mine;
#pragma unroll
    for (int u = 0; u < RC_PER; ++u) {
      run += y[u] ? (unsigned long long)c[u] << 32 : (unsigned long long)c[u];
      if (p0 + u < N) row[p0 + u] = uint2{(unsigned)(run >> 32), (unsigned)run};
    }
    carry += tot;
  }
  __syncthreads();                            // the row is written; this workgroup alone reads it back
  const unsigned Pr = (unsigned)(carry >> 32), Nr = (unsigned)carry;
  const bool ok = Pr > 0u && Nr > 0u && bad[0] == 0;
  if (tid == 0) valid[r] = ok ? 1 : 0;
  int G = Gp[0];
  if (G < 1) G = 1;
  if (G > N) G = N;
  const double dP = (double)Pr, dN = (double)Nr;
  for (int q = tid; q < Q; q += RC_THREADS) {
    double out = __longlong_as_double(0x7FF8000000000000ll);
    if (ok) {
      const double x = grid[q];
      int lo = 0, hi = G;                     // the rightmost vertex j with fpr_j <= x (numpy's search); fpr_0 = 0
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const double f = (double)roc_vertex(row, gend, mid, N).y / dN;
        if (f <= x) lo = mid; else hi = mid - 1;
      }
      const uint2 a = roc_vertex(row, gend, lo, N);
      const double ta = (double)a.x / dP;
      if (lo == G) {
        out = ta;
      } else {
        const uint2 b = roc_vertex(row, gend, lo + 1, N);
        const double fa = (double)a.y / dN, fb = (double)b.y / dN, tb = (double)b.x / dP;
        const double slope = (tb - ta) / (fb - fa);     // np.interp's expression, operation for operation
        const double prod = slope * (x - fa);
        out = prod + ta;
      }
    }
    tpr[r * (size_t)Q + q] = out;
  }
}

// ---- band -------------------------------------------------------------------------------------------------------------
// thread q: the valid rows in index order, numpy's axis-0 order: mean = sum / n, std = sqrt(sum((v - mean)^2) / n)
__global__ __launch_bounds__(64) void k_roc_band(const double* __restrict__ tpr, const unsigned char* __restrict__ valid, int R,
                                                 int Q, double* __restrict__ mean, double* __restrict__ std,
                                                 int* __restrict__ n_valid) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= Q) return;
  int n = 0;
  double s = 0.0;
  for (int r = 0; r < R; ++r)
    if (valid[r]) {
      s = s + tpr[(size_t)r * Q + q];
      ++n;
    }
  const double m = s / (double)n;
  double v = 0.0;
  for (int r = 0; r < R; ++r)
    if (valid[r]) {
      const double d = tpr[(size_t)r * Q + q] - m;
      const double dd = d * d;
      v = v + dd;
    }
  mean[q] = m;
  std[q] = __dsqrt_rn(v / (double)n);
  if (q == 0) n_valid[0] = n;
}

// ---- binary evaluation accumulate ---------------------------------------------------------------------------------------
// one workgroup (the binary twin of k_det_eval): scores = sigmoid(logits) rounded once from fp64, the batch-mean
// BCEWithLogitsLoss from fp64 terms in a fixed tree, rounded to fp32 as loss.item() is; integer LDS atomics for the matrix
__global__ __launch_bounds__(256) void k_bin_eval(const float* __restrict__ logits, const float* __restrict__ labels, int B,
                                                  float* __restrict__ scores, double* __restrict__ loss_sum,
                                                  long long* __restrict__ batches, long long* __restrict__ confusion) {
  __shared__ int cm[4];
  const int tid = threadIdx.x;
  if (tid < 4) cm[tid] = 0;
  __syncthreads();
  double s = 0.0;
  for (int i = tid; i < B; i += 256) {
    const double z = (double)logits[i], y = (double)labels[i];
    const float p = (float)(1.0 / (1.0 + exp(-z)));
    scores[i] = p;
    s += fmax(z, 0.0) - z * y + log1p(exp(-fabs(z)));
    const int pred = rintf(p) > 0.5f ? 1 : 0;           // torch.round: half to even, a probability of exactly 0.5 is class 0
    atomicAdd(&cm[(labels[i] > 0.5f ? 2 : 0) + pred], 1);
  }
  s = block_sum_f64(s);                      // its barriers also order cm
  if (tid == 0) {
    loss_sum[0] += (double)(float)(s / (double)B);
    batches[0] += 1;
  }
  if (tid < 4) confusion[tid] += cm[tid];
}

}  // namespace gww

using namespace gww;

extern "C" int gww_roc_tile(void) { return RC_TILE; }

extern "C" size_t gww_roc_sort_workspace_bytes(long N) {
  if (N < 2 || N > RC_NMAX) return 0;
  return radix_carve<unsigned>(nullptr, N).bytes;
}

extern "C" int gww_roc_sort_f32(const float* scores, const float* labels, long N, int* order, int* rank, unsigned char* pos,
                                int* gend, int* G, int* n_nan, void* ws, size_t ws_bytes, void* stream) {
  GWW_REQUIRE(scores && labels && order && rank && pos && gend && G && n_nan && ws, "gww_roc_sort_f32: NULL argument");
  GWW_REQUIRE(N >= 2 && N <= RC_NMAX, "gww_roc_sort_f32: N=%ld must be 2..2^24", N);
  GWW_REQUIRE(ws_bytes >= gww_roc_sort_workspace_bytes(N), "gww_roc_sort_f32: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_roc_sort_workspace_bytes(N));
  GWW_REQUIRE(aligned(ws, 16), "gww_roc_sort_f32: workspace must be 16-byte aligned");
  const RadixWs<unsigned> w = radix_carve<unsigned>(ws, N);
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N;
  const unsigned b256 = (unsigned)cdiv(N, 256);
  hipLaunchKernelGGL(k_roc_init, dim3(1), dim3(64), 0, s, G, n_nan);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_roc_keys, dim3(b256), dim3(256), 0, s, scores, n, w.key_a, w.idx_a, n_nan);
  GWW_LAUNCH_CHECK();
  const unsigned* key;
  const int* idx;
  GWW_TRY(radix_sort_pairs(w, nullptr, N, s, &key, &idx));
  hipLaunchKernelGGL(k_roc_finish, dim3(b256), dim3(256), 0, s, idx, labels, n, order, rank, pos);
  GWW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_roc_groups, dim3(1), dim3(RC_THREADS), 0, s, key, n, gend, G);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_roc_curve_workspace_bytes(long N) {
  if (N < 2 || N > RC_NMAX) return 0;
  return (size_t)N * sizeof(unsigned);
}

extern "C" int gww_roc_curve_f64(const unsigned char* pos, const int* gend, const int* G, long N, long long* fps, long long* tps,
                                 double* fpr, double* tpr, long long* counts, double* auc, void* ws, size_t ws_bytes,
                                 void* stream) {
  GWW_REQUIRE(pos && gend && G && fps && tps && fpr && tpr && counts && auc && ws, "gww_roc_curve_f64: NULL argument");
  GWW_REQUIRE(N >= 2 && N <= RC_NMAX, "gww_roc_curve_f64: N=%ld must be 2..2^24", N);
  GWW_REQUIRE(ws_bytes >= gww_roc_curve_workspace_bytes(N), "gww_roc_curve_f64: workspace of %zu bytes, %zu needed", ws_bytes,
              gww_roc_curve_workspace_bytes(N));
  GWW_REQUIRE(aligned(ws, 4), "gww_roc_curve_f64: workspace must be 4-byte aligned");
  hipLaunchKernelGGL(k_roc_curve, dim3(1), dim3(RC_THREADS), 0, (hipStream_t)stream, pos, gend, G, (int)N,
                     reinterpret_cast<unsigned*>(ws), fps, tps, fpr, tpr, counts, auc);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" size_t gww_roc_bootstrap_workspace_bytes(long Rc, long N) {
  if (Rc < 1 || Rc > 65535 || N < 2 || N > RC_NMAX) return 0;
  return (size_t)Rc * (size_t)N * sizeof(uint2);
}

extern "C" int gww_roc_bootstrap_tpr_f64(const int* rank, const unsigned char* pos, const int* gend, const int* G,
                                         const int* idx, long Rc, long N, const double* grid, int Q, double* tpr,
                                         unsigned char* valid, void* ws, size_t ws_bytes, void* stream) {
  GWW_REQUIRE(rank && pos && gend && G && idx && grid && tpr && valid && ws, "gww_roc_bootstrap_tpr_f64: NULL argument");
  GWW_REQUIRE(N >= 2 && N <= RC_NMAX, "gww_roc_bootstrap_tpr_f64: N=%ld must be 2..2^24", N);
  GWW_REQUIRE(Rc >= 1 && Rc <= 65535, "gww_roc_bootstrap_tpr_f64: Rc=%ld must be 1..65535", Rc);
  GWW_REQUIRE(Q >= 1 && Q <= RC_QMAX, "gww_roc_bootstrap_tpr_f64: Q=%d must be 1..%d", Q, RC_QMAX);
  GWW_REQUIRE(ws_bytes >= gww_roc_bootstrap_workspace_bytes(Rc, N), "gww_roc_bootstrap_tpr_f64: workspace of %zu bytes, %zu needed",
              ws_bytes, gww_roc_bootstrap_workspace_bytes(Rc, N));
  GWW_REQUIRE(aligned(ws, 8), "gww_roc_bootstrap_tpr_f64: workspace must be 8-byte aligned");
  const size_t lds = (size_t)RC_TILE * sizeof(unsigned) + RC_WAVES * sizeof(unsigned long long) + 16;
  GWW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_roc_bootstrap), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_roc_bootstrap, dim3((unsigned)Rc), dim3(RC_THREADS), lds, (hipStream_t)stream, rank, pos, gend, G, idx,
                     (int)N, grid, Q, reinterpret_cast<uint2*>(ws), tpr, valid);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_roc_band_f64(const double* tpr, const unsigned char* valid, long R, int Q, double* mean, double* std,
                                int* n_valid, void* stream) {
  GWW_REQUIRE(tpr && valid && mean && std && n_valid, "gww_roc_band_f64: NULL argument");
  GWW_REQUIRE(R >= 1 && R <= (1L << 24), "gww_roc_band_f64: R=%ld must be 1..2^24", R);
  GWW_REQUIRE(Q >= 1 && Q <= RC_QMAX, "gww_roc_band_f64: Q=%d must be 1..%d", Q, RC_QMAX);
  hipLaunchKernelGGL(k_roc_band, dim3((unsigned)cdiv(Q, 64)), dim3(64), 0, (hipStream_t)stream, tpr, valid, (int)R, Q, mean, std,
                     n_valid);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}

extern "C" int gww_binary_eval_accumulate(const float* logits, const float* labels, int B, float* scores, long offset,
                                          long capacity, double* loss_sum, long long* batches, long long* confusion,
                                          void* stream) {
  GWW_REQUIRE(logits && labels && scores && loss_sum && batches && confusion, "gww_binary_eval_accumulate: NULL argument");
  GWW_REQUIRE(B >= 1 && B <= 65536, "gww_binary_eval_accumulate: B=%d must be 1..65536", B);
  GWW_REQUIRE(offset >= 0 && capacity >= 0 && offset <= capacity - B,
              "gww_binary_eval_accumulate: offset=%ld + B=%d exceeds the capacity=%ld of scores", offset, B, capacity);
  hipLaunchKernelGGL(k_bin_eval, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, B, scores + offset, loss_sum,
                     batches, confusion);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
