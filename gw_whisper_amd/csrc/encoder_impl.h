// What the three host drivers of the encoder share: the handle and its packed weights (encoder.hip: create / pack /
// inference forward, encoder_train.hip: the bf16 training step, encoder_train_f32.hip: the exact-fp32 one), the checks and the
// table of the adapter targets of both training backwards.  Internal: not installed, nothing of it is part of the C ABI.
#pragma once

#include "common.h"
#include "epilogue.h"

#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace gww {

struct LayerW {
  // bf16 panels
  unsigned short *wqkv, *wo, *w1, *w2;
  // fp32 panels (parity path)
  float *wqkv32, *wo32, *w132, *w232;
  float *bqkv, *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
  float* bqkv16;   // q | k | v bias of the bf16 panels: the q part carries log2(e) like the packed bf16 q weights
  // LayerNorm-folded panels for the A-stationary GEMMs (gain folded into W, see gemm_astat.hip)
  unsigned short *wqkv_ln, *w1_ln;
  unsigned short* wmlp;   // fused-MLP weight stream (d = 384): mlp_fused.hip
  unsigned short* wqkv_st; // the folded q / k / v panel alone as a tile stream (layer 0: LN1 + q / k / v alone)
  unsigned short* wmlp_op; // the fused-MLP stream with the W_o tiles in front (inference: out_proj fused into the block)
  float *uqkv, *cbqkv, *u1, *cb1;
  // transposed bf16 panels [K][N] for the dX GEMMs of the training backward
  unsigned short *wqkvT, *woT, *w1T, *w2T;
};

// conv1's K (3 taps x n_mels) padded to a multiple of 64: 256 for 80 mels, 384 for 128 (whisper-large-v3)
constexpr int conv1_kpad(int n_mels) { return (3 * n_mels + 63) / 64 * 64; }

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Rows of a row-indexed activation of M = B * T tokens: padded so that the large-M GEMMs store whole 256-row panels
// unconditionally (rows past M are scratch); + 512 covers conv2's remapped garbage rows
inline size_t padded_rows(size_t M) { return (M + 255) / 256 * 256 + 512; }

// The head of both training arenas (caller-owned): L layer records of layer_stride bytes, x_in[l] at `x_in` inside
// record l, and behind them x_in[L], the input of the final LayerNorm.
struct SavedArena {
  size_t layer_stride, x_in, total;
  int n_layers;
  float* x_in_at(void* saved, int l) const {
    return (float*)((char*)saved + (l < n_layers ? (size_t)l * layer_stride + x_in : (size_t)n_layers * layer_stride));
  }
  const float* x_in_at(const void* saved, int l) const { return x_in_at(const_cast<void*>(saved), l); }
};

// GWW_GENERIC_PATH, the laboratory build's debug mask of the host drivers (0 in the product build, read once per process):
// each bit takes one fast path out.  Read it through generic_path_mask() alone.
enum : int {
  GP_LAYER_GEMMS = 1,      // bit 0: generic layer GEMMs (no A-stationary kernels)
  GP_CONV1 = 2,            // bit 1: generic conv1
  GP_CONV2 = 4,            // bit 2: conv2 off k_gemm_bf16_v4
  GP_MLP = 8,              // bit 3: unfused MLP (separate fc1 / fc2 kernels)
  GP_QKV = 16,             // bit 4: stand-alone LN1 + q / k / v kernels
  GP_POOLED = 32,          // bit 5: no pooled last layer
  GP_LNQKV0 = 64,          // bit 6: layer 0's LN1 + q / k / v by the LN-fused A-stationary GEMM
  GP_OUT_PROJ = 128,       // bit 7: stand-alone out_proj (inference, training forward; with bit 4: the packer's plain stream)
  GP_FINAL_LN = 256,       // bit 8: stand-alone final LayerNorm
  GP_ASTAT_512 = 512,      // bit 9: A-stationary layer GEMMs at d = 512
  GP_CONV2_FULLN = 1024,   // bit 10: conv2 on the generic GEMM where k_gemm_fulln would take it
  GP_STEM_SHORTCUT = 2048, // bit 11: no constant-tail shortcut of the stem
  GP_X_NATIVE = 4096,      // bit 12: the residual stream in row order between the fused blocks too
};
inline int generic_path_mask() {
  static const int mask = (int)lab_int("GWW_GENERIC_PATH", 0);
  return mask;
}

// The adapter targets of a training backward (gww_dora_target), checked and indexed once for both drivers.  check_targets
// reads nothing of the handle: the targets' own fields (rank, the seven pointers), then that no (layer, proj) comes twice.
inline int check_targets(const char* who, const gww_dora_target* t, int n) {
  for (int i = 0; i < n; ++i) {
    GWW_REQUIRE(t[i].r >= 1 && t[i].r <= 64, "%s: target %d has rank %d: adapter gradients support ranks 1..64", who, i, t[i].r);
    GWW_REQUIRE(t[i].A && t[i].B && t[i].mag && t[i].nrm && t[i].dA && t[i].dB && t[i].dm, "%s: NULL pointer in target %d", who, i);
  }
  for (int i = 1; i < n; ++i)
    for (int j = 0; j < i; ++j)
      GWW_REQUIRE(t[i].layer != t[j].layer || t[i].proj != t[j].proj, "%s: duplicate target: %d and %d both name layer %d proj %d",
                  who, j, i, t[i].layer, t[i].proj);
  return GWW_OK;
}
// ... and, once the handle has given L, their layer / proj range
inline int check_target_range(const char* who, const gww_dora_target* t, int n, int L) {
  for (int i = 0; i < n; ++i)
    GWW_REQUIRE(t[i].layer >= 0 && t[i].layer < L && t[i].proj >= 0 && t[i].proj <= 5, "%s: bad target %d", who, i);
  return GWW_OK;
}
// at(layer, proj): the target of that projection or nullptr, of targets that passed both checks
struct TargetTable {
  std::vector<const gww_dora_target*> slot;   // [L][6]; empty without targets
  TargetTable() = default;
  TargetTable(const gww_dora_target* t, int n, int L) : slot(n > 0 ? (size_t)L * 6 : 0, nullptr) {
    for (int i = 0; i < n; ++i) slot[(size_t)t[i].layer * 6 + t[i].proj] = &t[i];
  }
  const gww_dora_target* at(int layer, int proj) const { return slot.empty() ? nullptr : slot[(size_t)layer * 6 + proj]; }
};

}  // namespace gww

// kernel classes of one forward, for the optional per-kernel event trace (bench.py roofline)
enum : int { TR_MEL = 0, TR_CONV1, TR_CONV2, TR_QKV, TR_ATTN, TR_OUT, TR_FC1, TR_FC2, TR_LN, TR_MLP, TR_MLPQKV, TR_LNROWS, TR_MLPFIN, TR_COUNT };

struct TraceSpan { int cls; hipEvent_t a, b; };

struct gww_encoder {
  gww_enc_cfg cfg{};
  bool ready = false;
  bool trace = false;
  bool stem_shortcut = true;        // the constant-tail shortcut of the bf16 inference stem (gww_encoder_set_stem_shortcut)
  bool x_native = true;             // the residual stream in accumulator order between fused blocks (gww_encoder_set_x_native)
  std::vector<TraceSpan> spans;     // recorded since the last read
  std::vector<hipEvent_t> pool;     // reusable events
  // dual-stream split: two half batches on two library-owned streams, so HBM-bound kernels of one
  // half overlap MFMA-bound kernels of the other on different CUs
  int split = 0;                    // 0: off, 1: on for batch >= 2 * kSplitMin
  hipStream_t s2[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_skew = nullptr, ev_join[2] = {nullptr, nullptr};
  char* blob = nullptr;
  size_t blob_bytes = 0;
  unsigned short *c1w = nullptr, *c2w = nullptr;
  unsigned short *c1wT = nullptr, *c2wT = nullptr;   // [Kpad, d] / [3 d, d]: input-gradient GEMMs of the stem
  float *c1w32 = nullptr, *c2w32 = nullptr;
  float *c1b = nullptr, *c2b = nullptr, *pos = nullptr, *lnw = nullptr, *lnb = nullptr;
  float* pos_c = nullptr;           // [kStemTt, d] positions of the compact stem: pos[0 .. Tt - 3], a zero row, pos[T - 1]
  std::vector<gww::LayerW> layers;
};
