// Every launcher, size function and support predicate that one translation unit defines and another calls, declared
// ONCE, default arguments included.  common.h includes this file at its end, so every .hip sees it -- the defining one
// too: a definition whose signature drifts from its declaration, or that repeats a default, does not compile.
// Every launcher returns a gww status code.
#pragma once

namespace gww {

// ---- elementwise.hip
int launch_layernorm(const float* x, const float* w, const float* b, void* y, int out_bf16,
                     long M, int d, hipStream_t s, const void* delta_bf16 = nullptr);
int launch_layernorm_rows(const float* x, long row_stride, const float* w, const float* b, float* y,
                          long M, int d, hipStream_t s, const void* delta_bf16 = nullptr);
int launch_pack_weight(const float* w, void* out, int out_bf16, int N, int C, int taps, int Kpad,
                       float scale, hipStream_t s);

// ---- the front end of any configuration: logmel_host.cpp (plain C++: the supported set, the frame arithmetic and the
// tables, shared by both twins), logmel_any.hip
int frontend_validate(const gww_frontend_cfg* c, const char* who);
int frontend_live_frames(const gww_frontend_cfg* c, int n_eff);
void frontend_tables(const gww_frontend_cfg* c, float* win, float* cost, float* sint, float* fbT);
struct LogmelAnyPlan {
  int n_mels, n_fft, hop, chunk, n_frames;
  int S;               // row stride of the folded frames in LDS: n_fft / 2 + 1 rounded up to 4
  int ft, groups;      // frames per thread (8 or 4), thread groups per workgroup (1, 2 or 4)
  size_t lds_bytes;
};
int logmel_any_plan(const gww_frontend_cfg* c, LogmelAnyPlan* p);
// tables: win | cost | sint [n_fft] each, then fbT [n_fft / 2 + 1][n_mels] (device)
// n_outer x n_seg segments: segment o n_seg + i starts at wave + o outer_stride + i wave_stride
int launch_logmel_any(const LogmelAnyPlan& p, const float* tables, const float* wave, int n_seg, int n_eff, int live,
                      long wave_stride, float* out, float* seg_max, hipStream_t s, int n_outer = 1, long outer_stride = 0);
// ---- the windows of a series: logmel_host.cpp (the route and the frame counts: plain C++), logmel_windows.hip
int logmel_windows_plan(const gww_frontend_cfg* c, int step, int n_windows, gww_windows_plan* out, const char* who);
// wp: the plan of (cfg, step, n_windows); workspace: n_rows * wp.workspace_bytes bytes, 16-byte aligned
int launch_logmel_windows(const LogmelAnyPlan& p, const gww_windows_plan& wp, const float* tables, const float* series,
                          int n_rows, int n_series, long row_stride, int step, int w0, int n_windows, float* out,
                          int out_rows_major, void* workspace, hipStream_t s);

// ---- the conv stem: conv1_mel.hip, stem_tail.hip, gemm_bf16.hip
bool conv1_mel_supported(int n_mels, int d, int kpad);
int launch_conv1_mel(const float* mel, const void* W, const float* bias, void* c1, int B, int T, int d, hipStream_t s,
                     int t_stride = 0, const int* run_flag = nullptr, int run_if = 0);
bool stem_tail_supported(int t_in, int d);
int launch_stem_detect(const float* mel, int* flag, long rows, int t_in, hipStream_t s);
int launch_stem_fill(const float* xs, const float* tr, const float* pos, float* x, const int* flag, int B, int T, int d,
                     hipStream_t s, int Tt = kStemTt);
int launch_mel_to_tokens(const float* mel, void* out, int out_bf16, int B, int C, int T, hipStream_t s);

// ---- GEMMs: gemm_astat.hip, gemm_bf16.hip, gemm_v4.hip, gemm_fulln.hip, gemm_f32.hip
int launch_gemm_astat(const void* A, long lda, const void* delta, float* x_out, const float* ln_u,
                      const float* ln_cb, const void* W, const float* bias, void* C, long M, int N, int K,
                      int epi, int rows_per_batch, hipStream_t s, long c_panel_rows = 0);
int launch_gemm_bf16(const void* A, long lda, const void* W, const float* bias, const float* resid,
                     const float* pos, void* C, long M, int N, int K, int epi, int rows_per_batch,
                     hipStream_t s, int rows_padded_256 = 0);
int launch_gemm_bf16_v4(const void* A, long lda, const void* W, const float* bias, const float* resid, void* C, long M,
                        int N, int K, int epi, hipStream_t s, int force_split = 0, const float* pos = nullptr,
                        int rows_per_batch = 0, int n_real = 0, float* dump = nullptr, const int* run_flag = nullptr,
                        int run_if = 0, float* tmpl_r = nullptr, int tmpl_t = 0);
int launch_gemm_fulln(const void* A, long lda, const void* W, const float* bias, const float* pos, void* C,
                      long M, int N, int K, int epi, int rows_per_batch, hipStream_t s);
int launch_gemm_f32(const float* A, long lda, const float* W, const float* bias, const float* resid,
                    const float* pos, float* C, long M, int N, int K, int epi, int rows_per_batch,
                    hipStream_t s);

// ---- attention.hip, attention_w64.hip (laboratory build), attention_probs.hip, attention_bwd.hip
int launch_attention_bf16(const void* qkv, void* ctx, int B, int T, int H, hipStream_t s, float* lse = nullptr,
                          bool last_tile_only = false, bool q_log2 = false);
int launch_attention_w64_bf16(const void* qkv, void* ctx, int B, int T, int H, hipStream_t s, float* lse);
bool attention_log2q_enabled();   // the inference path packs q in log2 units (attention.hip)
int launch_attention_f32(const float* qkv, float* ctx, int B, int T, int H, hipStream_t s);
int launch_attention_probs(const void* qkv, bool bf16, bool q_log2, float* probs, int B, int T, int H, hipStream_t s);
int launch_attention_bwd_bf16(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* D,
                              void* dqkv, int B, int T, int H, hipStream_t s, bool q_log2);

// ---- mlp_fused.hip
int launch_mlp_pack(const void* w1_folded, const void* w2, const void* wqkv_folded, void* out, int d, int F, int NQ,
                    hipStream_t s, const void* wo = nullptr);
bool mlp_fused_supported(int d, int F);   // the fused block exists for this width / ffn (MF_D, MF_FMAX)
bool mlp_fused_x_native_supported();      // ... and its accumulator-order instantiations (MlpFusedArgs::x_native_in / _out)
// The operands of the compact stem (stem_tail.hip) from which layer 0 forms its rows of the residual stream: xs [B, Tt, 384],
// tr [B, 384], pos [T, 384] where *flag == 1; x is read where it is 0 (decided in the kernel).  M = B T.
struct MfX0 {
  const float *xs, *tr, *pos;
  const int* flag;
  int T, Tt;
};
// One launch of k_mlp_fused.  Unset fields stay null / 0; which are set selects the instantiation <MODE, OP, X0>:
//   neither delta nor ctx : LayerNorm 1 + q / k / v of x alone (qkv_* set, no block operand)           <2, false>
//   delta                 : x_new = x + delta, then LN2 + fc1 + GELU + fc2                               <., false>
//   ctx + bo              : x_new = x + bf16(ctx W_o^T + bo) first; Wt starts with the W_o tiles           <., true>
//   ... then C            : the block's bf16 delta, to be added to x_new by the next reader                <0, .>
//   ... or qkv_out        : x_next = x_new + block, LN1 + q / k / v of it behind (the next layer's)        <1, .>
//   ... or y (ctx only)   : y = LayerNorm_final(x_new + block), the encoder's last block                   <3, true>
//   x0                    : x is formed in registers from the compact stem; modes <2, false> and <1, true> only
struct MlpFusedArgs {
  const char* who = "mlp_fused";   // the calling entry point, for error messages
  const float* x = nullptr;        // fp32 [M, 384] residual stream entering the launch
  const void* delta = nullptr;     // bf16 [M, 384] delta pending on x
  const void* ctx = nullptr;       // bf16 [M, 384] attention context ...
  const float* bo = nullptr;       // ... and the out_proj bias
  float* x_new = nullptr;          // fp32 [M, 384], != x: the block's intermediate residual stream ...
  bool keep_x_new = false;         // ... which a caller that reads it afterwards must ask for
  const float *ln_u = nullptr, *ln_cb = nullptr;   // LN2 folded into fc1 (gww_ln_fold_weights)
  const void* Wt = nullptr;        // launch_mlp_pack's stream for this mode
  const float* b2 = nullptr;
  void* C = nullptr;               // bf16 [>= roundup(M, 128), 384] (whole 128-row panels are stored)
  const float *qkv_u = nullptr, *qkv_cb = nullptr;   // LN1 folded into the q / k / v panel
  void* qkv_out = nullptr;         // bf16 [>= roundup(M, 128), NQ]
  int NQ = 0;
  float* x_next = nullptr;         // fp32 [M, 384], != x_new; unset: x_next is written over x
  const float *lnf_w = nullptr, *lnf_b = nullptr;   // the final LayerNorm
  float* y = nullptr;              // fp32 [M, 384], != x_new
  float* last_token = nullptr;     // (with y) fp32 [M / T, 384]: row T - 1 of every segment of y once more ...
  int T = 0;                       // ... T: rows per segment, M % T == 0
  // The residual stream in accumulator order (x_native_offset, common.h; ctx blocks only, [roundup(M, 128), 384] then):
  bool x_native_in = false;        // x is read in it (neither side with x0, never with x_new kept) ...
  bool x_native_out = false;       // ... x_next is written in it (qkv_out blocks)
  const MfX0* x0 = nullptr;         // (k_mlp_fused takes it by value)
  long M = 0;
  int d = 0, F = 0;
};
int launch_mlp_fused(const MlpFusedArgs& a, hipStream_t s);

// ---- the bf16 training step: train_ops.hip, dora_grads.hip, wgrad.hip
int launch_ln_bwd(const float* x, const float* gamma, const void* dy, int dy_f32, float* dx, int accumulate,
                  void* dx_bf16, long M, int d, hipStream_t s);
int launch_gelu_bf16(const void* z, const void* df, void* out, long n, hipStream_t s);
int launch_sub_f32_bf16(const float* a, const float* b, void* out, long n, hipStream_t s);
int launch_add_delta_f32(const float* x, const void* delta_bf16, float* out, long n, hipStream_t s);
int launch_stem_dz2(const void* dxb, const void* z2, void* out, int B, int T, int d, hipStream_t s);
int launch_stem_dz1(const void* col, const void* z1, void* out, int B, int T, int Tin, int d, hipStream_t s);
int launch_stem_dmel(const void* col1, float* dmel, int B, int Tin, int C, int Kp, hipStream_t s);
int launch_ln_param_grads(const float* x, const void* dy, int dy_f32, long M, int d, float* dgamma, float* dbeta,
                          void* workspace, size_t ws_bytes, hipStream_t s);
size_t ln_param_grads_workspace_bytes(long M, int d);
int launch_pos_grad(const float* dx0, float* dpos, int B, int T, int d, hipStream_t s);
int launch_dora_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                      float yscale, float scaling, const float* A, const float* Bm, const float* mag,
                      const float* nrm, float* dA, float* dB, float* dm, long M, int d, int r, hipStream_t s,
                      void* scratch = nullptr, size_t scratch_bytes = 0);
int launch_dora_grads_multi(const void* X, long ldx, const void* dY, const void* Y, long ldy, int np,
                            const long* col_off, const float* const* bias_st, const float* yscale,
                            const float* scaling, const float* const* A, const float* const* Bm,
                            const float* const* mag, const float* const* nrm, float* const* dA, float* const* dB,
                            float* const* dm, long M, int d, hipStream_t s, void* scratch, size_t scratch_bytes);
size_t dora_grads_scratch_bytes(int np, int d);
int launch_adapter_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                         float yscale, float scaling, const float* A, const float* Bm, const float* mag,
                         const float* nrm, float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r,
                         hipStream_t s, void* scratch, size_t scratch_bytes);
size_t adapter_grads_scratch_bytes(long M, int d_in, int d_out, int r);
int launch_wgrad(const void* dY, long ldy, const void* X, long ldx, long M, int N, int K, float alpha, float* dW,
                 float* db, int conv_cin, void* workspace, size_t ws_bytes, hipStream_t s);
size_t wgrad_workspace_bytes(long M, int N, int K);

// ---- the exact-fp32 training step: attention.hip, attention_bwd_f32.hip, train_f32.hip
int launch_attention_lse_f32(const float* qkv, float* ctx, float* lse, int B, int T, int H, bool last_tile_only,
                             hipStream_t s);
int launch_attention_bwd_f32(const float* qkv, const float* ctx, const float* dctx, const float* lse, float* scratch,
                             float* dqkv, int B, int T, int H, hipStream_t s);
size_t attention_bwd_f32_scratch_words(int B, int T, int H);
int launch_gemm_f32_dx(const float* A, long lda, const float* W, float* C, long ldc, long M, int N, int K, hipStream_t s);
int launch_adapter_grads_f32(const float* X, long ldx, const float* dY, const float* Y, long ldy, const float* bias,
                             float yscale, float scaling, const float* A, const float* Bm, const float* mag,
                             const float* nrm, float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r,
                             hipStream_t s, void* scratch, size_t scratch_bytes);
size_t adapter_grads_f32_scratch_bytes(long M, int d_in, int d_out, int r);
int launch_gelu_f32(const float* z, const float* g, float* out, long n, hipStream_t s);
int launch_sub_f32(const float* a, const float* b, float* out, long n, hipStream_t s);
int launch_stem_dz2_f32(const float* dx0, const float* z2, float* out, int B, int T, int d, hipStream_t s);
int launch_stem_dz1_f32(const float* col, const float* z1, float* out, int B, int T, int Tin, int d, hipStream_t s);
int launch_stem_dmel_f32(const float* col1, float* dmel, int B, int Tin, int C, int Kp, hipStream_t s);

}  // namespace gww
