// DoRA / LoRA training step in exact fp32 (precision="fp32", the parity twin of the bf16 step of encoder_train.hip): every saved
// activation is fp32 and every contraction runs on the fp32 MFMA (gemm_f32.hip, train_f32.hip, attention_bwd_f32.hip).
// It mirrors the per-op branch of the bf16 step at every width (the fused d = 384 kernels are bf16-only), including the
// pooled last layer and the stem backward, and shares the target checks and the TargetTable of encoder_impl.h with it.  The dX
// GEMMs read the stored fp32 [out][in] panels un-transposed (k_gemm_f32_dx): no second set for the optimizer step's re-pack.
//
// saved arena, per layer l:  x_in[l] [Mp,d] | qkv [Mp,3d] | lse [B,H,T] | ctx [Mp,d] | x_mid [Mp,d]   (+ x_in[L])
// LN1(x_in), LN2(x_mid) and the fc1 pre-activation z are recomputed in the backward (one LayerNorm + one fc1 GEMM per
// layer): storing them would add 6 d floats per row, twice the arena (whisper-large-v3 at 64 segments: ~190 GB
// instead of ~95 GB).  The pooled last layer keeps x_mid and x_in[L] compact ([B, d]).
#include "encoder_impl.h"

using namespace gww;

namespace {
struct SavedLayout32 : SavedArena {
  size_t qkv, lse, ctx, x_mid;
};
SavedLayout32 saved_layout32(const gww_enc_cfg& c, int B) {
  const size_t d = c.d_model, T = c.t_in / 2, H = c.n_heads;
  const size_t Mp = padded_rows((size_t)B * T);
  SavedLayout32 s{};
  s.n_layers = c.n_layers;
  Arena a;
  s.x_in = a.take(Mp * d * 4);
  s.qkv = a.take(Mp * 3 * d * 4);
  s.lse = a.take((size_t)B * H * T * 4);
  s.ctx = a.take(Mp * d * 4);
  s.x_mid = a.take(Mp * d * 4);
  s.layer_stride = a.total();
  s.total = s.layer_stride * c.n_layers + align_up(Mp * d * 4);   // + x_in[L]
  return s;
}
struct TrainWs32 {
  size_t melT, c1, h, zb, fb, dx, dh, dctx, dqkv, Dv, ascr, ascr_bytes, total;
};
TrainWs32 train_ws32(const gww_enc_cfg& c, int B) {
  const size_t d = c.d_model, F = c.ffn, Tin = c.t_in, T = c.t_in / 2, C = c.n_mels, H = c.n_heads;
  const size_t Kc1 = conv1_kpad(c.n_mels);
  const size_t Mp = padded_rows((size_t)B * T);
  const size_t M1 = (size_t)B * (Tin + 2) + 256;   // conv1 rows of the stem backward
  TrainWs32 w{};
  Arena a;
  w.melT = a.take(((size_t)B * (Tin + 2) * C + Kc1) * 4);
  w.c1 = a.take((((size_t)B * (Tin + 2) + 255) / 256 * 256 + 520) * d * 4);
  w.h = a.take(Mp * d * 4);                              // LN1 / LN2 output (forward, recomputed in the backward)
  w.zb = a.take(std::max(Mp * F, M1 * Kc1) * 4);         // fc1 pre-activation z; stem: z2, col, col1
  w.fb = a.take(std::max(Mp * F, M1 * d) * 4);           // gelu(z) / d(fc1 pre-activation); stem: dz2, z1 / dz1
  w.dx = a.take(Mp * d * 4);
  w.dh = a.take(Mp * d * 4);
  w.dctx = a.take(Mp * d * 4);
  w.dqkv = a.take(Mp * 3 * d * 4);
  w.Dv = a.take(attention_bwd_f32_scratch_words(B, (int)T, (int)H) * 4);
  const long M = (long)B * T;
  size_t mx = 0;
  for (int di : {c.d_model, c.ffn})
    for (int dd : {c.d_model, c.ffn}) mx = std::max(mx, adapter_grads_f32_scratch_bytes(M, di, dd, 64));
  w.ascr_bytes = align_up(mx);
  w.ascr = a.take(w.ascr_bytes);
  w.total = a.total();
  return w;
}

// ---- conv stem backward: x0 = gelu(conv2(gelu(conv1(mel)))) + pos, dx = d(x0) in; melT and c1 of the forward are still in
// the workspace, the pre-activations are recomputed by the same GEMMs with a plain bias epilogue
int stem_backward(const gww_encoder* e, char* base, const TrainWs32& w, const float* dx, float* d_mel, int B, hipStream_t s) {
  const int d = e->cfg.d_model, Tin = e->cfg.t_in, T = Tin / 2, C = e->cfg.n_mels, Kc1 = conv1_kpad(C);
  const float* melT = (const float*)(base + w.melT);
  const float* c1 = (const float*)(base + w.c1);
  float* zb = (float*)(base + w.zb);
  float* fb = (float*)(base + w.fb);
  const long M2 = (long)B * (T + 1), M1 = (long)B * (Tin + 2);
  GWW_TRY(launch_gemm_f32(c1, 2L * d, e->c2w32, e->c2b, nullptr, nullptr, zb, M2, d, 3 * d, EPI_BIAS, 0, s));   // z2
  GWW_TRY(launch_stem_dz2_f32(dx, zb, fb, B, T, d, s));                                                       // dz2
  GWW_TRY(launch_gemm_f32_dx(fb, d, e->c2w32, zb, 3L * d, M2, 3 * d, d, s));                                  // col
  GWW_TRY(launch_gemm_f32(melT, C, e->c1w32, e->c1b, nullptr, nullptr, fb, M1, d, Kc1, EPI_BIAS, 0, s));      // z1
  GWW_TRY(launch_stem_dz1_f32(zb, fb, fb, B, T, Tin, d, s));                                                 // dz1
  GWW_TRY(launch_gemm_f32_dx(fb, d, e->c1w32, zb, Kc1, M1, Kc1, d, s));                                       // col1
  return launch_stem_dmel_f32(zb, d_mel, B, Tin, C, Kc1, s);
}
}  // namespace

extern "C" size_t gww_train_saved_bytes_f32(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? saved_layout32(e->cfg, batch).total : 0;
}
extern "C" size_t gww_train_workspace_bytes_f32(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? train_ws32(e->cfg, batch).total : 0;
}

extern "C" int gww_encoder_train_forward_f32(gww_encoder* e, const float* mel, int batch, void* workspace,
                                             size_t workspace_bytes, void* saved, size_t saved_bytes, float* last_hidden,
                                             int pooled, void* stream) {
  GWW_REQUIRE(e && mel && workspace && saved && last_hidden, "gww_encoder_train_forward_f32: NULL argument");
  if (!e->ready) return fail(GWW_ERR_STATE, "gww_encoder_train_forward_f32: weights not set");
  GWW_REQUIRE(batch > 0, "gww_encoder_train_forward_f32: batch must be positive");
  const SavedLayout32 sl = saved_layout32(e->cfg, batch);
  const TrainWs32 w = train_ws32(e->cfg, batch);
  if (workspace_bytes < w.total || saved_bytes < sl.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_forward_f32: workspace %zu / saved %zu bytes < required %zu / %zu",
                workspace_bytes, saved_bytes, w.total, sl.total);
  GWW_REQUIRE((((uintptr_t)mel) & 15) == 0 && (((uintptr_t)workspace) & 255) == 0 && (((uintptr_t)saved) & 255) == 0,
              "gww_encoder_train_forward_f32: mel must be 16-byte, workspace and saved 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int d = e->cfg.d_model, F = e->cfg.ffn, Tin = e->cfg.t_in, T = Tin / 2, C = e->cfg.n_mels, H = e->cfg.n_heads;
  const int Kc1 = conv1_kpad(C);
  const int B = batch, L = e->cfg.n_layers;
  const long M = (long)B * T;
  char* base = (char*)workspace;
  char* sv = (char*)saved;
  float* melT = (float*)(base + w.melT);
  float* c1 = (float*)(base + w.c1);
  float* h = (float*)(base + w.h);
  float* fb = (float*)(base + w.fb);
  // ---- stem, as the fp32 inference forward
  GWW_TRY(launch_mel_to_tokens(mel, melT, 0, B, C, Tin, s));
  GWW_HIP(hipMemsetAsync(melT + (size_t)B * (Tin + 2) * C, 0, (size_t)Kc1 * 4, s));
  GWW_HIP(hipMemsetAsync(c1, 0, (size_t)d * 4, s));
  GWW_TRY(launch_gemm_f32(melT, C, e->c1w32, e->c1b, nullptr, nullptr, c1, (long)B * (Tin + 2), d, Kc1, EPI_CONV1, Tin + 2, s));
  GWW_TRY(launch_gemm_f32(c1, 2L * d, e->c2w32, e->c2b, nullptr, e->pos, sl.x_in_at(sv, 0), (long)B * (T + 1), d, 3 * d, EPI_CONV2,
                          T + 1, s));
  for (int l = 0; l < L; ++l) {
    const LayerW& W = e->layers[l];
    char* lb = sv + (size_t)l * sl.layer_stride;
    float* qkv = (float*)(lb + sl.qkv);
    float* lse = (float*)(lb + sl.lse);
    float* ctx = (float*)(lb + sl.ctx);
    float* x_mid = (float*)(lb + sl.x_mid);
    GWW_TRY(launch_layernorm(sl.x_in_at(sv, l), W.ln1w, W.ln1b, h, 0, M, d, s));
    GWW_TRY(launch_gemm_f32(h, d, W.wqkv32, W.bqkv, nullptr, nullptr, qkv, M, 3 * d, d, EPI_BIAS, 0, s));
    if (pooled && l == L - 1) {
      // only token T - 1 is used: attention for the query tile that holds it (the other rows of ctx / lse stay zero, so
      // that the backward's row dots see finite values), then out_proj / LN2 / fc1 / GELU / fc2 / final LN on B rows;
      // x_mid and x_in[L] are saved compact
      GWW_HIP(hipMemsetAsync(ctx, 0, (size_t)M * d * 4, s));
      GWW_HIP(hipMemsetAsync(lse, 0, (size_t)B * H * T * 4, s));
      GWW_TRY(launch_attention_lse_f32(qkv, ctx, lse, B, T, H, /*last_tile_only=*/true, s));
      float* xl = (float*)(base + w.dx);   // x_in[L-1] rows (b, T-1); the gradient buffers are idle in the forward
      GWW_HIP(hipMemcpy2DAsync(xl, (size_t)d * 4, sl.x_in_at(sv, l) + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                               hipMemcpyDeviceToDevice, s));
      GWW_TRY(launch_gemm_f32(ctx + (size_t)(T - 1) * d, (long)T * d, W.wo32, W.bo, xl, nullptr, x_mid, B, d, d, EPI_RESID,
                              0, s));
      GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, h, 0, B, d, s));
      GWW_TRY(launch_gemm_f32(h, d, W.w132, W.b1, nullptr, nullptr, fb, B, F, d, EPI_GELU, 0, s));
      GWW_TRY(launch_gemm_f32(fb, F, W.w232, W.b2, x_mid, nullptr, sl.x_in_at(sv, L), B, d, F, EPI_RESID, 0, s));
      GWW_TRY(launch_layernorm(sl.x_in_at(sv, L), e->lnw, e->lnb, last_hidden, 0, B, d, s));
      return GWW_OK;
    }
    GWW_TRY(launch_attention_lse_f32(qkv, ctx, lse, B, T, H, false, s));
    GWW_TRY(launch_gemm_f32(ctx, d, W.wo32, W.bo, sl.x_in_at(sv, l), nullptr, x_mid, M, d, d, EPI_RESID, 0, s));
    GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, h, 0, M, d, s));
    GWW_TRY(launch_gemm_f32(h, d, W.w132, W.b1, nullptr, nullptr, fb, M, F, d, EPI_GELU, 0, s));
    GWW_TRY(launch_gemm_f32(fb, F, W.w232, W.b2, x_mid, nullptr, sl.x_in_at(sv, l + 1), M, d, F, EPI_RESID, 0, s));
  }
  GWW_TRY(launch_layernorm(sl.x_in_at(sv, L), e->lnw, e->lnb, last_hidden, 0, M, d, s));
  return GWW_OK;
}

// The contract of gww_encoder_train_backward (targets accumulated into, d_x0 / d_mel optional, same `pooled` as the
// forward) on the arena of gww_encoder_train_forward_f32.
extern "C" int gww_encoder_train_backward_f32(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes,
                                              const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                              const gww_dora_target* targets, int n_targets, float* d_x0, float* d_mel,
                                              int pooled, void* stream) {
  const char* who = "gww_encoder_train_backward_f32";
  GWW_REQUIRE(e && workspace && saved && d_last_hidden, "%s: NULL argument", who);
  GWW_REQUIRE(batch > 0 && n_targets >= 0 && (n_targets == 0 || targets), "%s: bad argument", who);
  GWW_TRY(check_targets(who, targets, n_targets));   // the targets' own fields first (nothing of the handle is read for them)
  GWW_REQUIRE((((uintptr_t)workspace) & 255) == 0 && (((uintptr_t)saved) & 255) == 0 && (((uintptr_t)d_last_hidden) & 15) == 0,
              "%s: workspace and saved must be 256-byte, d_last_hidden 16-byte aligned", who);
  if (!e->ready) return fail(GWW_ERR_STATE, "%s: weights not set", who);
  const int L = e->cfg.n_layers;
  GWW_TRY(check_target_range(who, targets, n_targets, L));
  const TargetTable tt(targets, n_targets, L);
  const SavedLayout32 sl = saved_layout32(e->cfg, batch);
  const TrainWs32 w = train_ws32(e->cfg, batch);
  if (workspace_bytes < w.total || saved_bytes < sl.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_backward_f32: workspace / saved arena too small");
  hipStream_t s = (hipStream_t)stream;
  const int d = e->cfg.d_model, F = e->cfg.ffn, T = e->cfg.t_in / 2, H = e->cfg.n_heads;
  const int B = batch;
  const long M = (long)B * T;
  char* base = (char*)workspace;
  const char* sv = (const char*)saved;
  float* h = (float*)(base + w.h);
  float* zb = (float*)(base + w.zb);
  float* fb = (float*)(base + w.fb);
  float* dx = (float*)(base + w.dx);
  float* dh = (float*)(base + w.dh);
  float* dctx = (float*)(base + w.dctx);
  float* dqkv = (float*)(base + w.dqkv);
  float* Dv = (float*)(base + w.Dv);
  void* ascr = base + w.ascr;
  auto agrad = [&](const gww_dora_target& t, const float* X, long ldx, const float* dY, const float* Y, long ldy,
                   const float* bias, float ysc, long rows, int d_in, int d_out) -> int {
    return launch_adapter_grads_f32(X, ldx, dY, Y, ldy, bias, ysc, t.scaling, t.A, t.B, t.mag, t.nrm, t.dA, t.dB, t.dm,
                                    rows, d_in, d_out, t.r, s, ascr, w.ascr_bytes);
  };
  const float q_ysc = 0.125f;   // the stored q is (W' x + b) / 8: the fp32 panels keep natural units
  // final LayerNorm backward -> dx (grad w.r.t. x_in[L]); pooled: on the B last-token rows only
  GWW_TRY(launch_ln_bwd(sl.x_in_at(sv, L), e->lnw, d_last_hidden, 1, dx, 0, nullptr, pooled ? B : M, d, s));
  for (int l = L - 1; l >= 0; --l) {
    const LayerW& W = e->layers[l];
    const char* lb = sv + (size_t)l * sl.layer_stride;
    const float* qkv = (const float*)(lb + sl.qkv);
    const float* lse = (const float*)(lb + sl.lse);
    const float* ctx = (const float*)(lb + sl.ctx);
    const float* x_mid = (const float*)(lb + sl.x_mid);
    const bool last_pooled = pooled && l == L - 1;
    const long rows = last_pooled ? B : M;   // everything above the attention runs on the B last-token rows when pooled
    // fc2 / GELU / fc1 / LN2   (x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))); dx = d(x_out)
    GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, h, 0, rows, d, s));
    GWW_TRY(launch_gemm_f32(h, d, W.w132, W.b1, nullptr, nullptr, zb, rows, F, d, EPI_BIAS, 0, s));   // z
    if (const gww_dora_target* t = tt.at(l, 5)) {   // fc2: x = gelu(z), dy = d(x_out), y = x_out - x_mid
      GWW_TRY(launch_gelu_f32(zb, nullptr, fb, rows * F, s));
      GWW_TRY(launch_sub_f32(sl.x_in_at(sv, l + 1), x_mid, dh, rows * d, s));
      GWW_TRY(agrad(*t, fb, F, dx, dh, d, W.b2, 1.0f, rows, F, d));
    }
    GWW_TRY(launch_gemm_f32_dx(dx, d, W.w232, fb, F, rows, F, d, s));
    GWW_TRY(launch_gelu_f32(zb, fb, fb, rows * F, s));   // d(pre-activation)
    if (const gww_dora_target* t = tt.at(l, 4))   // fc1: x = LN2(x_mid), dy = d(pre-activation), y = z
      GWW_TRY(agrad(*t, h, d, fb, zb, F, W.b1, 1.0f, rows, d, F));
    GWW_TRY(launch_gemm_f32_dx(fb, F, W.w132, dh, d, rows, d, F, s));
    GWW_TRY(launch_ln_bwd(x_mid, W.ln2w, dh, 1, dx, 1, nullptr, rows, d, s));
    // out_proj: x = ctx, dy = d(x_mid) (= dx), y = x_mid - x_in
    const float* ctx_x = last_pooled ? ctx + (size_t)(T - 1) * d : ctx;
    const long ldc = last_pooled ? (long)T * d : d;
    if (const gww_dora_target* t = tt.at(l, 3)) {
      if (last_pooled) {
        GWW_HIP(hipMemcpy2DAsync(dctx, (size_t)d * 4, sl.x_in_at(sv, l) + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                                 hipMemcpyDeviceToDevice, s));
        GWW_TRY(launch_sub_f32(x_mid, dctx, dh, (long)B * d, s));
      } else {
        GWW_TRY(launch_sub_f32(x_mid, sl.x_in_at(sv, l), dh, M * d, s));
      }
      GWW_TRY(agrad(*t, ctx_x, ldc, dx, dh, d, W.bo, 1.0f, rows, d, d));
    }
    if (last_pooled) {
      // d(ctx) rows (b, T-1) -> the dense, otherwise zero dctx; the compact residual gradient -> row T-1 of a zero dx
      GWW_TRY(launch_gemm_f32_dx(dx, d, W.wo32, dh, d, B, d, d, s));
      GWW_HIP(hipMemsetAsync(dctx, 0, (size_t)M * d * 4, s));
      GWW_HIP(hipMemcpy2DAsync(dctx + (size_t)(T - 1) * d, (size_t)T * d * 4, dh, (size_t)d * 4, (size_t)d * 4, B,
                               hipMemcpyDeviceToDevice, s));
      GWW_HIP(hipMemcpyAsync(fb, dx, (size_t)B * d * 4, hipMemcpyDeviceToDevice, s));
      GWW_HIP(hipMemsetAsync(dx, 0, (size_t)M * d * 4, s));
      GWW_HIP(hipMemcpy2DAsync(dx + (size_t)(T - 1) * d, (size_t)T * d * 4, fb, (size_t)d * 4, (size_t)d * 4, B,
                               hipMemcpyDeviceToDevice, s));
    } else {
      GWW_TRY(launch_gemm_f32_dx(dx, d, W.wo32, dctx, d, M, d, d, s));
    }
    GWW_TRY(launch_attention_bwd_f32(qkv, ctx, dctx, lse, Dv, dqkv, B, T, H, s));
    // q / k / v adapters: x = LN1(x_in) (recomputed), dy / y = the q | k | v sections of dqkv / qkv
    bool have_h1 = false;
    for (int pr = 0; pr < 3; ++pr) {
      const gww_dora_target* t = tt.at(l, pr);
      if (!t) continue;
      if (!have_h1) {
        GWW_TRY(launch_layernorm(sl.x_in_at(sv, l), W.ln1w, W.ln1b, h, 0, M, d, s));
        have_h1 = true;
      }
      const long off = (long)pr * d;
      GWW_TRY(agrad(*t, h, d, dqkv + off, qkv + off, 3L * d, W.bqkv + off, pr == 0 ? q_ysc : 1.0f, M, d, d));
    }
    // below layer 0 the gradient only continues into LN1 of layer 0 and the conv stem
    if (l == 0 && !d_x0 && !d_mel) break;
    GWW_TRY(launch_gemm_f32_dx(dqkv, 3L * d, W.wqkv32, dh, d, M, d, 3 * d, s));
    GWW_TRY(launch_ln_bwd(sl.x_in_at(sv, l), W.ln1w, dh, 1, dx, 1, nullptr, M, d, s));
  }
  if (d_x0) GWW_HIP(hipMemcpyAsync(d_x0, dx, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
  return d_mel ? stem_backward(e, base, w, dx, d_mel, B, s) : GWW_OK;
}
