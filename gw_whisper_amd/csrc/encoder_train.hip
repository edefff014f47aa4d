// DoRA training step (bf16): forward that keeps the activations the backward needs, and the
// backward through the whole layer stack down to the residual stream entering layer 0.
// Plain per-op path (LayerNorm kernel, generic GEMM with residual epilogue): the weights are
// frozen, so there are no weight-gradient GEMMs -- only dX GEMMs against transposed panels,
// the flash-attention backward and the rank-r DoRA parameter gradients.
//
// saved arena (caller-owned), per layer l:
//   x_in[l] f32 [Mp,d] | h1 bf16 [Mp,d] | qkv bf16 [Mp,3d] | lse f32 [B,H,T] | ctx bf16 [Mp,d] |
//   x_mid f32 [Mp,d] | z bf16 [Mp,ffn]                      and x_in[L] = input of the final LayerNorm
#include "encoder_impl.h"

using namespace gww;

namespace {
struct SavedLayout : SavedArena {
  size_t h1, qkv, lse, ctx, x_mid, z;
};
SavedLayout saved_layout(const gww_enc_cfg& c, int B) {
  const size_t d = c.d_model, F = c.ffn, T = c.t_in / 2, H = c.n_heads;
  const size_t Mp = padded_rows((size_t)B * T);
  SavedLayout s{};
  s.n_layers = c.n_layers;
  Arena a;
  s.x_in = a.take(Mp * d * 4);
  s.h1 = a.take(Mp * d * 2);
  s.qkv = a.take(Mp * 3 * d * 2);
  s.lse = a.take((size_t)B * H * T * 4);
  s.ctx = a.take(Mp * d * 2);
  s.x_mid = a.take(Mp * d * 4);
  s.z = a.take(Mp * F * 2);
  s.layer_stride = a.total();
  s.total = s.layer_stride * c.n_layers + align_up(Mp * d * 4);   // + x_in[L]
  return s;
}
struct TrainWs {
  size_t melT, c1, h2, f1, d2, dx, dxb, dbig, dh, dctx, dqkv, Dv, z1, col1, dgs, dgs_bytes, total;
};
TrainWs train_ws(const gww_enc_cfg& c, int B) {
  const size_t d = c.d_model, F = c.ffn, Tin = c.t_in, T = c.t_in / 2, C = c.n_mels, H = c.n_heads;
  const size_t Kc1 = conv1_kpad(c.n_mels);
  const size_t Mp = padded_rows((size_t)B * T);
  TrainWs w{};
  Arena a;
  w.melT = a.take(((size_t)B * (Tin + 2) * C + Kc1) * 2);
  w.c1 = a.take((((size_t)B * (Tin + 2) + 255) / 256 * 256 + 520) * d * 2);
  w.h2 = a.take(Mp * d * 2);      // per-op path: LN2 output; fused path: out_proj delta (fwd), recomputed LN1 output (bwd)
  w.f1 = a.take(Mp * F * 2);      // per-op path: gelu(fc1); fused path: recomputed pre-GELU fc1 output (bwd)
  w.d2 = a.take(Mp * d * 2);      // fused path: the last layer's fc2 delta
  w.dx = a.take(Mp * d * 4);
  w.dxb = a.take(Mp * d * 2);
  w.dbig = a.take(Mp * F * 2);
  w.dh = a.take(Mp * d * 2);
  w.dctx = a.take(Mp * d * 2);
  w.dqkv = a.take(Mp * 3 * d * 2);
  w.Dv = a.take((size_t)B * H * (T + (T + 63) / 64) * 4);   // row dots + live-tile flags
  w.z1 = a.take(((size_t)B * (Tin + 2) + 256) * d * 2);            // stem backward: conv1 pre-activation / its gradient
  w.col1 = a.take(((size_t)B * (Tin + 2) + 256) * Kc1 * 2); // stem backward: conv1 taps side by side
  w.dgs_bytes = (d == 384 || d == 512) ? dora_grads_scratch_bytes(3, (int)d)        // DoRA-gradient partial sums
                : d == 768 ? dora_grads_scratch_bytes(1, (int)d) : 0;
  w.dgs = a.take(w.dgs_bytes);
  w.total = a.total();
  return w;
}
}  // namespace

// d = 384: the training forward runs on the fused inference kernels (GWW_TRAIN_FUSED=0: the per-op forward of round 1)
static bool train_fused(const gww_enc_cfg& c) {
  static const bool off = lab_int("GWW_TRAIN_FUSED", 1) == 0;
  return !off && mlp_fused_supported(c.d_model, c.ffn);
}

// full fine-tuning: behind the backward's workspace, the partial slabs of the weight-gradient GEMMs and of the LayerNorm
// gain / bias sums (one region, reused by every launch in stream order)
static size_t train_param_scratch_bytes(const gww_enc_cfg& c, int B) {
  const long d = c.d_model, F = c.ffn, T = c.t_in / 2, M = (long)B * T;
  size_t mx = 0;
  for (long m : {M, (long)B}) {
    mx = std::max(mx, wgrad_workspace_bytes(m, (int)d, (int)d));
    mx = std::max(mx, wgrad_workspace_bytes(m, (int)F, (int)d));
    mx = std::max(mx, wgrad_workspace_bytes(m, (int)d, (int)F));
    mx = std::max(mx, ln_param_grads_workspace_bytes(m, (int)d));
  }
  mx = std::max(mx, wgrad_workspace_bytes((long)B * (T + 1), (int)d, 3 * (int)d));
  mx = std::max(mx, wgrad_workspace_bytes((long)B * (c.t_in + 2), (int)d, conv1_kpad(c.n_mels)));
  return align_up(mx);
}

extern "C" size_t gww_train_workspace_bytes_full(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? train_ws(e->cfg, batch).total + train_param_scratch_bytes(e->cfg, batch) : 0;
}

// fc1 / fc2 targets and ranks other than 8 (the adapter-gradient kernel): its scratch for the largest target shape,
// behind the backward's workspace (and behind the full fine-tuning region, should both be asked for)
static size_t train_adapter_scratch_bytes(const gww_enc_cfg& c, int B, int max_r) {
  const long M = (long)B * (c.t_in / 2);
  const int d = c.d_model, F = c.ffn;
  size_t mx = 0;
  for (int di : {d, F})
    for (int dd : {d, F}) mx = std::max(mx, adapter_grads_scratch_bytes(M, di, dd, max_r));
  return align_up(mx);
}

extern "C" size_t gww_train_workspace_bytes_adapters(const gww_encoder* e, int batch, int max_r) {
  return (e && batch > 0 && max_r >= 1 && max_r <= 64)
             ? train_ws(e->cfg, batch).total + train_adapter_scratch_bytes(e->cfg, batch, max_r) : 0;
}

extern "C" size_t gww_train_saved_bytes(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? saved_layout(e->cfg, batch).total : 0;
}
extern "C" size_t gww_train_workspace_bytes(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? train_ws(e->cfg, batch).total : 0;
}

// The last layer of a pooled step above its attention, on both forward paths.  Only token T-1 of the output is used
// (Signal_vs_Noise/src/model.py:25-26), and past the last attention every op is row-wise: out_proj / LN2 / fc1 / GELU /
// fc2 / final LN run on the B last-token rows alone.  x_mid, z and x_in[L] (= x_out) of this layer are saved COMPACT
// ([B, .]) -- the pooled backward expects exactly that.  xl: [B, d] fp32 of scratch for the x_in[L-1] rows (b, T-1) (the
// gradient buffers are idle in the forward); h2 / f1: the workspace's LN2 output and gelu(fc1) buffers.
static int train_pooled_tail(gww_encoder* e, const LayerW& W, const float* x_in, const void* ctx, float* xl, float* x_mid,
                             void* h2, void* z, void* f1, float* x_out, float* last_hidden, int B, hipStream_t s) {
  const int d = e->cfg.d_model, F = e->cfg.ffn, T = e->cfg.t_in / 2;
  GWW_HIP(hipMemcpy2DAsync(xl, (size_t)d * 4, x_in + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                           hipMemcpyDeviceToDevice, s));
  GWW_TRY(launch_gemm_bf16((const unsigned short*)ctx + (size_t)(T - 1) * d, (long)T * d, W.wo, W.bo, xl, nullptr,
                           x_mid, B, d, d, EPI_RESID, 0, s, 0));
  GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, h2, 1, B, d, s));
  GWW_TRY(launch_gemm_bf16(h2, d, W.w1, W.b1, nullptr, nullptr, z, B, F, d, EPI_BIAS, 0, s, 0));
  GWW_TRY(launch_gelu_bf16(z, nullptr, f1, (((long)B * F + 7) / 8) * 8, s));
  GWW_TRY(launch_gemm_bf16(f1, F, W.w2, W.b2, x_mid, nullptr, x_out, B, d, F, EPI_RESID, 0, s, 0));
  return launch_layernorm(x_out, e->lnw, e->lnb, last_hidden, 0, B, d, s);
}

extern "C" int gww_encoder_train_forward(gww_encoder* e, const float* mel, int batch, void* workspace,
                                         size_t workspace_bytes, void* saved, size_t saved_bytes,
                                         float* last_hidden, int pooled, void* stream) {
  GWW_REQUIRE(e && mel && workspace && saved && last_hidden, "gww_encoder_train_forward: NULL argument");
  if (!e->ready) return fail(GWW_ERR_STATE, "gww_encoder_train_forward: weights not set");
  GWW_REQUIRE(batch > 0, "gww_encoder_train_forward: batch must be positive");
  const SavedLayout sl = saved_layout(e->cfg, batch);
  const TrainWs w = train_ws(e->cfg, batch);
  if (workspace_bytes < w.total || saved_bytes < sl.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_forward: workspace %zu / saved %zu bytes < required %zu / %zu",
                workspace_bytes, saved_bytes, w.total, sl.total);
  hipStream_t s = (hipStream_t)stream;
  const int d = e->cfg.d_model, F = e->cfg.ffn, Tin = e->cfg.t_in, T = Tin / 2, C = e->cfg.n_mels, H = e->cfg.n_heads;
  const int Kc1 = conv1_kpad(C);
  const int B = batch, L = e->cfg.n_layers;
  const long M = (long)B * T;
  char* base = (char*)workspace;
  char* sv = (char*)saved;
  void* melT = base + w.melT;
  void* c1 = base + w.c1;
  void* h2 = base + w.h2;
  void* f1 = base + w.f1;
  // ---- stem (same kernels as inference) -> x_in[0]
  GWW_TRY(launch_mel_to_tokens(mel, melT, 1, B, C, Tin, s));
  GWW_HIP(hipMemsetAsync((char*)melT + (size_t)B * (Tin + 2) * C * 2, 0, Kc1 * 2, s));
  GWW_HIP(hipMemsetAsync(c1, 0, (size_t)d * 2, s));
  if (train_fused(e->cfg)) {   // the inference stem kernels (A-stationary conv1, full-N conv2)
    GWW_TRY(launch_gemm_astat(melT, C, nullptr, nullptr, nullptr, nullptr, e->c1w, e->c1b, c1, (long)B * (Tin + 2), d,
                              Kc1, EPI_CONV1, Tin + 2, s));
    GWW_TRY(launch_gemm_bf16_v4(c1, 2L * d, e->c2w, e->c2b, nullptr, sl.x_in_at(sv, 0), (long)B * (T + 1), (d + 255) / 256 * 256, 3 * d,
                                EPI_CONV2, s, 0, e->pos, T + 1, d, (float*)h2));   // (h2 is idle here: the scratch row of the garbage rows)
  } else {
    GWW_TRY(launch_gemm_bf16(melT, C, e->c1w, e->c1b, nullptr, nullptr, c1, (long)B * (Tin + 2), d, Kc1, EPI_CONV1,
                             Tin + 2, s, 0));
    GWW_TRY(launch_gemm_bf16(c1, 2L * d, e->c2w, e->c2b, nullptr, e->pos, sl.x_in_at(sv, 0), (long)B * (T + 1), d, 3 * d, EPI_CONV2,
                             T + 1, s, 1));
  }
  const bool fast = (d == 384 || d == 512) && F % 128 == 0;   // A-stationary kernel for the K = d GEMMs without a residual
  if (train_fused(e->cfg)) {
    // ---- fused forward (d = 384): the INFERENCE kernels -- LayerNorm-folded A-stationary q/k/v GEMM for layer 0, flash
    // attention (+ lse), out_proj as a bf16 delta, fused MLP + the next layer's LN1 + q/k/v -- writing what the
    // backward needs straight into the arena: x_in[l], qkv, lse, ctx, x_mid (= x_in + out_proj, the fused kernel's
    // x_new).  LN1 / LN2 outputs and the pre-GELU fc1 output are NOT kept: the backward recomputes them (that is what
    // the reference's gradient_checkpointing_enable() at MLGWSC-1/train.py:662 trades, too).
    void* d1 = h2;
    void* d2 = base + w.d2;
    const bool q_log2 = attention_log2q_enabled();
    for (int l = 0; l < L; ++l) {
      const LayerW& W = e->layers[l];
      char* lb = sv + (size_t)l * sl.layer_stride;
      void* qkv = lb + sl.qkv;
      float* lse = (float*)(lb + sl.lse);
      void* ctx = lb + sl.ctx;
      float* x_mid = (float*)(lb + sl.x_mid);
      void* z = lb + sl.z;
      if (l == 0) {
        // layer 0: LN1 + q / k / v on the fused block's panel prologue + tail (k_mlp_fused<2, false>), as the inference
        // forward does (round 3 ran the LayerNorm kernel + the plain A-stationary GEMM here: 41 + 112 us at 64 segments)
        MlpFusedArgs a;
        a.who = "gww_encoder_train_forward"; a.x = sl.x_in_at(sv, 0); a.Wt = W.wqkv_st; a.M = M; a.d = d;
        a.qkv_u = W.uqkv; a.qkv_cb = W.cbqkv; a.qkv_out = qkv; a.NQ = 3 * d;
        GWW_TRY(launch_mlp_fused(a, s));
      }
      if (pooled && l == L - 1) {
        // only the query tile that holds token T - 1 is needed (forward and backward): the other rows of ctx / lse stay
        // zero so that the backward's row dots see finite values
        GWW_HIP(hipMemsetAsync(ctx, 0, (size_t)M * d * 2, s));
        GWW_HIP(hipMemsetAsync(lse, 0, (size_t)B * H * T * 4, s));
        GWW_TRY(launch_attention_bf16(qkv, ctx, B, T, H, s, lse, /*last_tile_only=*/true, q_log2));
        return train_pooled_tail(e, W, sl.x_in_at(sv, l), ctx, (float*)(base + w.dx), x_mid, h2, z, f1, sl.x_in_at(sv, L),
                                 last_hidden, B, s);
      }
      GWW_TRY(launch_attention_bf16(qkv, ctx, B, T, H, s, lse, false, q_log2));
      // out_proj fused in front of the block as on the inference path: x_mid = x_in + bf16(ctx W_o^T + bo) comes out of
      // the kernel's seam and is kept (the backward needs ctx and x_mid, never the delta)
      MlpFusedArgs a;
      a.who = "gww_encoder_train_forward"; a.x = sl.x_in_at(sv, l); a.x_new = x_mid; a.keep_x_new = true;
      a.ln_u = W.u1; a.ln_cb = W.cb1; a.b2 = W.b2; a.M = M; a.d = d; a.F = F;
      if (generic_path_mask() & GP_OUT_PROJ) {
        GWW_TRY(launch_gemm_astat(ctx, d, nullptr, nullptr, nullptr, nullptr, W.wo, W.bo, d1, M, d, d, EPI_BIAS, 0, s));
        a.delta = d1; a.Wt = W.wmlp;
      } else {
        a.ctx = ctx; a.bo = W.bo; a.Wt = W.wmlp_op;
      }
      if (l + 1 < L) {   // the next layer's LN1 + q / k / v behind the block, x_next straight into the arena
        const LayerW& Wn = e->layers[l + 1];
        a.qkv_u = Wn.uqkv; a.qkv_cb = Wn.cbqkv; a.qkv_out = sv + (size_t)(l + 1) * sl.layer_stride + sl.qkv; a.NQ = 3 * d;
        a.x_next = sl.x_in_at(sv, l + 1);
        GWW_TRY(launch_mlp_fused(a, s));
      } else {
        a.C = d2;
        GWW_TRY(launch_mlp_fused(a, s));
        GWW_TRY(launch_add_delta_f32(x_mid, d2, sl.x_in_at(sv, L), M * d, s));
      }
    }
    GWW_TRY(launch_layernorm(sl.x_in_at(sv, L), e->lnw, e->lnb, last_hidden, 0, M, d, s));
    return GWW_OK;
  }
  for (int l = 0; l < L; ++l) {
    const LayerW& W = e->layers[l];
    char* lb = sv + (size_t)l * sl.layer_stride;
    void* h1 = lb + sl.h1;
    void* qkv = lb + sl.qkv;
    float* lse = (float*)(lb + sl.lse);
    void* ctx = lb + sl.ctx;
    float* x_mid = (float*)(lb + sl.x_mid);
    void* z = lb + sl.z;
    GWW_TRY(launch_layernorm(sl.x_in_at(sv, l), W.ln1w, W.ln1b, h1, 1, M, d, s));
    if (fast) GWW_TRY(launch_gemm_astat(h1, d, nullptr, nullptr, nullptr, nullptr, W.wqkv, W.bqkv16, qkv, M, 3 * d, d, EPI_BIAS, 0, s));
    else GWW_TRY(launch_gemm_bf16(h1, d, W.wqkv, W.bqkv16, nullptr, nullptr, qkv, M, 3 * d, d, EPI_BIAS, 0, s, 1));
    GWW_TRY(launch_attention_bf16(qkv, ctx, B, T, H, s, lse, false, attention_log2q_enabled()));
    if (pooled && l == L - 1) {
      return train_pooled_tail(e, W, sl.x_in_at(sv, l), ctx, (float*)(base + w.dx), x_mid, h2, z, f1, sl.x_in_at(sv, L),
                               last_hidden, B, s);
    }
    GWW_TRY(launch_gemm_bf16(ctx, d, W.wo, W.bo, sl.x_in_at(sv, l), nullptr, x_mid, M, d, d, EPI_RESID, 0, s, 1));
    GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, h2, 1, M, d, s));
    if (fast) GWW_TRY(launch_gemm_astat(h2, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, z, M, F, d, EPI_BIAS, 0, s));
    else GWW_TRY(launch_gemm_bf16(h2, d, W.w1, W.b1, nullptr, nullptr, z, M, F, d, EPI_BIAS, 0, s, 1));
    GWW_TRY(launch_gelu_bf16(z, nullptr, f1, ((M * F + 7) / 8) * 8, s));
    GWW_TRY(launch_gemm_bf16(f1, F, W.w2, W.b2, x_mid, nullptr, sl.x_in_at(sv, l + 1), M, d, F, EPI_RESID, 0, s, 1));
  }
  GWW_TRY(launch_layernorm(sl.x_in_at(sv, L), e->lnw, e->lnb, last_hidden, 0, M, d, s));
  return GWW_OK;
}

// d_last_hidden: fp32 [B*T, d] gradient of the loss w.r.t. last_hidden_state.
// targets: DoRA-adapted projections whose A / B / magnitude gradients are wanted; the gradient buffers
// are ACCUMULATED into (zero them once per step).  d_x0 (optional, fp32 [B*T, d]): gradient w.r.t. the
// residual stream entering layer 0 (the conv stem output).  d_mel (optional, fp32 [B, n_mels, t_in]): gradient
// w.r.t. the input features, through the conv stem (MLGWSC-1/train.py:494-504 trains its Q-adapter through
// the frozen encoder).
//
// grads (full fine-tuning, may be NULL): fp32 gradients of the base parameters, accumulated into.  Each weight gradient
// is a weight-gradient GEMM (wgrad.hip) of a gradient / activation pair this backward already has in hand:
//   fc2: d(x_out) x gelu(fc1(LN2 x_mid))    fc1: d(fc1 pre-act) x LN2(x_mid)    out_proj: d(x_mid) x ctx
//   q / k / v: dqkv x LN1(x_in) (q with the q_ysc of the stored q)     conv2 / conv1: dz2 / dz1 x im2col views
// and the LayerNorm gains / biases and the positions are fixed-order column sums.
static int train_backward_impl(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes, const void* saved,
                               size_t saved_bytes, const float* d_last_hidden, const gww_dora_target* targets,
                               int n_targets, float* d_x0, float* d_mel, int pooled, const gww_enc_grads* grads,
                               hipStream_t s) {
  GWW_REQUIRE(e && workspace && saved && d_last_hidden, "gww_encoder_train_backward: NULL argument");
  GWW_REQUIRE(batch > 0 && n_targets >= 0 && (n_targets == 0 || targets), "gww_encoder_train_backward: bad argument");
  const SavedLayout sl = saved_layout(e->cfg, batch);
  const TrainWs w = train_ws(e->cfg, batch);
  if (workspace_bytes < w.total || saved_bytes < sl.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_backward: workspace / saved arena too small");
  const size_t pscr_bytes = grads ? train_param_scratch_bytes(e->cfg, batch) : 0;
  if (grads && workspace_bytes < w.total + pscr_bytes)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_backward_full: workspace %zu bytes < required %zu (base gradients)",
                workspace_bytes, w.total + pscr_bytes);
  const int d = e->cfg.d_model, F = e->cfg.ffn, T = e->cfg.t_in / 2, H = e->cfg.n_heads;
  const int B = batch, L = e->cfg.n_layers;
  const long M = (long)B * T;
  char* base = (char*)workspace;
  const char* sv = (const char*)saved;
  float* dx = (float*)(base + w.dx);
  void* dxb = base + w.dxb;
  void* dbig = base + w.dbig;
  void* dh = base + w.dh;
  void* dctx = base + w.dctx;
  void* dqkv = base + w.dqkv;
  float* Dv = (float*)(base + w.Dv);
  // ---- base-parameter gradients (full fine-tuning)
  void* pscr = base + w.total;
  void* f1 = base + w.f1;   // gelu(fc1) recomputed for the fc2 weight gradient (idle in the backward otherwise)
  void* ln2o = base + w.d2; // LN2(x_mid) recomputed for the fc1 weight gradient (per-op and pooled paths)
  auto wg = [&](const void* dY, long ldy, const void* X, long ldx, long rows, int N, int K, float alpha, float* dW,
                float* db, int cin) -> int {
    if (!dW && !db) return GWW_OK;
    return launch_wgrad(dY, ldy, X, ldx, rows, N, K, alpha, dW, db, cin, pscr, pscr_bytes, s);
  };
  auto lng = [&](const float* x, const void* dy, int dy_f32, long rows, float* dg, float* db) -> int {
    if (!dg && !db) return GWW_OK;
    return launch_ln_param_grads(x, dy, dy_f32, rows, d, dg, db, pscr, pscr_bytes, s);
  };
  static const gww_enc_layer_grads no_layer_grads{};
  auto LGf = [&](int l) -> const gww_enc_layer_grads& {
    return (grads && grads->layers) ? grads->layers[l] : no_layer_grads;
  };
  const bool want_conv2 = grads && (grads->conv2_w || grads->conv2_b);
  const bool want_conv1 = grads && (grads->conv1_w || grads->conv1_b);
  const bool want_stem = want_conv1 || want_conv2 || (grads && grads->pos);
  const bool want_ln1_0 = L > 0 && (LGf(0).ln1_w || LGf(0).ln1_b);
  for (int i = 0; i < n_targets; ++i) {
    const gww_dora_target& t = targets[i];
    GWW_REQUIRE(t.layer >= 0 && t.layer < L && t.proj >= 0 && t.proj <= 5, "gww_encoder_train_backward: bad target %d", i);
    GWW_REQUIRE(t.r >= 1 && t.r <= 64, "gww_encoder_train_backward: target %d has rank %d: adapter gradients support "
                "ranks 1..64", i, t.r);
    GWW_REQUIRE(t.A && t.B && t.mag && t.nrm && t.dA && t.dB && t.dm, "gww_encoder_train_backward: NULL pointer in target %d", i);
  }
  // dX GEMMs: A-stationary kernel for the K <= 512 contractions, full-N kernel for the long-K, N = d ones
  // (d = 384 / 512); generic tiles otherwise.  All buffers are padded to whole 256-row panels.
  const bool fast = (d == 384 || d == 512) && F % 128 == 0;
  auto gemm_dx = [&](const void* A, long lda, const void* Wt, void* Cout, int N, int K) -> int {
    // the wide product of the MLP backward (d(fc1 output) = d(out) W2: N = ffn, K = d) on the 256 x 256 x 64 kernel: 113 GFLOP
    // in ~130 us against ~200 on the A-stationary kernel, whose 12 n-tile epilogues per panel run with nothing beside them
    if (fast && lda == K && N % 256 == 0 && N >= 1024 && K % 128 == 0) {
      const int rc = launch_gemm_bf16_v4(A, lda, Wt, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, s);
      if (rc != -1) return rc;
    }
    if (fast && lda == K && (K == 384 || K == 512) && N % 128 == 0)
      return launch_gemm_astat(A, lda, nullptr, nullptr, nullptr, nullptr, Wt, nullptr, Cout, M, N, K, EPI_BIAS, 0, s);
    if (fast && N == d && K % 64 == 0 && K > 512)
      return launch_gemm_fulln(A, lda, Wt, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, 0, s);
    return launch_gemm_bf16(A, lda, Wt, nullptr, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, 0, s, 1);
  };
  // the stored q is  q_ysc * (W' x + b): 1 / 8 (head_dim^-0.5), times log2(e) when the bf16 panels carry log2 units
  const float q_ysc = attention_log2q_enabled() ? 0.125f * 1.44269504088896340736f : 0.125f;
  bool multi_ok = (d == 384 || d == 512) && lab_int("GWW_DORA_OLD", 0) == 0;
  for (int i = 0; i < n_targets; ++i) multi_ok = multi_ok && (targets[i].proj > 2 || targets[i].r == 8);
  // fc1 / fc2 targets and ranks other than 8: the adapter-gradient kernel (dora_grads.hip), its scratch behind the
  // workspace when the caller sized it with gww_train_workspace_bytes_adapters (else allocated stream-ordered)
  const size_t a_off = w.total + pscr_bytes;
  void* ascr = workspace_bytes > a_off ? base + a_off : nullptr;
  const size_t ascr_bytes = workspace_bytes > a_off ? workspace_bytes - a_off : 0;
  auto agrad = [&](const gww_dora_target& t, const void* X, long ldx, const void* dY, const void* Y, long ldy,
                   const float* bias, float ysc, long rows, int d_in, int d_out) -> int {
    return launch_adapter_grads(X, ldx, dY, Y, ldy, bias, ysc, t.scaling, t.A, t.B, t.mag, t.nrm, t.dA, t.dB, t.dm, rows,
                                d_in, d_out, t.r, s, ascr, ascr_bytes);
  };
  // q / k / v / out_proj targets (d x d): the rank-8 kernels of launch_dora_grads, the adapter-gradient kernel otherwise
  auto dgrad = [&](const gww_dora_target& t, const void* X, long ldx, const void* dY, const void* Y, long ldy,
                   const float* bias, float ysc, long rows) -> int {
    if (t.r != 8) return agrad(t, X, ldx, dY, Y, ldy, bias, ysc, rows, d, d);
    return launch_dora_grads(X, ldx, dY, Y, ldy, bias, ysc, t.scaling, t.A, t.B, t.mag, t.nrm, t.dA, t.dB, t.dm, rows, d,
                             t.r, s, base + w.dgs, w.dgs_bytes);
  };
  auto find_target = [&](int l, int proj) -> const gww_dora_target* {
    for (int i = 0; i < n_targets; ++i)
      if (targets[i].layer == l && targets[i].proj == proj) return &targets[i];
    return nullptr;
  };
  // final LayerNorm backward -> dx (grad w.r.t. x_in[L]); pooled: on the B last-token rows only
  if (grads) GWW_TRY(lng(sl.x_in_at(sv, L), d_last_hidden, 1, pooled ? B : M, grads->ln_w, grads->ln_b));
  GWW_TRY(launch_ln_bwd(sl.x_in_at(sv, L), e->lnw, d_last_hidden, 1, dx, 0, dxb, pooled ? B : M, d, s));
  for (int l = L - 1; l >= 0; --l) {
    const LayerW& W = e->layers[l];
    const gww_enc_layer_grads& LG = LGf(l);
    const char* lb = sv + (size_t)l * sl.layer_stride;
    const void* h1 = lb + sl.h1;
    const void* qkv = lb + sl.qkv;
    const float* lse = (const float*)(lb + sl.lse);
    const void* ctx = lb + sl.ctx;
    const float* x_mid = (const float*)(lb + sl.x_mid);
    const void* z = lb + sl.z;
    const bool fused = train_fused(e->cfg);
    if (fused) {
      // the fused forward kept neither LN1(x_in) (the X operand of the q / k / v adapter gradients) nor the pre-GELU
      // fc1 output: LN1 is recomputed here, fc1 inside the GELU-backward GEMM below
      GWW_TRY(launch_layernorm(sl.x_in_at(sv, l), W.ln1w, W.ln1b, base + w.h2, 1, M, d, s));
      h1 = base + w.h2;
    }
    if (pooled && l == L - 1) {
      // ---- last layer of a pooled step: everything above the attention lives on the B last-token rows
      // (x_mid, z, x_in[L] were saved compact by the pooled forward); the attention backward then sees a dctx
      // that is zero except for row T-1 of every segment and skips the dead query tiles.
      GWW_TRY(launch_gemm_bf16(dxb, d, W.w2T, nullptr, nullptr, nullptr, dbig, B, F, d, EPI_BIAS, 0, s, 0));
      if (LG.fc2_w || LG.fc2_b) {   // z was saved compact by the pooled forward (both paths)
        GWW_TRY(launch_gelu_bf16(z, nullptr, f1, (((long)B * F + 7) / 8) * 8, s));
        GWW_TRY(wg(dxb, d, f1, F, B, d, F, 1.0f, LG.fc2_w, LG.fc2_b, 0));
      }
      GWW_TRY(launch_gelu_bf16(z, dbig, dbig, (((long)B * F + 7) / 8) * 8, s));
      const gww_dora_target* fc1t = find_target(l, 4);
      const gww_dora_target* fc2t = find_target(l, 5);
      if (LG.fc1_w || LG.fc1_b || fc1t) GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, ln2o, 1, B, d, s));
      if (LG.fc1_w || LG.fc1_b) GWW_TRY(wg(dbig, F, ln2o, d, B, F, d, 1.0f, LG.fc1_w, LG.fc1_b, 0));
      // fc1 adapter: x = LN2(x_mid), dy = d(pre-activation), y = z;  fc2: x = gelu(z), dy = d(x_out), y = x_out - x_mid
      if (fc1t) GWW_TRY(agrad(*fc1t, ln2o, d, dbig, z, F, W.b1, 1.0f, B, d, F));
      if (fc2t) {
        GWW_TRY(launch_gelu_bf16(z, nullptr, f1, (((long)B * F + 7) / 8) * 8, s));
        GWW_TRY(launch_sub_f32_bf16(sl.x_in_at(sv, L), x_mid, dh, (long)B * d, s));
        GWW_TRY(agrad(*fc2t, f1, F, dxb, dh, d, W.b2, 1.0f, B, F, d));
      }
      GWW_TRY(launch_gemm_bf16(dbig, F, W.w1T, nullptr, nullptr, nullptr, dh, B, d, F, EPI_BIAS, 0, s, 0));
      GWW_TRY(lng(x_mid, dh, 0, B, LG.ln2_w, LG.ln2_b));
      GWW_TRY(launch_ln_bwd(x_mid, W.ln2w, dh, 0, dx, 1, dxb, B, d, s));
      const unsigned short* ctx_last = (const unsigned short*)ctx + (size_t)(T - 1) * d;
      bool have_y = false;
      for (int i = 0; i < n_targets; ++i) {
        const gww_dora_target& t = targets[i];
        if (t.layer != l || t.proj != 3) continue;
        if (!have_y) {   // y = x_mid - x_in on the last-token rows
          float* xl = (float*)dbig;
          GWW_HIP(hipMemcpy2DAsync(xl, (size_t)d * 4, sl.x_in_at(sv, l) + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4,
                                   B, hipMemcpyDeviceToDevice, s));
          GWW_TRY(launch_sub_f32_bf16(x_mid, xl, dh, (long)B * d, s));
          have_y = true;
        }
        GWW_TRY(dgrad(t, ctx_last, (long)T * d, dxb, dh, d, W.bo, 1.0f, B));
      }
      GWW_TRY(wg(dxb, d, ctx_last, (long)T * d, B, d, d, 1.0f, LG.o_w, LG.o_b, 0));
      // d(ctx) rows (b, T-1) -> the dense, otherwise zero dctx
      GWW_TRY(launch_gemm_bf16(dxb, d, W.woT, nullptr, nullptr, nullptr, dh, B, d, d, EPI_BIAS, 0, s, 0));
      GWW_HIP(hipMemsetAsync(dctx, 0, (size_t)M * d * 2, s));
      GWW_HIP(hipMemcpy2DAsync((unsigned short*)dctx + (size_t)(T - 1) * d, (size_t)T * d * 2, dh, (size_t)d * 2,
                               (size_t)d * 2, B, hipMemcpyDeviceToDevice, s));
      // the residual gradient likewise: compact dx -> row T-1 of a zero dense dx
      GWW_HIP(hipMemcpyAsync(dbig, dx, (size_t)B * d * 4, hipMemcpyDeviceToDevice, s));
      GWW_HIP(hipMemsetAsync(dx, 0, (size_t)M * d * 4, s));
      GWW_HIP(hipMemcpy2DAsync(dx + (size_t)(T - 1) * d, (size_t)T * d * 4, dbig, (size_t)d * 4, (size_t)d * 4, B,
                               hipMemcpyDeviceToDevice, s));
    } else {
    // fc2 / GELU / fc1 / LN2   (x_out = x_mid + fc2(gelu(fc1(LN2(x_mid)))))
    GWW_TRY(gemm_dx(dxb, d, W.w2T, dbig, F, d));
    const bool want_fc2 = LG.fc2_w || LG.fc2_b;
    const void* ln2_out = nullptr;   // LN2(x_mid), when a weight gradient needs it
    const gww_dora_target* fc1t = find_target(l, 4);
    const gww_dora_target* fc2t = find_target(l, 5);
    if (fc1t || fc2t) {
      // fc1 / fc2 adapters.  fc1: x = LN2(x_mid), dy = d(pre-activation), y = z (+ b1);  fc2: x = gelu(z),
      // dy = d(x_out) (dxb), y = x_out - x_mid (+ b2).  The fused forward kept no z: it is recomputed into f1 by the
      // A-stationary GEMM with the plain bias epilogue, and the GELU backward reads it from there.
      const void* zz = z;
      if (fused) {
        GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, dctx, 1, M, d, s));
        ln2_out = dctx;
        GWW_TRY(launch_gemm_astat(dctx, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, f1, M, F, d, EPI_BIAS, 0, s));
        zz = f1;
      } else if (fc1t) {
        GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, ln2o, 1, M, d, s));
        ln2_out = ln2o;
      }
      GWW_TRY(launch_gelu_bf16(zz, dbig, dbig, ((M * F + 7) / 8) * 8, s));
      if (fc1t) GWW_TRY(agrad(*fc1t, ln2_out, d, dbig, zz, F, W.b1, 1.0f, M, d, F));
      if (fc2t || want_fc2) GWW_TRY(launch_gelu_bf16(zz, nullptr, f1, ((M * F + 7) / 8) * 8, s));   // in place when fused
      if (fc2t) {
        GWW_TRY(launch_sub_f32_bf16(sl.x_in_at(sv, l + 1), x_mid, dh, M * d, s));
        GWW_TRY(agrad(*fc2t, f1, F, dxb, dh, d, W.b2, 1.0f, M, F, d));
      }
    } else if (fused) {
      // recompute: LN2(x_mid) (LayerNorm kernel, into the idle dctx buffer) -> fc1 as a plain A-stationary GEMM whose
      // epilogue applies gelu'(pre-activation) to the gradient in place: neither the pre-activation nor a separate
      // GELU-backward pass touches HBM
      GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, dctx, 1, M, d, s));
      ln2_out = dctx;
      // full fine-tuning: gelu(fc1(LN2 x_mid)), the fc2 weight gradient's X operand, is not kept by the fused forward
      if (want_fc2)
        GWW_TRY(launch_gemm_astat(dctx, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, f1, M, F, d, EPI_GELU, 0, s));
      GWW_TRY(launch_gemm_astat(dctx, d, dbig, nullptr, nullptr, nullptr, W.w1, W.b1, dbig, M, F, d, EPI_DGELU, 0, s));
    } else {
      if (want_fc2) GWW_TRY(launch_gelu_bf16(z, nullptr, f1, ((M * F + 7) / 8) * 8, s));
      GWW_TRY(launch_gelu_bf16(z, dbig, dbig, ((M * F + 7) / 8) * 8, s));
    }
    GWW_TRY(wg(dxb, d, f1, F, M, d, F, 1.0f, LG.fc2_w, LG.fc2_b, 0));
    if (LG.fc1_w || LG.fc1_b) {
      if (!ln2_out) {
        GWW_TRY(launch_layernorm(x_mid, W.ln2w, W.ln2b, ln2o, 1, M, d, s));
        ln2_out = ln2o;
      }
      GWW_TRY(wg(dbig, F, ln2_out, d, M, F, d, 1.0f, LG.fc1_w, LG.fc1_b, 0));
    }
    GWW_TRY(gemm_dx(dbig, F, W.w1T, dh, d, F));
    GWW_TRY(lng(x_mid, dh, 0, M, LG.ln2_w, LG.ln2_b));
    GWW_TRY(launch_ln_bwd(x_mid, W.ln2w, dh, 0, dx, 1, dxb, M, d, s));
    // out_proj / attention / QKV / LN1   (x_mid = x_in + out_proj(attn(qkv(LN1(x_in)))))
    {   // out_proj DoRA targets: x = ctx, dy = d(x_mid) (= dxb), y = x_mid - x_in (rebuilt into dh, free here)
      bool have_y = false;
      for (int i = 0; i < n_targets; ++i) {
        const gww_dora_target& t = targets[i];
        if (t.layer != l || t.proj != 3) continue;
        if (!have_y) {
          GWW_TRY(launch_sub_f32_bf16(x_mid, sl.x_in_at(sv, l), dh, M * d, s));
          have_y = true;
        }
        GWW_TRY(dgrad(t, ctx, d, dxb, dh, d, W.bo, 1.0f, M));
      }
    }
    GWW_TRY(wg(dxb, d, ctx, d, M, d, d, 1.0f, LG.o_w, LG.o_b, 0));
    GWW_TRY(gemm_dx(dxb, d, W.woT, dctx, d, d));
    }
    GWW_TRY(launch_attention_bwd_bf16(qkv, ctx, dctx, lse, Dv, dqkv, B, T, H, s, attention_log2q_enabled()));
    if (multi_ok) {
      // q / k / v adapters of this layer read the same h1: one pass over h1, dqkv and qkv on the matrix cores
      long off[3];
      const float *bias[3], *Aa[3], *Bb[3], *mg[3], *nr[3];
      float ysc[3], scl[3], *dAa[3], *dBb[3], *dmm[3];
      int np = 0;
      for (int i = 0; i < n_targets; ++i) {
        const gww_dora_target& t = targets[i];
        if (t.layer != l || t.proj > 2) continue;
        GWW_REQUIRE(np < 3, "gww_encoder_train_backward: duplicate q/k/v target in layer %d", l);
        off[np] = (long)t.proj * d;
        bias[np] = W.bqkv16 + off[np];
        ysc[np] = t.proj == 0 ? q_ysc : 1.0f;
        scl[np] = t.scaling;
        Aa[np] = t.A; Bb[np] = t.B; mg[np] = t.mag; nr[np] = t.nrm;
        dAa[np] = t.dA; dBb[np] = t.dB; dmm[np] = t.dm;
        ++np;
      }
      if (np > 0)
        GWW_TRY(launch_dora_grads_multi(h1, d, dqkv, qkv, 3L * d, np, off, bias, ysc, scl, Aa, Bb, mg, nr, dAa, dBb, dmm, M,
                                        d, s, base + w.dgs, w.dgs_bytes));
    } else {
      for (int i = 0; i < n_targets; ++i) {
        const gww_dora_target& t = targets[i];
        if (t.layer != l || t.proj > 2) continue;
        const long off = (long)t.proj * d;   // q | k | v section
        GWW_TRY(dgrad(t, h1, d, (const unsigned short*)dqkv + off, (const unsigned short*)qkv + off, 3L * d, W.bqkv16 + off,
                      t.proj == 0 ? q_ysc : 1.0f, M));
      }
    }
    // q / k / v weight gradients: dqkv is the gradient of the STORED q (q_ysc (W x + b)), k has no bias
    GWW_TRY(wg(dqkv, 3L * d, h1, d, M, d, d, q_ysc, LG.q_w, LG.q_b, 0));
    GWW_TRY(wg((const unsigned short*)dqkv + d, 3L * d, h1, d, M, d, d, 1.0f, LG.k_w, nullptr, 0));
    GWW_TRY(wg((const unsigned short*)dqkv + 2 * d, 3L * d, h1, d, M, d, d, 1.0f, LG.v_w, LG.v_b, 0));
    // below layer 0 the gradient only continues into LN1 of layer 0 and the conv stem: skip it when nobody asked for
    // d_x0 / d_mel or one of their parameter gradients
    if (l == 0 && !d_x0 && !d_mel && !want_stem && !want_ln1_0) break;
    GWW_TRY(gemm_dx(dqkv, 3L * d, W.wqkvT, dh, d, 3 * d));
    GWW_TRY(lng(sl.x_in_at(sv, l), dh, 0, M, LG.ln1_w, LG.ln1_b));
    GWW_TRY(launch_ln_bwd(sl.x_in_at(sv, l), W.ln1w, dh, 0, dx, 1, dxb, M, d, s));
  }
  if (d_x0) GWW_HIP(hipMemcpyAsync(d_x0, dx, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
  if (grads && grads->pos) GWW_TRY(launch_pos_grad(dx, grads->pos, B, T, d, s));   // x0 = gelu(conv2) + pos
  if (d_mel || want_conv1 || want_conv2) {
    // ---- conv stem backward: x0 = gelu(conv2(gelu(conv1(mel)))) + pos (melT and c1 of the forward are still
    // in the workspace); the pre-activations are recomputed by the same GEMMs with a plain bias epilogue
    const int Tin = e->cfg.t_in, C = e->cfg.n_mels, Kc1 = conv1_kpad(C);
    GWW_REQUIRE(B <= 512, "gww_encoder_train_backward: d_mel and the conv-stem gradients support batch <= 512");
    const void* melT = base + w.melT;
    const void* c1 = base + w.c1;
    void* z1 = base + w.z1;
    void* col1 = base + w.col1;
    const long M2 = (long)B * (T + 1), M1 = (long)B * (Tin + 2);
    GWW_TRY(launch_gemm_bf16(c1, 2L * d, e->c2w, e->c2b, nullptr, nullptr, dh, M2, d, 3 * d, EPI_BIAS, 0, s, 0));       // z2
    GWW_TRY(launch_stem_dz2(dxb, dh, dctx, B, T, d, s));                                                              // dz2
    // conv2 weight gradient on the forward's im2col view of c1 (row m: padded rows 2 t .. 2 t + 2); the junk row
    // t = T of every segment has dz2 = 0
    if (want_conv2) GWW_TRY(wg(dctx, d, c1, 2L * d, M2, d, 3 * d, 1.0f, grads->conv2_w, grads->conv2_b, d));
    if (d_mel || want_conv1) {
      GWW_TRY(launch_gemm_bf16(dctx, d, e->c2wT, nullptr, nullptr, nullptr, dqkv, M2, 3 * d, d, EPI_BIAS, 0, s, 0));   // col
      GWW_TRY(launch_gemm_bf16(melT, C, e->c1w, e->c1b, nullptr, nullptr, z1, M1, d, Kc1, EPI_BIAS, 0, s, 0));  // z1
      GWW_TRY(launch_stem_dz1(dqkv, z1, z1, B, T, Tin, d, s));                                                        // dz1
      // conv1 weight gradient on the im2col view of melT (K = Kc1: taps 0..2 of C channels + padding, dropped)
      if (want_conv1) GWW_TRY(wg(z1, d, melT, C, M1, d, Kc1, 1.0f, grads->conv1_w, grads->conv1_b, C));
    }
    if (d_mel) {
      GWW_TRY(launch_gemm_bf16(z1, d, e->c1wT, nullptr, nullptr, nullptr, col1, M1, Kc1, d, EPI_BIAS, 0, s, 0));  // col1
      GWW_TRY(launch_stem_dmel(col1, d_mel, B, Tin, C, Kc1, s));
    }
  }
  return GWW_OK;
}

extern "C" int gww_encoder_train_backward(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes,
                                          const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                          const gww_dora_target* targets, int n_targets, float* d_x0,
                                          float* d_mel, int pooled, void* stream) {
  return train_backward_impl(e, batch, workspace, workspace_bytes, saved, saved_bytes, d_last_hidden, targets, n_targets,
                             d_x0, d_mel, pooled, nullptr, (hipStream_t)stream);
}

extern "C" int gww_encoder_train_backward_full(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes,
                                               const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                               const gww_dora_target* targets, int n_targets, float* d_x0,
                                               float* d_mel, int pooled, const gww_enc_grads* grads, void* stream) {
  return train_backward_impl(e, batch, workspace, workspace_bytes, saved, saved_bytes, d_last_hidden, targets, n_targets,
                             d_x0, d_mel, pooled, grads, (hipStream_t)stream);
}
