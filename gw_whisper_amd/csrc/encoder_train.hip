// DoRA / LoRA / full fine-tuning training step (bf16): a forward that keeps the activations the backward needs, and the
// backward through the whole layer stack down to the residual stream entering layer 0 and, on request, the conv stem.
// plan_train makes every choice of path once (TrainPlan: fused or per-op forward, the dX GEMM kernels, the adapter-gradient
// kernels, what is wanted below layer 0, the workspace carve-up, the target table); Step carries the plan and the carved
// buffers; its forward is stem + walk_fused | walk_per_op, its backward ONE layer walk for pooled and dense steps (rows = B
// above the pooled last layer's attention, M elsewhere) + stem_backward.  DESIGN.md section 20.
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

// full fine-tuning: the partial slabs of the weight-gradient GEMMs and of the LayerNorm gain / bias sums (one region,
// reused by every launch in stream order)
size_t train_param_scratch_bytes(const gww_enc_cfg& c, int B) {
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
// fc1 / fc2 targets and ranks other than 8 (the adapter-gradient kernel): its scratch for the largest target shape
size_t train_adapter_scratch_bytes(const gww_enc_cfg& c, int B, int max_r) {
  const long M = (long)B * (c.t_in / 2);
  size_t mx = 0;
  for (int di : {c.d_model, c.ffn})
    for (int dd : {c.d_model, c.ffn}) mx = std::max(mx, adapter_grads_scratch_bytes(M, di, dd, max_r));
  return align_up(mx);
}

// THE carve-up of the workspace: the four gww_train_workspace_bytes* queries and both entry points take it from here.
// Behind the step's own buffers lie the full fine-tuning region (grads) and behind that the adapter-gradient scratch
// (max_r > 0: sized by the query; the backward uses whatever the caller's workspace holds past `ascr`).
struct TrainWs {
  size_t melT, c1, h2, f1, d2, dx, dxb, dbig, dh, dctx, dqkv, Dv, z1, col1, dgs, dgs_bytes, pscr, pscr_bytes, ascr, total;
};
TrainWs train_ws(const gww_enc_cfg& c, int B, bool grads = false, int max_r = 0) {
  const size_t d = c.d_model, F = c.ffn, Tin = c.t_in, T = c.t_in / 2, C = c.n_mels, H = c.n_heads;
  const size_t Kc1 = conv1_kpad(c.n_mels);
  const size_t Mp = padded_rows((size_t)B * T);
  TrainWs w{};
  Arena a;
  w.melT = a.take(((size_t)B * (Tin + 2) * C + Kc1) * 2);
  w.c1 = a.take((((size_t)B * (Tin + 2) + 255) / 256 * 256 + 520) * d * 2);
  w.h2 = a.take(Mp * d * 2);      // per-op path: LN2 output; fused path: out_proj delta (fwd), recomputed LN1 output (bwd)
  w.f1 = a.take(Mp * F * 2);      // gelu(fc1): forward (per-op), backward (recomputed for fc2's weight / adapter gradient); fused bwd: also z
  w.d2 = a.take(Mp * d * 2);      // fused path: the last layer's fc2 delta; backward: LN2(x_mid) where z is in the arena
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
  w.pscr_bytes = grads ? train_param_scratch_bytes(c, B) : 0;
  w.pscr = a.take(w.pscr_bytes);
  w.ascr = a.take(max_r > 0 ? train_adapter_scratch_bytes(c, B, max_r) : 0);
  w.total = a.total();
  return w;
}

// d = 384: the training forward runs on the fused inference kernels (GWW_TRAIN_FUSED=0: the per-op forward of round 1)
bool train_fused(const gww_enc_cfg& c) {
  static const bool off = lab_int("GWW_TRAIN_FUSED", 1) == 0;
  return !off && mlp_fused_supported(c.d_model, c.ffn);
}

// ---- the plan of one training step: EVERY choice, made once.  The forward asks with no targets, grads, d_x0 or d_mel (it
// reads fused / op / fast / q_log2 / ws); the targets have passed check_targets and check_target_range.
struct TrainPlan {
  bool pooled;        // only token T - 1 is used: the last layer runs on the B last-token rows above its attention
  bool fused;         // the forward on the fused inference kernels; it keeps no LN1 / LN2 output and no z: the backward recomputes them
  bool op;            // ... with out_proj in front of the fused block (GWW_GENERIC_PATH bit 7: stand-alone)
  bool fast;          // d = 384 / 512: A-stationary kernel for the K = d GEMMs without a residual, v4 / full-N for the other dX GEMMs
  bool multi_ok;      // a layer's q / k / v adapters in one launch_dora_grads_multi (d = 384 / 512, all of rank 8; GWW_DORA_OLD=1: one by one)
  bool q_log2;        // the bf16 q panels carry log2 units
  float q_ysc;        // the stored q is  q_ysc * (W' x + b): 1 / 8 (head_dim^-0.5), times log2(e) with q_log2
  bool want_conv1, want_conv2, want_stem, want_ln1_0;   // base-parameter gradients below layer 0's q / k / v
  bool below_layer0;  // the gradient continues into LN1 of layer 0: somebody asked for d_x0 / d_mel or one of those
  bool stem_bwd;      // ... and through the conv stem
  TrainWs ws;
  TargetTable tt;
};
TrainPlan plan_train(const gww_enc_cfg& c, int batch, int pooled, const gww_dora_target* targets, int n_targets,
                     const gww_enc_grads* grads, const float* d_x0, const float* d_mel) {
  const int d = c.d_model;
  TrainPlan p{};
  p.pooled = pooled != 0;
  p.fused = train_fused(c);
  p.op = !(generic_path_mask() & GP_OUT_PROJ);
  p.fast = (d == 384 || d == 512) && c.ffn % 128 == 0;
  p.multi_ok = (d == 384 || d == 512) && lab_int("GWW_DORA_OLD", 0) == 0;
  for (int i = 0; i < n_targets; ++i) p.multi_ok = p.multi_ok && (targets[i].proj > 2 || targets[i].r == 8);
  p.q_log2 = attention_log2q_enabled();
  p.q_ysc = p.q_log2 ? 0.125f * 1.44269504088896340736f : 0.125f;
  p.want_conv2 = grads && (grads->conv2_w || grads->conv2_b);
  p.want_conv1 = grads && (grads->conv1_w || grads->conv1_b);
  p.want_stem = p.want_conv1 || p.want_conv2 || (grads && grads->pos);
  p.want_ln1_0 = c.n_layers > 0 && grads && grads->layers && (grads->layers[0].ln1_w || grads->layers[0].ln1_b);
  p.below_layer0 = d_x0 || d_mel || p.want_stem || p.want_ln1_0;
  p.stem_bwd = d_mel || p.want_conv1 || p.want_conv2;
  p.ws = train_ws(c, batch, grads != nullptr);
  p.tt = TargetTable(targets, n_targets, c.n_layers);
  return p;
}

// One forward or backward: the plan, the carved workspace and arena, and the launches its parts share.
struct Step {
  gww_encoder* e;
  TrainPlan p;
  SavedLayout sl;
  hipStream_t s;
  int B, d, F, T, H, L;
  long M;
  char *base, *sv;
  void *melT, *c1, *h2, *f1, *d2, *dxb, *dbig, *dh, *dctx, *dqkv;
  float *dx, *Dv;
  const gww_enc_grads* grads = nullptr;   // backward, full fine-tuning: fp32 gradients of the base parameters
  size_t ascr_bytes = 0;                  // backward: what the caller's workspace holds past ws.ascr

  Step(gww_encoder* e_, TrainPlan&& p_, int batch, void* workspace, const void* saved, void* stream)
      : e(e_), p(std::move(p_)), sl(saved_layout(e_->cfg, batch)), s((hipStream_t)stream), B(batch), d(e_->cfg.d_model),
        F(e_->cfg.ffn), T(e_->cfg.t_in / 2), H(e_->cfg.n_heads), L(e_->cfg.n_layers), M((long)batch * T),
        base((char*)workspace), sv((char*)const_cast<void*>(saved)) {
    const TrainWs& w = p.ws;
    melT = base + w.melT; c1 = base + w.c1; h2 = base + w.h2; f1 = base + w.f1; d2 = base + w.d2; dxb = base + w.dxb;
    dbig = base + w.dbig; dh = base + w.dh; dctx = base + w.dctx; dqkv = base + w.dqkv;
    dx = (float*)(base + w.dx); Dv = (float*)(base + w.Dv);
  }
  float* x_in(int l) const { return sl.x_in_at(sv, l); }
  struct Rec { void *h1, *qkv; float* lse; void* ctx; float* x_mid; void* z; };
  Rec rec(int l) const {
    char* lb = sv + (size_t)l * sl.layer_stride;
    return {lb + sl.h1, lb + sl.qkv, (float*)(lb + sl.lse), lb + sl.ctx, (float*)(lb + sl.x_mid), lb + sl.z};
  }
  // forward
  int stem(const float* mel);
  int walk_fused(float* last_hidden);
  int walk_per_op(float* last_hidden);
  int pooled_tail(int l, float* last_hidden);
  // backward
  int backward(const float* d_last_hidden, float* d_x0, float* d_mel);
  int layer_upper(int l, const LayerW& W, const gww_enc_layer_grads& LG, const Rec& r);
  int scatter_pooled();
  int stem_backward(float* d_mel);
  // ---- base-parameter gradients (full fine-tuning); nothing is launched for a gradient nobody wants
  const gww_enc_layer_grads& LG(int l) const {
    static const gww_enc_layer_grads none{};
    return (grads && grads->layers) ? grads->layers[l] : none;
  }
  int wg(const void* dY, long ldy, const void* X, long ldx, long rows, int N, int K, float alpha, float* dW, float* db, int cin) {
    if (!dW && !db) return GWW_OK;
    return launch_wgrad(dY, ldy, X, ldx, rows, N, K, alpha, dW, db, cin, base + p.ws.pscr, p.ws.pscr_bytes, s);
  }
  int lng(const float* x, const void* dy, int dy_f32, long rows, float* dg, float* db) {
    if (!dg && !db) return GWW_OK;
    return launch_ln_param_grads(x, dy, dy_f32, rows, d, dg, db, base + p.ws.pscr, p.ws.pscr_bytes, s);
  }
  // dX GEMMs.  compact (the B rows of the pooled last layer): the generic kernel.  Dense: A-stationary kernel for the
  // K <= 512 contractions, full-N kernel for the long-K, N = d ones (d = 384 / 512); generic tiles otherwise.  All dense
  // buffers are padded to whole 256-row panels.
  int gemm_dx(const void* A, long lda, const void* Wt, void* Cout, int N, int K, bool compact = false) {
    if (compact) return launch_gemm_bf16(A, lda, Wt, nullptr, nullptr, nullptr, Cout, B, N, K, EPI_BIAS, 0, s, 0);
    // the wide product of the MLP backward (d(fc1 output) = d(out) W2: N = ffn, K = d) on the 256 x 256 x 64 kernel: 113 GFLOP
    // in ~130 us against ~200 on the A-stationary kernel, whose 12 n-tile epilogues per panel run with nothing beside them
    if (p.fast && lda == K && N % 256 == 0 && N >= 1024 && K % 128 == 0) {
      const int rc = launch_gemm_bf16_v4(A, lda, Wt, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, s);
      if (rc != -1) return rc;
    }
    if (p.fast && lda == K && (K == 384 || K == 512) && N % 128 == 0)
      return launch_gemm_astat(A, lda, nullptr, nullptr, nullptr, nullptr, Wt, nullptr, Cout, M, N, K, EPI_BIAS, 0, s);
    if (p.fast && N == d && K % 64 == 0 && K > 512)
      return launch_gemm_fulln(A, lda, Wt, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, 0, s);
    return launch_gemm_bf16(A, lda, Wt, nullptr, nullptr, nullptr, Cout, M, N, K, EPI_BIAS, 0, s, 1);
  }
  // fc1 / fc2 targets and ranks other than 8: the adapter-gradient kernel (dora_grads.hip), its scratch behind the
  // workspace when the caller sized it with gww_train_workspace_bytes_adapters (else allocated stream-ordered)
  int agrad(const gww_dora_target& t, const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias,
            float ysc, long rows, int d_in, int d_out) {
    return launch_adapter_grads(X, ldx, dY, Y, ldy, bias, ysc, t.scaling, t.A, t.B, t.mag, t.nrm, t.dA, t.dB, t.dm, rows,
                                d_in, d_out, t.r, s, ascr_bytes ? base + p.ws.ascr : nullptr, ascr_bytes);
  }
  // q / k / v / out_proj targets (d x d): the rank-8 kernels of launch_dora_grads, the adapter-gradient kernel otherwise
  int dgrad(const gww_dora_target& t, const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias,
            float ysc, long rows) {
    if (t.r != 8) return agrad(t, X, ldx, dY, Y, ldy, bias, ysc, rows, d, d);
    return launch_dora_grads(X, ldx, dY, Y, ldy, bias, ysc, t.scaling, t.A, t.B, t.mag, t.nrm, t.dA, t.dB, t.dm, rows, d,
                             t.r, s, base + p.ws.dgs, p.ws.dgs_bytes);
  }
};

// ---- stem (same kernels as inference) -> x_in[0]
int Step::stem(const float* mel) {
  const int Tin = e->cfg.t_in, C = e->cfg.n_mels, Kc1 = conv1_kpad(C);
  GWW_TRY(launch_mel_to_tokens(mel, melT, 1, B, C, Tin, s));
  GWW_HIP(hipMemsetAsync((char*)melT + (size_t)B * (Tin + 2) * C * 2, 0, Kc1 * 2, s));
  GWW_HIP(hipMemsetAsync(c1, 0, (size_t)d * 2, s));
  if (p.fused) {   // the inference stem kernels (A-stationary conv1, full-N conv2)
    GWW_TRY(launch_gemm_astat(melT, C, nullptr, nullptr, nullptr, nullptr, e->c1w, e->c1b, c1, (long)B * (Tin + 2), d,
                              Kc1, EPI_CONV1, Tin + 2, s));
    return launch_gemm_bf16_v4(c1, 2L * d, e->c2w, e->c2b, nullptr, x_in(0), (long)B * (T + 1), (d + 255) / 256 * 256, 3 * d,
                               EPI_CONV2, s, 0, e->pos, T + 1, d, (float*)h2);   // (h2 is idle here: the scratch row of the garbage rows)
  }
  GWW_TRY(launch_gemm_bf16(melT, C, e->c1w, e->c1b, nullptr, nullptr, c1, (long)B * (Tin + 2), d, Kc1, EPI_CONV1,
                           Tin + 2, s, 0));
  return launch_gemm_bf16(c1, 2L * d, e->c2w, e->c2b, nullptr, e->pos, x_in(0), (long)B * (T + 1), d, 3 * d, EPI_CONV2,
                          T + 1, s, 1);
}

// The last layer of a pooled step above its attention, on both forward paths.  Only token T-1 of the output is used
// (Signal_vs_Noise/src/model.py:25-26), and past the last attention every op is row-wise: out_proj / LN2 / fc1 / GELU /
// fc2 / final LN run on the B last-token rows alone.  x_mid, z and x_in[L] (= x_out) of this layer are saved COMPACT
// ([B, .]) -- the pooled backward expects exactly that.  xl: [B, d] fp32 of scratch for the x_in[L-1] rows (b, T-1) (the
// gradient buffers are idle in the forward); h2 / f1: the workspace's LN2 output and gelu(fc1) buffers.
int Step::pooled_tail(int l, float* last_hidden) {
  const LayerW& W = e->layers[l];
  const Rec r = rec(l);
  float *xl = dx, *x_out = x_in(L);
  GWW_HIP(hipMemcpy2DAsync(xl, (size_t)d * 4, x_in(l) + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                           hipMemcpyDeviceToDevice, s));
  GWW_TRY(launch_gemm_bf16((const unsigned short*)r.ctx + (size_t)(T - 1) * d, (long)T * d, W.wo, W.bo, xl, nullptr,
                           r.x_mid, B, d, d, EPI_RESID, 0, s, 0));
  GWW_TRY(launch_layernorm(r.x_mid, W.ln2w, W.ln2b, h2, 1, B, d, s));
  GWW_TRY(launch_gemm_bf16(h2, d, W.w1, W.b1, nullptr, nullptr, r.z, B, F, d, EPI_BIAS, 0, s, 0));
  GWW_TRY(launch_gelu_bf16(r.z, nullptr, f1, (((long)B * F + 7) / 8) * 8, s));
  GWW_TRY(launch_gemm_bf16(f1, F, W.w2, W.b2, r.x_mid, nullptr, x_out, B, d, F, EPI_RESID, 0, s, 0));
  return launch_layernorm(x_out, e->lnw, e->lnb, last_hidden, 0, B, d, s);
}

// ---- fused forward (d = 384): the INFERENCE kernels -- LayerNorm-folded A-stationary q/k/v GEMM for layer 0, flash
// attention (+ lse), out_proj as a bf16 delta, fused MLP + the next layer's LN1 + q/k/v -- writing what the
// backward needs straight into the arena: x_in[l], qkv, lse, ctx, x_mid (= x_in + out_proj, the fused kernel's
// x_new).  LN1 / LN2 outputs and the pre-GELU fc1 output are NOT kept: the backward recomputes them (that is what
// the reference's gradient_checkpointing_enable() at MLGWSC-1/train.py:662 trades, too).
int Step::walk_fused(float* last_hidden) {
  void* d1 = h2;
  for (int l = 0; l < L; ++l) {
    const LayerW& W = e->layers[l];
    const Rec r = rec(l);
    if (l == 0) {
      // layer 0: LN1 + q / k / v on the fused block's panel prologue + tail (k_mlp_fused<2, false>), as the inference
      // forward does (round 3 ran the LayerNorm kernel + the plain A-stationary GEMM here: 41 + 112 us at 64 segments)
      MlpFusedArgs a;
      a.who = "gww_encoder_train_forward"; a.x = x_in(0); a.Wt = W.wqkv_st; a.M = M; a.d = d;
      a.qkv_u = W.uqkv; a.qkv_cb = W.cbqkv; a.qkv_out = r.qkv; a.NQ = 3 * d;
      GWW_TRY(launch_mlp_fused(a, s));
    }
    if (p.pooled && l == L - 1) {
      // only the query tile that holds token T - 1 is needed (forward and backward): the other rows of ctx / lse stay
      // zero so that the backward's row dots see finite values
      GWW_HIP(hipMemsetAsync(r.ctx, 0, (size_t)M * d * 2, s));
      GWW_HIP(hipMemsetAsync(r.lse, 0, (size_t)B * H * T * 4, s));
      GWW_TRY(launch_attention_bf16(r.qkv, r.ctx, B, T, H, s, r.lse, /*last_tile_only=*/true, p.q_log2));
      return pooled_tail(l, last_hidden);
    }
    GWW_TRY(launch_attention_bf16(r.qkv, r.ctx, B, T, H, s, r.lse, false, p.q_log2));
    // out_proj fused in front of the block as on the inference path: x_mid = x_in + bf16(ctx W_o^T + bo) comes out of
    // the kernel's seam and is kept (the backward needs ctx and x_mid, never the delta)
    MlpFusedArgs a;
    a.who = "gww_encoder_train_forward"; a.x = x_in(l); a.x_new = r.x_mid; a.keep_x_new = true;
    a.ln_u = W.u1; a.ln_cb = W.cb1; a.b2 = W.b2; a.M = M; a.d = d; a.F = F;
    if (p.op) {
      a.ctx = r.ctx; a.bo = W.bo; a.Wt = W.wmlp_op;
    } else {
      GWW_TRY(launch_gemm_astat(r.ctx, d, nullptr, nullptr, nullptr, nullptr, W.wo, W.bo, d1, M, d, d, EPI_BIAS, 0, s));
      a.delta = d1; a.Wt = W.wmlp;
    }
    if (l + 1 < L) {   // the next layer's LN1 + q / k / v behind the block, x_next straight into the arena
      const LayerW& Wn = e->layers[l + 1];
      a.qkv_u = Wn.uqkv; a.qkv_cb = Wn.cbqkv; a.qkv_out = rec(l + 1).qkv; a.NQ = 3 * d;
      a.x_next = x_in(l + 1);
      GWW_TRY(launch_mlp_fused(a, s));
    } else {
      a.C = d2;
      GWW_TRY(launch_mlp_fused(a, s));
      GWW_TRY(launch_add_delta_f32(r.x_mid, d2, x_in(L), M * d, s));
    }
  }
  return launch_layernorm(x_in(L), e->lnw, e->lnb, last_hidden, 0, M, d, s);
}

// ---- per-op forward: LayerNorm kernel, GEMM with bias / residual epilogue; LN1 output and z are kept
int Step::walk_per_op(float* last_hidden) {
  for (int l = 0; l < L; ++l) {
    const LayerW& W = e->layers[l];
    const Rec r = rec(l);
    GWW_TRY(launch_layernorm(x_in(l), W.ln1w, W.ln1b, r.h1, 1, M, d, s));
    if (p.fast) GWW_TRY(launch_gemm_astat(r.h1, d, nullptr, nullptr, nullptr, nullptr, W.wqkv, W.bqkv16, r.qkv, M, 3 * d, d, EPI_BIAS, 0, s));
    else GWW_TRY(launch_gemm_bf16(r.h1, d, W.wqkv, W.bqkv16, nullptr, nullptr, r.qkv, M, 3 * d, d, EPI_BIAS, 0, s, 1));
    GWW_TRY(launch_attention_bf16(r.qkv, r.ctx, B, T, H, s, r.lse, false, p.q_log2));
    if (p.pooled && l == L - 1) return pooled_tail(l, last_hidden);
    GWW_TRY(launch_gemm_bf16(r.ctx, d, W.wo, W.bo, x_in(l), nullptr, r.x_mid, M, d, d, EPI_RESID, 0, s, 1));
    GWW_TRY(launch_layernorm(r.x_mid, W.ln2w, W.ln2b, h2, 1, M, d, s));
    if (p.fast) GWW_TRY(launch_gemm_astat(h2, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, r.z, M, F, d, EPI_BIAS, 0, s));
    else GWW_TRY(launch_gemm_bf16(h2, d, W.w1, W.b1, nullptr, nullptr, r.z, M, F, d, EPI_BIAS, 0, s, 1));
    GWW_TRY(launch_gelu_bf16(r.z, nullptr, f1, ((M * F + 7) / 8) * 8, s));
    GWW_TRY(launch_gemm_bf16(f1, F, W.w2, W.b2, r.x_mid, nullptr, x_in(l + 1), M, d, F, EPI_RESID, 0, s, 1));
  }
  return launch_layernorm(x_in(L), e->lnw, e->lnb, last_hidden, 0, M, d, s);
}

// ---- backward of one layer above its attention: fc2 / GELU / fc1 / LN2 / out_proj, dxb = d(x_out) in, dctx out.
//   x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))      x_mid = x_in + out_proj(ctx)
// The last layer of a pooled step lives on the B last-token rows (x_mid, z, x_in[L] were saved compact by the pooled
// forward); the attention backward then sees a dctx that is zero except for row T-1 of every segment and skips the dead
// query tiles.  Weight gradients (wgrad.hip) pair a gradient and an activation this walk has in hand:
//   fc2: d(x_out) x gelu(z)    fc1: d(z) x LN2(x_mid)    out_proj: d(x_mid) x ctx
int Step::layer_upper(int l, const LayerW& W, const gww_enc_layer_grads& LG, const Rec& r) {
  const bool last_pooled = p.pooled && l == L - 1;
  const long rows = last_pooled ? B : M, nz = ((rows * F + 7) / 8) * 8;
  const bool z_saved = !p.fused || last_pooled;   // else z is recomputed: fc1 of LN2(x_mid) on the A-stationary kernel
  void* ln2_buf = z_saved ? d2 : dctx;            // LN2(x_mid), in a buffer that is idle here
  const void* ln2_out = nullptr;                  // ... once somebody has needed it
  auto ln2 = [&]() -> int {
    if (!ln2_out) GWW_TRY(launch_layernorm(r.x_mid, W.ln2w, W.ln2b, ln2_buf, 1, rows, d, s));
    ln2_out = ln2_buf;
    return GWW_OK;
  };
  const bool want_fc2 = LG.fc2_w || LG.fc2_b, want_fc1 = LG.fc1_w || LG.fc1_b;
  const gww_dora_target *fc1t = p.tt.at(l, 4), *fc2t = p.tt.at(l, 5);
  GWW_TRY(gemm_dx(dxb, d, W.w2T, dbig, F, d, last_pooled));
  if (fc1t || fc2t) {
    // fc1 / fc2 adapters.  fc1: x = LN2(x_mid), dy = d(pre-activation), y = z (+ b1);  fc2: x = gelu(z),
    // dy = d(x_out) (dxb), y = x_out - x_mid (+ b2).  A z that is not in the arena is recomputed into f1 with the plain
    // bias epilogue, and the GELU backward reads it from there.
    const void* zz = r.z;
    if (!z_saved) {
      GWW_TRY(ln2());
      GWW_TRY(launch_gemm_astat(ln2_out, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, f1, M, F, d, EPI_BIAS, 0, s));
      zz = f1;
    } else if (fc1t) {
      GWW_TRY(ln2());
    }
    GWW_TRY(launch_gelu_bf16(zz, dbig, dbig, nz, s));
    if (fc1t) GWW_TRY(agrad(*fc1t, ln2_out, d, dbig, zz, F, W.b1, 1.0f, rows, d, F));
    if (fc2t || want_fc2) GWW_TRY(launch_gelu_bf16(zz, nullptr, f1, nz, s));   // in place when recomputed
    if (fc2t) {
      GWW_TRY(launch_sub_f32_bf16(x_in(l + 1), r.x_mid, dh, rows * d, s));
      GWW_TRY(agrad(*fc2t, f1, F, dxb, dh, d, W.b2, 1.0f, rows, F, d));
    }
  } else if (!z_saved) {
    // fc1 as a plain A-stationary GEMM whose epilogue applies gelu'(pre-activation) to the gradient in place: neither
    // the pre-activation nor a separate GELU-backward pass touches HBM; full fine-tuning: the same GEMM with the GELU
    // epilogue first, for the fc2 weight gradient's X operand
    GWW_TRY(ln2());
    if (want_fc2)
      GWW_TRY(launch_gemm_astat(ln2_out, d, nullptr, nullptr, nullptr, nullptr, W.w1, W.b1, f1, M, F, d, EPI_GELU, 0, s));
    GWW_TRY(launch_gemm_astat(ln2_out, d, dbig, nullptr, nullptr, nullptr, W.w1, W.b1, dbig, M, F, d, EPI_DGELU, 0, s));
  } else {
    if (want_fc2) GWW_TRY(launch_gelu_bf16(r.z, nullptr, f1, nz, s));
    GWW_TRY(launch_gelu_bf16(r.z, dbig, dbig, nz, s));
  }
  GWW_TRY(wg(dxb, d, f1, F, rows, d, F, 1.0f, LG.fc2_w, LG.fc2_b, 0));
  if (want_fc1) {
    GWW_TRY(ln2());
    GWW_TRY(wg(dbig, F, ln2_out, d, rows, F, d, 1.0f, LG.fc1_w, LG.fc1_b, 0));
  }
  GWW_TRY(gemm_dx(dbig, F, W.w1T, dh, d, F, last_pooled));
  GWW_TRY(lng(r.x_mid, dh, 0, rows, LG.ln2_w, LG.ln2_b));
  GWW_TRY(launch_ln_bwd(r.x_mid, W.ln2w, dh, 0, dx, 1, dxb, rows, d, s));
  // out_proj: x = ctx (pooled: its rows (b, T-1)), dy = d(x_mid) (= dxb), y = x_mid - x_in (rebuilt into dh, free here)
  const unsigned short* ctx_x = (const unsigned short*)r.ctx + (last_pooled ? (size_t)(T - 1) * d : 0);
  const long ldc = last_pooled ? (long)T * d : d;
  if (const gww_dora_target* t = p.tt.at(l, 3)) {
    const float* xl = x_in(l);
    if (last_pooled) {   // the x_in rows (b, T-1), compact, into the idle dbig
      GWW_HIP(hipMemcpy2DAsync(dbig, (size_t)d * 4, xl + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                               hipMemcpyDeviceToDevice, s));
      xl = (const float*)dbig;
    }
    GWW_TRY(launch_sub_f32_bf16(r.x_mid, xl, dh, rows * d, s));
    GWW_TRY(dgrad(*t, ctx_x, ldc, dxb, dh, d, W.bo, 1.0f, rows));
  }
  GWW_TRY(wg(dxb, d, ctx_x, ldc, rows, d, d, 1.0f, LG.o_w, LG.o_b, 0));
  GWW_TRY(gemm_dx(dxb, d, W.woT, last_pooled ? dh : dctx, d, d, last_pooled));
  return last_pooled ? scatter_pooled() : GWW_OK;
}

// The pooled last layer hands over to the dense walk: d(ctx) rows (b, T-1) (compact in dh) -> the dense, otherwise zero
// dctx; the residual gradient likewise: compact dx -> row T-1 of a zero dense dx
int Step::scatter_pooled() {
  GWW_HIP(hipMemsetAsync(dctx, 0, (size_t)M * d * 2, s));
  GWW_HIP(hipMemcpy2DAsync((unsigned short*)dctx + (size_t)(T - 1) * d, (size_t)T * d * 2, dh, (size_t)d * 2,
                           (size_t)d * 2, B, hipMemcpyDeviceToDevice, s));
  GWW_HIP(hipMemcpyAsync(dbig, dx, (size_t)B * d * 4, hipMemcpyDeviceToDevice, s));
  GWW_HIP(hipMemsetAsync(dx, 0, (size_t)M * d * 4, s));
  GWW_HIP(hipMemcpy2DAsync(dx + (size_t)(T - 1) * d, (size_t)T * d * 4, dbig, (size_t)d * 4, (size_t)d * 4, B,
                           hipMemcpyDeviceToDevice, s));
  return GWW_OK;
}

// ---- conv stem backward: x0 = gelu(conv2(gelu(conv1(mel)))) + pos, dxb = d(x0) in (melT and c1 of the forward are still
// in the workspace); the pre-activations are recomputed by the same GEMMs with a plain bias epilogue
int Step::stem_backward(float* d_mel) {
  const int Tin = e->cfg.t_in, C = e->cfg.n_mels, Kc1 = conv1_kpad(C);
  GWW_REQUIRE(B <= 512, "gww_encoder_train_backward: d_mel and the conv-stem gradients support batch <= 512");
  void* z1 = base + p.ws.z1;
  void* col1 = base + p.ws.col1;
  const long M2 = (long)B * (T + 1), M1 = (long)B * (Tin + 2);
  GWW_TRY(launch_gemm_bf16(c1, 2L * d, e->c2w, e->c2b, nullptr, nullptr, dh, M2, d, 3 * d, EPI_BIAS, 0, s, 0));       // z2
  GWW_TRY(launch_stem_dz2(dxb, dh, dctx, B, T, d, s));                                                              // dz2
  // conv2 weight gradient on the forward's im2col view of c1 (row m: padded rows 2 t .. 2 t + 2); the junk row
  // t = T of every segment has dz2 = 0
  if (p.want_conv2) GWW_TRY(wg(dctx, d, c1, 2L * d, M2, d, 3 * d, 1.0f, grads->conv2_w, grads->conv2_b, d));
  if (d_mel || p.want_conv1) {
    GWW_TRY(launch_gemm_bf16(dctx, d, e->c2wT, nullptr, nullptr, nullptr, dqkv, M2, 3 * d, d, EPI_BIAS, 0, s, 0));   // col
    GWW_TRY(launch_gemm_bf16(melT, C, e->c1w, e->c1b, nullptr, nullptr, z1, M1, d, Kc1, EPI_BIAS, 0, s, 0));  // z1
    GWW_TRY(launch_stem_dz1(dqkv, z1, z1, B, T, Tin, d, s));                                                        // dz1
    // conv1 weight gradient on the im2col view of melT (K = Kc1: taps 0..2 of C channels + padding, dropped)
    if (p.want_conv1) GWW_TRY(wg(z1, d, melT, C, M1, d, Kc1, 1.0f, grads->conv1_w, grads->conv1_b, C));
  }
  if (d_mel) {
    GWW_TRY(launch_gemm_bf16(z1, d, e->c1wT, nullptr, nullptr, nullptr, col1, M1, Kc1, d, EPI_BIAS, 0, s, 0));  // col1
    GWW_TRY(launch_stem_dmel(col1, d_mel, B, Tin, C, Kc1, s));
  }
  return GWW_OK;
}

int Step::backward(const float* d_last_hidden, float* d_x0, float* d_mel) {
  // final LayerNorm backward -> dx (grad w.r.t. x_in[L]); pooled: on the B last-token rows only
  const long rows_L = p.pooled ? B : M;
  if (grads) GWW_TRY(lng(x_in(L), d_last_hidden, 1, rows_L, grads->ln_w, grads->ln_b));
  GWW_TRY(launch_ln_bwd(x_in(L), e->lnw, d_last_hidden, 1, dx, 0, dxb, rows_L, d, s));
  for (int l = L - 1; l >= 0; --l) {
    const LayerW& W = e->layers[l];
    const gww_enc_layer_grads& G = LG(l);
    Rec r = rec(l);
    if (p.fused) {   // the fused forward kept no LN1(x_in), the X operand of the q / k / v gradients: recomputed here
      GWW_TRY(launch_layernorm(x_in(l), W.ln1w, W.ln1b, h2, 1, M, d, s));
      r.h1 = h2;
    }
    GWW_TRY(layer_upper(l, W, G, r));
    // attention / QKV / LN1   (x_mid = x_in + out_proj(attn(qkv(LN1(x_in)))))
    GWW_TRY(launch_attention_bwd_bf16(r.qkv, r.ctx, dctx, r.lse, Dv, dqkv, B, T, H, s, p.q_log2));
    // q / k / v adapters: x = h1, dy / y = the q | k | v sections of dqkv / qkv
    long off[3];
    const float *bias[3], *Aa[3], *Bb[3], *mg[3], *nr[3];
    float ysc[3], scl[3], *dAa[3], *dBb[3], *dmm[3];
    int np = 0;
    for (int pr = 0; pr < 3; ++pr) {
      const gww_dora_target* t = p.tt.at(l, pr);
      if (!t) continue;
      off[np] = (long)pr * d;
      bias[np] = W.bqkv16 + off[np];
      ysc[np] = pr == 0 ? p.q_ysc : 1.0f;
      if (!p.multi_ok) {
        GWW_TRY(dgrad(*t, r.h1, d, (const unsigned short*)dqkv + off[np], (const unsigned short*)r.qkv + off[np], 3L * d,
                      bias[np], ysc[np], M));
        continue;
      }
      scl[np] = t->scaling;
      Aa[np] = t->A; Bb[np] = t->B; mg[np] = t->mag; nr[np] = t->nrm;
      dAa[np] = t->dA; dBb[np] = t->dB; dmm[np] = t->dm;
      ++np;
    }
    if (np > 0)   // (multi_ok) they read the same h1: one pass over h1, dqkv and qkv on the matrix cores
      GWW_TRY(launch_dora_grads_multi(r.h1, d, dqkv, r.qkv, 3L * d, np, off, bias, ysc, scl, Aa, Bb, mg, nr, dAa, dBb, dmm, M,
                                      d, s, base + p.ws.dgs, p.ws.dgs_bytes));
    // q / k / v weight gradients: dqkv is the gradient of the STORED q (q_ysc (W x + b)), k has no bias
    GWW_TRY(wg(dqkv, 3L * d, r.h1, d, M, d, d, p.q_ysc, G.q_w, G.q_b, 0));
    GWW_TRY(wg((const unsigned short*)dqkv + d, 3L * d, r.h1, d, M, d, d, 1.0f, G.k_w, nullptr, 0));
    GWW_TRY(wg((const unsigned short*)dqkv + 2 * d, 3L * d, r.h1, d, M, d, d, 1.0f, G.v_w, G.v_b, 0));
    // below layer 0 the gradient only continues into LN1 of layer 0 and the conv stem
    if (l == 0 && !p.below_layer0) break;
    GWW_TRY(gemm_dx(dqkv, 3L * d, W.wqkvT, dh, d, 3 * d));
    GWW_TRY(lng(x_in(l), dh, 0, M, G.ln1_w, G.ln1_b));
    GWW_TRY(launch_ln_bwd(x_in(l), W.ln1w, dh, 0, dx, 1, dxb, M, d, s));
  }
  if (d_x0) GWW_HIP(hipMemcpyAsync(d_x0, dx, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
  if (grads && grads->pos) GWW_TRY(launch_pos_grad(dx, grads->pos, B, T, d, s));   // x0 = gelu(conv2) + pos
  return p.stem_bwd ? stem_backward(d_mel) : GWW_OK;
}
}  // namespace

extern "C" size_t gww_train_saved_bytes(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? saved_layout(e->cfg, batch).total : 0;
}
extern "C" size_t gww_train_workspace_bytes(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? train_ws(e->cfg, batch).total : 0;
}
extern "C" size_t gww_train_workspace_bytes_full(const gww_encoder* e, int batch) {
  return (e && batch > 0) ? train_ws(e->cfg, batch, true).total : 0;
}
extern "C" size_t gww_train_workspace_bytes_adapters(const gww_encoder* e, int batch, int max_r) {
  return (e && batch > 0 && max_r >= 1 && max_r <= 64) ? train_ws(e->cfg, batch, false, max_r).total : 0;
}

extern "C" int gww_encoder_train_forward(gww_encoder* e, const float* mel, int batch, void* workspace,
                                         size_t workspace_bytes, void* saved, size_t saved_bytes,
                                         float* last_hidden, int pooled, void* stream) {
  GWW_REQUIRE(e && mel && workspace && saved && last_hidden, "gww_encoder_train_forward: NULL argument");
  if (!e->ready) return fail(GWW_ERR_STATE, "gww_encoder_train_forward: weights not set");
  GWW_REQUIRE(batch > 0, "gww_encoder_train_forward: batch must be positive");
  Step st(e, plan_train(e->cfg, batch, pooled, nullptr, 0, nullptr, nullptr, nullptr), batch, workspace, saved, stream);
  if (workspace_bytes < st.p.ws.total || saved_bytes < st.sl.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_train_forward: workspace %zu / saved %zu bytes < required %zu / %zu",
                workspace_bytes, saved_bytes, st.p.ws.total, st.sl.total);
  GWW_TRY(st.stem(mel));
  return st.p.fused ? st.walk_fused(last_hidden) : st.walk_per_op(last_hidden);
}

// d_last_hidden: fp32 [B*T, d] gradient of the loss w.r.t. last_hidden_state.
// targets: DoRA-adapted projections whose A / B / magnitude gradients are wanted, at most one per (layer, proj); the
// gradient buffers are ACCUMULATED into (zero them once per step).  d_x0 (optional, fp32 [B*T, d]): gradient w.r.t. the
// residual stream entering layer 0 (the conv stem output).  d_mel (optional, fp32 [B, n_mels, t_in]): gradient
// w.r.t. the input features, through the conv stem (MLGWSC-1/train.py:494-504 trains its Q-adapter through
// the frozen encoder).  grads (full fine-tuning, may be NULL): fp32 gradients of the base parameters, accumulated into:
// weight-gradient GEMMs of pairs the walk has in hand, fixed-order column sums for LayerNorm gains / biases and positions.
static int train_backward_impl(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes, const void* saved,
                               size_t saved_bytes, const float* d_last_hidden, const gww_dora_target* targets,
                               int n_targets, float* d_x0, float* d_mel, int pooled, const gww_enc_grads* grads,
                               void* stream) {
  const char* who = "gww_encoder_train_backward";
  GWW_REQUIRE(e && workspace && saved && d_last_hidden, "%s: NULL argument", who);
  GWW_REQUIRE(batch > 0 && n_targets >= 0 && (n_targets == 0 || targets), "%s: bad argument", who);
  GWW_TRY(check_targets(who, targets, n_targets));   // (nothing of the handle is read for them)
  GWW_TRY(check_target_range(who, targets, n_targets, e->cfg.n_layers));
  Step st(e, plan_train(e->cfg, batch, pooled, targets, n_targets, grads, d_x0, d_mel), batch, workspace, saved, stream);
  if (workspace_bytes < st.p.ws.total || saved_bytes < st.sl.total)
    return fail(GWW_ERR_WORKSPACE, "%s%s: workspace %zu / saved %zu bytes < required %zu%s / %zu", who, grads ? "_full" : "",
                workspace_bytes, saved_bytes, st.p.ws.total, grads ? " (with base gradients)" : "", st.sl.total);
  st.grads = grads;
  st.ascr_bytes = workspace_bytes > st.p.ws.ascr ? workspace_bytes - st.p.ws.ascr : 0;
  return st.backward(d_last_hidden, d_x0, d_mel);
}

extern "C" int gww_encoder_train_backward(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes,
                                          const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                          const gww_dora_target* targets, int n_targets, float* d_x0,
                                          float* d_mel, int pooled, void* stream) {
  return train_backward_impl(e, batch, workspace, workspace_bytes, saved, saved_bytes, d_last_hidden, targets, n_targets,
                             d_x0, d_mel, pooled, nullptr, stream);
}

extern "C" int gww_encoder_train_backward_full(gww_encoder* e, int batch, void* workspace, size_t workspace_bytes,
                                               const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                               const gww_dora_target* targets, int n_targets, float* d_x0,
                                               float* d_mel, int pooled, const gww_enc_grads* grads, void* stream) {
  return train_backward_impl(e, batch, workspace, workspace_bytes, saved, saved_bytes, d_last_hidden, targets, n_targets,
                             d_x0, d_mel, pooled, grads, stream);
}
