// Encoder handle: weight packing + the forward launch sequence (host side of the
// C ABI).  Replaces WhisperEncoder.forward (HF:modeling_whisper.py:592-646):
//   conv1+GELU -> conv2(stride 2)+GELU + pos -> L x [LN, QKV, MHSA, out_proj+res,
//   LN, fc1+GELU, fc2+res] -> final LN.
//
// HBM layout of one forward (batch B, T_in = 3000 frames, T = 1500 tokens):
//   melT  [B, T_in+2, 80]   token-major mel, zero rows = Conv1d padding   (+tail pad)
//   c1    [B, T_in+2, d]    conv1 output, token-major, zero rows = padding (+1 row)
//   x     [B*T, d]   fp32   residual stream (never leaves fp32)
//   h     [B*T, d]          LayerNorm output (GEMM A operand)
//   qkv   [B*T, 3d]         q | k | v, q pre-scaled by 1/8
//   ctx   [B*T, d]          attention context
//   f1    [B*T, ffn]        fc1 + GELU
// In GWW_PREC_BF16 the activation tensors other than x are bf16; in GWW_PREC_F32
// everything is fp32.  All of it lives in the caller's workspace; the handle owns
// only the packed weights.
#include "encoder_impl.h"

namespace gww {
#ifdef GWW_LAB
long lab_int(const char* name, long dflt) {   // the laboratory build's only environment reader (common.h)
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}
#endif
}

using namespace gww;

// The packed weights, one allocation: THE list of its buffers, in blob order.  Run against a null base it only sizes the
// blob (the pointers it leaves are offsets); run against the blob it places them.
static size_t carve_blob(gww_encoder* e, char* blob) {
  const size_t d = e->cfg.d_model, F = e->cfg.ffn, T = e->cfg.t_in / 2, Kc1 = conv1_kpad(e->cfg.n_mels);
  const uintptr_t base = (uintptr_t)blob;
  Arena a;
  auto put = [&](auto*& p, size_t bytes) { p = (decltype(+p))(base + a.take(bytes)); };
  put(e->c1w, d * Kc1 * 2);
  put(e->c2w, (d + 255) / 256 * 256 * 3 * d * 2);   // rows d .. : zero padding (k_gemm_bf16_v4 takes N % 256 == 0)
  put(e->c1w32, d * Kc1 * 4);
  put(e->c2w32, d * 3 * d * 4);
  put(e->c1wT, d * Kc1 * 2);
  put(e->c2wT, d * 3 * d * 2);
  put(e->c1b, d * 4);
  put(e->c2b, d * 4);
  put(e->pos, T * d * 4);
  put(e->lnw, d * 4);
  put(e->lnb, d * 4);
  put(e->pos_c, kStemTt * d * 4);
  for (LayerW& w : e->layers) {
    put(w.wqkv, 3 * d * d * 2);
    put(w.wo, d * d * 2);
    put(w.w1, F * d * 2);
    put(w.w2, d * F * 2);
    put(w.wqkv32, 3 * d * d * 4);
    put(w.wo32, d * d * 4);
    put(w.w132, F * d * 4);
    put(w.w232, d * F * 4);
    put(w.bqkv, 3 * d * 4);
    put(w.bqkv16, 3 * d * 4);
    put(w.bo, d * 4);
    put(w.b1, F * 4);
    put(w.b2, d * 4);
    put(w.ln1w, d * 4);
    put(w.ln1b, d * 4);
    put(w.ln2w, d * 4);
    put(w.ln2b, d * 4);
    put(w.wqkv_ln, 3 * d * d * 2);
    put(w.w1_ln, F * d * 2);
    put(w.wmlp, (2 * F * d + 3 * d * d) * 2);                       // fc1' + fc2 (+ the next layer's q / k / v panel)
    put(w.wqkv_st, &w == &e->layers[0] ? 3 * d * d * 2 : 16);       // layer 0's own panel as a stream
    put(w.wmlp_op, (d * d + 2 * F * d + 3 * d * d) * 2);            // W_o + the stream above
    put(w.uqkv, 3 * d * 4);
    put(w.cbqkv, 3 * d * 4);
    put(w.u1, F * 4);
    put(w.cb1, F * 4);
    put(w.wqkvT, 3 * d * d * 2);
    put(w.woT, d * d * 2);
    put(w.w1T, F * d * 2);
    put(w.w2T, d * F * 2);
  }
  return a.total();
}

extern "C" int gww_encoder_create(const gww_enc_cfg* cfg, gww_encoder** out) {
  GWW_REQUIRE(cfg && out, "gww_encoder_create: NULL argument");
  const int d = cfg->d_model, L = cfg->n_layers, H = cfg->n_heads, F = cfg->ffn, C = cfg->n_mels;
  GWW_REQUIRE(d > 0 && d % 128 == 0 && d <= 1280, "gww_encoder_create: d_model=%d must be a multiple of 128 <= 1280", d);
  GWW_REQUIRE(H * 64 == d, "gww_encoder_create: n_heads=%d * 64 != d_model=%d (Whisper head_dim is 64)", H, d);
  GWW_REQUIRE(L > 0 && F > 0 && F % 64 == 0, "gww_encoder_create: bad n_layers=%d / ffn=%d", L, F);
  GWW_REQUIRE(C == 80 || C == 128, "gww_encoder_create: n_mels=%d (80, or 128 for large-v3)", C);
  GWW_REQUIRE(cfg->t_in > 0 && cfg->t_in % 2 == 0, "gww_encoder_create: t_in=%d must be even", cfg->t_in);

  gww_encoder* e = new gww_encoder();
  e->cfg = *cfg;
  e->layers.resize(L);
  const size_t bytes = carve_blob(e, nullptr);
  hipError_t err = hipMalloc(&e->blob, bytes);
  if (err != hipSuccess) {
    delete e;
    return fail(GWW_ERR_HIP, "hipMalloc(%zu bytes of packed weights) failed: %s", bytes, hipGetErrorString(err));
  }
  e->blob_bytes = carve_blob(e, e->blob);
  *out = e;
  return GWW_OK;
}

extern "C" int gww_encoder_trace_enable(gww_encoder* e, int on) {
  GWW_REQUIRE(e != nullptr, "gww_encoder_trace_enable: NULL handle");
  e->trace = on != 0;
  return GWW_OK;
}

// Sum the elapsed time (ms) and the launch count per kernel class since the last read; blocks until
// the recorded events have completed.  ms / counts: arrays of gww_encoder_trace_classes() entries.
extern "C" int gww_encoder_trace_read(gww_encoder* e, float* ms, int* counts) {
  GWW_REQUIRE(e && ms && counts, "gww_encoder_trace_read: NULL argument");
  for (int i = 0; i < TR_COUNT; ++i) { ms[i] = 0.f; counts[i] = 0; }
  for (TraceSpan& sp : e->spans) {
    GWW_HIP(hipEventSynchronize(sp.b));
    float t = 0.f;
    GWW_HIP(hipEventElapsedTime(&t, sp.a, sp.b));
    ms[sp.cls] += t;
    counts[sp.cls] += 1;
    e->pool.push_back(sp.a);
    e->pool.push_back(sp.b);
  }
  e->spans.clear();
  return GWW_OK;
}

extern "C" int gww_encoder_trace_classes(void) { return TR_COUNT; }
extern "C" const char* gww_encoder_trace_class_name(int i) {
  static const char* names[TR_COUNT] = {"mel_to_tokens", "conv1_gelu", "conv2_gelu_pos", "ln+qkv_proj", "attention",
                                        "out_proj", "ln+fc1_gelu", "fc2", "final_layernorm", "mlp_fused(ln+fc1+gelu+fc2)",
                                        "mlp_fused+next_ln_qkv", "layernorm_rows(B pooled rows)", "mlp_fused+final_layernorm"};
  return (i >= 0 && i < TR_COUNT) ? names[i] : "?";
}

extern "C" void gww_encoder_destroy(gww_encoder* e) {
  if (!e) return;
  for (TraceSpan& sp : e->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
  for (hipEvent_t ev : e->pool) (void)hipEventDestroy(ev);
  for (int i = 0; i < 2; ++i) {
    if (e->s2[i]) (void)hipStreamDestroy(e->s2[i]);
    if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]);
  }
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->blob) (void)hipFree(e->blob);
  delete e;
}

// Weight groups of one layer (bit mask of gww_encoder_update_weights): what has to be re-packed when a
// parameter of the group changed.
//   1 = q / k / v projections + their biases + self_attn_layer_norm   (QKV panels, LN-folded panel, transposes)
//   2 = out_proj          4 = fc1 + final_layer_norm          8 = fc2
static int pack_weights(gww_encoder* e, const gww_enc_globals* g, const gww_enc_layer* layers, int n_layers,
                        const unsigned* dirty, hipStream_t s) {
  const int d = e->cfg.d_model, F = e->cfg.ffn, C = e->cfg.n_mels, T = e->cfg.t_in / 2, Kc1 = conv1_kpad(C);
  const float qs = 0.125f;   // head_dim^-0.5 = 64^-0.5, exact power of two (HF:modeling_whisper.py:309)
  // Two dependency phases, one k_prep_batch launch each (per 40 ops): `pb` reads only the caller's fp32 tensors, `pt` (the
  // transposes for the backward's dX GEMMs) reads panels `pb` wrote.  A DoRA step on whisper-tiny used to enqueue ~75 launches
  // of 3 - 6 us here.
  PrepBatch pb(s), pt(s);
  auto pack = [&](const float* w, unsigned short* o16, float* o32, int N, int Cin, int taps, int Kpad,
                  float scale) -> int {
    GWW_TRY(pb.pack(w, o16, 1, N, Cin, taps, Kpad, scale));
    GWW_TRY(pb.pack(w, o32, 0, N, Cin, taps, Kpad, scale));
    return GWW_OK;
  };
  if (g) {
    GWW_REQUIRE(g->conv1_w && g->conv1_b && g->conv2_w && g->conv2_b && g->pos && g->ln_w && g->ln_b,
                "gww_encoder_set_weights: NULL global weight");
    GWW_TRY(pack(g->conv1_w, e->c1w, e->c1w32, d, C, 3, Kc1, 1.f));
    GWW_TRY(pack(g->conv2_w, e->c2w, e->c2w32, d, d, 3, 3 * d, 1.f));
    if (d % 256 != 0) GWW_HIP(hipMemsetAsync(e->c2w + (size_t)d * 3 * d, 0, (size_t)((d + 255) / 256 * 256 - d) * 3 * d * 2, s));
    GWW_TRY(pt.transpose(e->c1w, e->c1wT, d, Kc1));
    GWW_TRY(pt.transpose(e->c2w, e->c2wT, d, 3 * d));
    GWW_TRY(pb.copy(g->conv1_b, e->c1b, d, 1.f));
    GWW_TRY(pb.copy(g->conv2_b, e->c2b, d, 1.f));
    GWW_HIP(hipMemcpyAsync(e->pos, g->pos, (size_t)T * d * 4, hipMemcpyDeviceToDevice, s));
    if (T > kStemTt) {
      // the compact stem's table (stem_tail.hip): compact tokens 0 .. Tt - 3 are the real ones, Tt - 2 is the position-free
      // shared row (its store bypasses the table), Tt - 1 is the real token T - 1
      GWW_HIP(hipMemcpyAsync(e->pos_c, g->pos, (size_t)(kStemTt - 2) * d * 4, hipMemcpyDeviceToDevice, s));
      GWW_HIP(hipMemsetAsync(e->pos_c + (size_t)(kStemTt - 2) * d, 0, (size_t)d * 4, s));
      GWW_HIP(hipMemcpyAsync(e->pos_c + (size_t)(kStemTt - 1) * d, g->pos + (size_t)(T - 1) * d, (size_t)d * 4,
                             hipMemcpyDeviceToDevice, s));
    }
    GWW_TRY(pb.copy(g->ln_w, e->lnw, d, 1.f));
    GWW_TRY(pb.copy(g->ln_b, e->lnb, d, 1.f));
  }
  for (int i = 0; i < n_layers; ++i) {
    const unsigned m = dirty ? dirty[i] : 15u;
    if (!m) continue;
    const gww_enc_layer& L = layers[i];
    LayerW& w = e->layers[i];
    const size_t dd = (size_t)d * d;
    if (m & 1u) {
      GWW_REQUIRE(L.ln1_w && L.ln1_b && L.q_w && L.q_b && L.k_w && L.v_w && L.v_b,
                  "gww_encoder_set_weights: NULL attention weight in layer %d", i);
      // q in LOG2 UNITS on every bf16 panel (forward kernels of attention.hip: p = exp2(s) with no multiply per score;
      // attention_bwd.hip and the DoRA-gradient scale of q follow suit): log2(e) / 8 instead of 1 / 8.  The fp32 parity
      // panels keep natural units.
      const float qs16 = attention_log2q_enabled() ? qs * 1.44269504088896340736f : qs;
      GWW_TRY(pb.pack(L.q_w, w.wqkv, 1, d, d, 1, d, qs16));
      GWW_TRY(pb.pack(L.q_w, w.wqkv32, 0, d, d, 1, d, qs));
      GWW_TRY(pack(L.k_w, w.wqkv + dd, w.wqkv32 + dd, d, d, 1, d, 1.f));
      GWW_TRY(pack(L.v_w, w.wqkv + 2 * dd, w.wqkv32 + 2 * dd, d, d, 1, d, 1.f));
      GWW_TRY(pb.copy(L.q_b, w.bqkv, d, qs));
      GWW_TRY(pb.copy(nullptr, w.bqkv + d, d, 0.f));   // k_proj has no bias
      GWW_TRY(pb.copy(L.v_b, w.bqkv + 2 * d, d, 1.f));
      GWW_TRY(pb.copy(L.q_b, w.bqkv16, d, qs16));
      GWW_TRY(pb.copy(nullptr, w.bqkv16 + d, d, 0.f));
      GWW_TRY(pb.copy(L.v_b, w.bqkv16 + 2 * d, d, 1.f));
      GWW_TRY(pb.copy(L.ln1_w, w.ln1w, d, 1.f));
      GWW_TRY(pb.copy(L.ln1_b, w.ln1b, d, 1.f));
      // gain-folded panel + correction vectors for the algebraic LayerNorm of the A-stationary GEMM
      // (the A-stationary inference path feeds k_attention_l2_bf16, which takes q in log2 units: log2(e) rides in
      // the q panel, one rounding of the fp32 product instead of a second one on bf16 q)
      GWW_TRY(pb.ln_fold(L.q_w, L.ln1_w, L.ln1_b, L.q_b, qs16, d, d, w.wqkv_ln, w.uqkv, w.cbqkv));
      GWW_TRY(pb.ln_fold(L.k_w, L.ln1_w, L.ln1_b, nullptr, 1.f, d, d, w.wqkv_ln + dd, w.uqkv + d, w.cbqkv + d));
      GWW_TRY(pb.ln_fold(L.v_w, L.ln1_w, L.ln1_b, L.v_b, 1.f, d, d, w.wqkv_ln + 2 * dd, w.uqkv + 2 * d,
                             w.cbqkv + 2 * d));
      GWW_TRY(pt.transpose(w.wqkv, w.wqkvT, 3 * d, d));   // [N][K] -> [K][N] for the backward dX GEMM
    }
    if (m & 2u) {
      GWW_REQUIRE(L.o_w && L.o_b, "gww_encoder_set_weights: NULL out_proj weight in layer %d", i);
      GWW_TRY(pack(L.o_w, w.wo, w.wo32, d, d, 1, d, 1.f));
      GWW_TRY(pb.copy(L.o_b, w.bo, d, 1.f));
      GWW_TRY(pt.transpose(w.wo, w.woT, d, d));
    }
    if (m & 4u) {
      GWW_REQUIRE(L.ln2_w && L.ln2_b && L.fc1_w && L.fc1_b, "gww_encoder_set_weights: NULL fc1 weight in layer %d", i);
      GWW_TRY(pack(L.fc1_w, w.w1, w.w132, F, d, 1, d, 1.f));
      GWW_TRY(pb.copy(L.fc1_b, w.b1, F, 1.f));
      GWW_TRY(pb.copy(L.ln2_w, w.ln2w, d, 1.f));
      GWW_TRY(pb.copy(L.ln2_b, w.ln2b, d, 1.f));
      GWW_TRY(pb.ln_fold(L.fc1_w, L.ln2_w, L.ln2_b, L.fc1_b, 1.f, F, d, w.w1_ln, w.u1, w.cb1));
      GWW_TRY(pt.transpose(w.w1, w.w1T, F, d));
    }
    if (m & 8u) {
      GWW_REQUIRE(L.fc2_w && L.fc2_b, "gww_encoder_set_weights: NULL fc2 weight in layer %d", i);
      GWW_TRY(pack(L.fc2_w, w.w2, w.w232, d, F, 1, F, 1.f));
      GWW_TRY(pb.copy(L.fc2_b, w.b2, d, 1.f));
      GWW_TRY(pt.transpose(w.w2, w.w2T, d, F));
    }
  }
  GWW_TRY(pb.flush());
  GWW_TRY(pt.flush());
  // the fused-MLP weight stream of layer i: folded fc1 panel, fc2 and the folded q / k / v panel of layer i + 1
  if (mlp_fused_supported(d, F)) {
    for (int i = 0; i < n_layers; ++i) {
      const unsigned m = dirty ? dirty[i] : 15u, mn = i + 1 < n_layers ? (dirty ? dirty[i + 1] : 15u) : 0u;
      if (!(m & 14u) && !(mn & 1u)) continue;   // (bit 1: out_proj, in front of the wmlp_op stream)
      LayerW& w = e->layers[i];
      const void* wq_next = i + 1 < n_layers ? e->layers[i + 1].wqkv_ln : nullptr;
      // Only the stream the active path consumes is packed: the inference and the training forward both run the block with
      // out_proj in front (wmlp_op); the stream without it serves the debug paths GWW_GENERIC_PATH bits 4 / 7 alone (a
      // DoRA step used to pay two full fc1 + fc2 + q/k/v stream packs per layer, 2 x 3.2 MB of writes, for one consumer).
      const bool plain_stream = (generic_path_mask() & (GP_QKV | GP_OUT_PROJ)) != 0;
      if (plain_stream && ((m & 12u) || (mn & 1u))) GWW_TRY(launch_mlp_pack(w.w1_ln, w.w2, wq_next, w.wmlp, d, F, 3 * d, s));
      GWW_TRY(launch_mlp_pack(w.w1_ln, w.w2, wq_next, w.wmlp_op, d, F, 3 * d, s, w.wo));
    }
    if (!dirty || (dirty[0] & 1u))   // layer 0's folded q / k / v panel alone (no MLP in front of it)
      GWW_TRY(launch_mlp_pack(nullptr, nullptr, e->layers[0].wqkv_ln, e->layers[0].wqkv_st, d, 0, 3 * d, s));
  }
  return GWW_OK;
}

extern "C" int gww_encoder_set_weights(gww_encoder* e, const gww_enc_globals* g, const gww_enc_layer* layers,
                                       int n_layers, void* stream) {
  GWW_REQUIRE(e && g && layers, "gww_encoder_set_weights: NULL argument");
  GWW_REQUIRE(n_layers == e->cfg.n_layers, "gww_encoder_set_weights: got %d layers, handle has %d", n_layers,
              e->cfg.n_layers);
  GWW_TRY(pack_weights(e, g, layers, n_layers, nullptr, (hipStream_t)stream));
  e->ready = true;
  return GWW_OK;
}

// Re-pack only what changed since the last (full) gww_encoder_set_weights: `globals` may be NULL (stem, positions,
// final LayerNorm unchanged); layer_dirty[i] is the group mask above (0 = layer untouched; pointers of clean
// groups are not read).  A DoRA step touches group 1 (and 2) only: 15 small kernels per layer instead of 40.
extern "C" int gww_encoder_update_weights(gww_encoder* e, const gww_enc_globals* globals_or_null,
                                          const gww_enc_layer* layers, int n_layers, const unsigned* layer_dirty,
                                          void* stream) {
  GWW_REQUIRE(e && layers && layer_dirty, "gww_encoder_update_weights: NULL argument");
  GWW_REQUIRE(n_layers == e->cfg.n_layers, "gww_encoder_update_weights: got %d layers, handle has %d", n_layers,
              e->cfg.n_layers);
  if (!e->ready) return fail(GWW_ERR_STATE, "gww_encoder_update_weights: call gww_encoder_set_weights first");
  return pack_weights(e, globals_or_null, layers, n_layers, layer_dirty, (hipStream_t)stream);
}

namespace {
struct WsLayout {
  size_t melT, c1, x, x2, h, d2, qkv, ctx, f1, total;
};
WsLayout ws_layout(const gww_enc_cfg& c, int B, int precision) {
  const size_t es = precision == GWW_PREC_BF16 ? 2 : 4;
  const size_t d = c.d_model, F = c.ffn, Tin = c.t_in, T = c.t_in / 2, C = c.n_mels, Kc1 = conv1_kpad(c.n_mels);
  WsLayout w{};
  Arena a;
  const size_t Mp = padded_rows((size_t)B * T);
  w.melT = a.take(((size_t)B * (Tin + 2) * C + Kc1) * es);
  w.c1 = a.take((((size_t)B * (Tin + 2) + 255) / 256 * 256 + 520) * d * es);   // (+ 520: conv2's 256-row panels read 2 * 255 + 3 rows past the last segment)
  w.x = a.take(Mp * d * 4);
  w.x2 = a.take(Mp * d * 4);      // ping-pong partner of x for the fused residual-add prologue
  w.h = a.take(Mp * d * es);      // LayerNorm output, or out_proj delta on the A-stationary path
  w.d2 = a.take(Mp * d * es);     // fc2 delta on the A-stationary path
  w.qkv = a.take(Mp * 3 * d * es);
  w.ctx = a.take(Mp * d * es);
  w.f1 = a.take(Mp * F * es);
  w.total = a.total();
  return w;
}

// ---- the constant-tail shortcut of the bf16 inference stem (stem_tail.hip).  Its buffers live in workspace that is idle
// during the stem -- x2, the ping-pong partner of the residual stream, first written by layer 0 -- and its flag in the first
// word of melT, which the direct conv1 never touches: gww_encoder_workspace_bytes is unchanged.
struct StemTailLayout {
  size_t c1s, xs, tr, dump, total;   // byte offsets inside x2
};
StemTailLayout stem_tail_layout(int B, int d) {
  StemTailLayout t{};
  Arena a;
  // (like c1: conv2's 256-row panels read 2 * 255 + 3 rows past the last segment)
  t.c1s = a.take((((size_t)B * (kStemTc + 2) + 255) / 256 * 256 + 520) * d * 2);
  t.xs = a.take((size_t)B * kStemTt * d * 4);
  t.tr = a.take((size_t)B * d * 4);
  t.dump = a.take((size_t)d * 4);
  t.total = a.total();
  return t;
}

// ---- the plan of one inference forward: EVERY choice of kernels, made once from the handle, the batch, the precision and the
// outputs wanted (the lab mask included: generic_path_mask, encoder_impl.h).  The stem and the layer walks below only run it.
enum Conv1Kind { CONV1_DIRECT, CONV1_ASTAT, CONV1_GENERIC };
enum Conv2Kind { CONV2_V4, CONV2_FULLN, CONV2_GENERIC };
struct FwdWants {
  bool last_hidden, last_token, hidden_slab, attn_slab;
};
struct FwdPlan {
  Conv1Kind conv1;   // k_conv1_mel on the [B, mels, T] features themselves | transposition + A-stationary GEMM | + generic GEMM
  Conv2Kind conv2;   // the eight-phase 256 x 256 GEMM over overlapping rows (gemm_v4.hip) | k_gemm_fulln | generic GEMM
  bool shortcut;     // the stem's constant-tail shortcut: its compact conv1 / conv2 run in front of the direct conv1 and v4 conv2
  bool x0_layer0;    // ... and layer 0 forms x in registers from what they left (k_mlp_fused<., ., true>): no k_stem_fill
  bool astat;        // the A-stationary walk (K = d <= 512), else the generic one
  bool mlp_fused;    // LN2 + fc1 + GELU + fc2 in k_mlp_fused
  bool fuse_qkv;     // ... with the next layer's LN1 + q / k / v behind it
  bool lnqkv0;       // layer 0's LN1 + q / k / v on the fused kernel's prologue + tail
  bool op;           // out_proj in front of the fused block
  bool fuse_final;   // the last block ends in the encoder's final LayerNorm and writes last_hidden
  bool pooled;       // only the last token wanted: the last layer runs on B rows above its attention
  bool q_log2;       // the LN-folded q panel carries log2(e) (pack_weights)
  bool x_native;     // between the fused blocks the residual stream stays in accumulator order (x_native_offset, common.h)
};
FwdPlan plan_forward(const gww_encoder* e, int batch, int precision, FwdWants want) {
  const gww_enc_cfg& c = e->cfg;
  const int m = generic_path_mask(), d = c.d_model, F = c.ffn, T = c.t_in / 2;
  const bool bf = precision == GWW_PREC_BF16;
  FwdPlan p{};
  // bf16, the widths of whisper-tiny / -base / -small / -medium: conv1_mel.hip (no token-major copy of the input, W-stationary, one launch)
  p.conv1 = !bf || (m & GP_CONV1) ? CONV1_GENERIC
            : conv1_mel_supported(c.n_mels, d, conv1_kpad(c.n_mels)) ? CONV1_DIRECT : d % 128 == 0 ? CONV1_ASTAT : CONV1_GENERIC;
  p.conv2 = bf && d % 128 == 0 && d <= 3072 && !(m & GP_CONV2) ? CONV2_V4
            : bf && (d == 384 || d == 512) && !(m & GP_CONV2_FULLN) ? CONV2_FULLN : CONV2_GENERIC;
  const auto x2_bytes = [&] { const WsLayout w = ws_layout(c, batch, precision); return w.h - w.x2; };
  p.shortcut = p.conv1 == CONV1_DIRECT && p.conv2 == CONV2_V4 && e->stem_shortcut && batch > 0 && !(m & GP_STEM_SHORTCUT) &&
               stem_tail_supported(c.t_in, d) && stem_tail_layout(batch, d).total <= x2_bytes();
  // d = 512 (whisper-base): since round 3 the LayerNorm kernel + the 256 x 256 GEMM (k_gemm_bf16_v3) beat the LN-fused
  // A-stationary layer GEMMs there (8.78 against 9.33 ms per 64 segments; bit 9 of the mask brings them back)
  p.astat = bf && (d == 384 || (d == 512 && (m & GP_ASTAT_512))) && F % 128 == 0 && !(m & GP_LAYER_GEMMS);
  p.mlp_fused = p.astat && mlp_fused_supported(d, F) && !(m & GP_MLP);
  p.fuse_qkv = p.mlp_fused && !(m & GP_QKV);
  p.lnqkv0 = p.fuse_qkv && !(m & GP_LNQKV0);
  p.op = p.fuse_qkv && !(m & GP_OUT_PROJ);   // (fuse_qkv: every block then leaves xc complete, no delta pending in front of the next)
  p.fuse_final = p.op && want.last_hidden && !(m & GP_FINAL_LN);
  // per-layer outputs wanted: every layer runs on all rows
  p.pooled = bf && !want.last_hidden && want.last_token && T >= 3 && !(m & GP_POOLED) && !want.hidden_slab && !want.attn_slab;
  // Layer 0 forms the residual stream itself where both of its launches are the fused ones and nothing else reads x before the
  // block has rewritten it: the fill launch, its 0.59 GB store and the two 0.59 GB reads of it are gone.  Per-layer hidden
  // states (tap_hidden reads x in HBM), a last or pooled layer 0 and the generic paths keep the fill.
  p.x0_layer0 = p.shortcut && p.lnqkv0 && p.op && !want.hidden_slab && c.n_layers > 1;
  p.q_log2 = attention_log2q_enabled();
  // Block l's x_next has one reader where every block is the fused ctx block and the last one writes last_hidden: block l + 1,
  // by the lanes that wrote it.  It then never needs row order in HBM.  Whoever else reads x there -- a hidden slab, the pooled
  // last layer, a stand-alone kernel of a generic path -- keeps it in rows.  (The order lives in x alone, whose padded_rows
  // cover whole 128-row panels; a half batch of the split has its own x, so its first row opens a panel.)
  p.x_native = e->x_native && p.op && p.fuse_final && !p.pooled && !want.hidden_slab && c.n_layers > 1 && d == 384 &&
               mlp_fused_x_native_supported() && !(m & GP_X_NATIVE) &&
               x_native_bytes((long)batch * T) <= padded_rows((size_t)batch * T) * d * 4;
  return p;
}
}  // namespace

constexpr int kSplitMin = 32;   // segments per half below which splitting does not pay

static bool use_split(const gww_encoder* e, int batch) { return e->split && batch >= 2 * kSplitMin; }

extern "C" size_t gww_encoder_workspace_bytes(const gww_encoder* e, int batch, int precision) {
  if (!e || batch <= 0) return 0;
  if (use_split(e, batch)) {
    const int b0 = batch / 2;
    return ws_layout(e->cfg, b0, precision).total + ws_layout(e->cfg, batch - b0, precision).total;
  }
  return ws_layout(e->cfg, batch, precision).total;
}

extern "C" int gww_encoder_set_stem_shortcut(gww_encoder* e, int on) {
  GWW_REQUIRE(e != nullptr, "gww_encoder_set_stem_shortcut: NULL handle");
  e->stem_shortcut = on != 0;
  return GWW_OK;
}

extern "C" int gww_encoder_set_x_native(gww_encoder* e, int on) {
  GWW_REQUIRE(e != nullptr, "gww_encoder_set_x_native: NULL handle");
  e->x_native = on != 0;
  return GWW_OK;
}

// (host only: the layout function itself, for tests and tools)
extern "C" size_t gww_x_native_offset(long row, int col, long M) {
  if (row < 0 || col < 0 || col >= 384 || M <= 0) return (size_t)-1;
  return x_native_offset(row, col, M);
}
extern "C" size_t gww_x_native_bytes(long M) { return M > 0 ? x_native_bytes(M) : 0; }

// The device flags of the last forward that ran in `workspace` with this batch and precision (blocking; synchronise the
// forward's stream first): flags[i] = 1 where half batch i took the shortcut, 0 where it ran the full stem, -1 where the
// shortcut does not apply (switched off, fp32, a generic path, no second half).
extern "C" int gww_encoder_stem_shortcut_flags(const gww_encoder* e, int batch, int precision, const void* workspace,
                                               int* flags) {
  GWW_REQUIRE(e && workspace && flags, "gww_encoder_stem_shortcut_flags: NULL argument");
  GWW_REQUIRE(batch > 0 && (precision == GWW_PREC_BF16 || precision == GWW_PREC_F32),
              "gww_encoder_stem_shortcut_flags: bad batch %d / precision %d", batch, precision);
  flags[0] = flags[1] = -1;
  const bool split = use_split(e, batch);
  const int b[2] = {split ? batch / 2 : batch, split ? batch - batch / 2 : 0};
  size_t off = 0;
  for (int i = 0; i < 2 && b[i] > 0; ++i) {
    const WsLayout w = ws_layout(e->cfg, b[i], precision);
    if (plan_forward(e, b[i], precision, FwdWants{}).shortcut)
      GWW_HIP(hipMemcpy(&flags[i], (const char*)workspace + off + w.melT, sizeof(int), hipMemcpyDeviceToHost));
    off += w.total;
  }
  return GWW_OK;
}

extern "C" int gww_encoder_set_split(gww_encoder* e, int on) {
  GWW_REQUIRE(e != nullptr, "gww_encoder_set_split: NULL handle");
  if (on && !e->s2[0]) {
    for (int i = 0; i < 2; ++i) {
      GWW_HIP(hipStreamCreateWithFlags(&e->s2[i], hipStreamNonBlocking));
      GWW_HIP(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming));
    }
    GWW_HIP(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    GWW_HIP(hipEventCreateWithFlags(&e->ev_skew, hipEventDisableTiming));
  }
  e->split = on ? 1 : 0;
  return GWW_OK;
}

// optional per-kernel event trace: TR(cls, launch-expression) around a launch on tr's stream
struct Tracer {
  gww_encoder* e;
  hipStream_t s;
  int begin(int cls) {
    if (!e->trace) return GWW_OK;
    TraceSpan sp{cls, nullptr, nullptr};
    for (hipEvent_t* ev : {&sp.a, &sp.b}) {
      if (!e->pool.empty()) { *ev = e->pool.back(); e->pool.pop_back(); }
      else GWW_HIP(hipEventCreate(ev));
    }
    GWW_HIP(hipEventRecord(sp.a, s));
    e->spans.push_back(sp);
    return GWW_OK;
  }
  int end() {
    if (!e->trace) return GWW_OK;
    GWW_HIP(hipEventRecord(e->spans.back().b, s));
    return GWW_OK;
  }
};
#define TR(cls, expr)        \
  do {                       \
    GWW_TRY(tr.begin(cls));  \
    GWW_TRY(expr);           \
    GWW_TRY(tr.end());       \
  } while (0)

// One inference forward of one (half) batch: the plan, the carved workspace, the outputs and the launches every part shares.
// hidden_slab / attn_slab (gww_encoder_forward_outputs): per-layer outputs, layer l at + l * hs_stride / as_stride
// elements.  They only ADD stores and launches: every launch that feeds last_hidden is the one the plain forward makes.
struct Fwd {
  gww_encoder* e;
  FwdPlan p;
  Tracer tr;
  hipStream_t s;
  bool bf;
  int B, d, F, T, H, n_layers;
  long M;
  void *melT, *c1, *h, *d2, *qkv, *ctx, *f1;
  float *x, *x2;
  // the compact stem's buffers (in x2) and flag (shortcut)
  int* st_flag;
  void* c1s;
  float *xs, *st_tr, *st_dump;
  MfX0 x0;
  float *last_hidden, *last_token, *hidden_slab, *attn_slab;
  size_t hs_stride, as_stride;
  hipEvent_t skew_event;

  // generic GEMM dispatch on precision
  int gemm(const void* A, long lda, const void* W16, const float* W32, const float* bias, const float* resid, const float* pos,
           void* Cout, long Mr, int N, int K, int epi, int rpb) const {
    return bf ? launch_gemm_bf16(A, lda, W16, bias, resid, pos, Cout, Mr, N, K, epi, rpb, s, /*rows_padded_256=*/1)
              : launch_gemm_f32((const float*)A, lda, W32, bias, resid, pos, (float*)Cout, Mr, N, K, epi, rpb, s);
  }
  // per-layer outputs: hidden_states[l] = the residual stream entering layer l (complete: no delta pending where it is
  // tapped), attentions[l] = softmax of the q / k in qkv, read before the next launch overwrites qkv;
  // hidden_states[L] = last_hidden (a copy unless the caller placed last_hidden in the slab)
  int tap_hidden(int l, const float* src) const {
    if (hidden_slab)
      GWW_HIP(hipMemcpyAsync(hidden_slab + (size_t)l * hs_stride, src, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
    return GWW_OK;
  }
  int tap_attn(int l) const {
    if (attn_slab) GWW_TRY(launch_attention_probs(qkv, bf, bf && p.q_log2, attn_slab + (size_t)l * as_stride, B, T, H, s));
    return GWW_OK;
  }
  int tap_final() const {
    float* dst = hidden_slab ? hidden_slab + (size_t)n_layers * hs_stride : nullptr;
    if (dst && dst != last_hidden)
      GWW_HIP(hipMemcpyAsync(dst, last_hidden, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
    return GWW_OK;
  }
  int stem(const float* mel);
  int walk_astat();
  int walk_generic();
  int pooled_last_layer(const LayerW& L, const float* x, float* rows, void* hb);
  int final_layernorm(const float* xc, const void* pending);
};

// ---- stem.  The constant tail of a padded log-mel (stem_tail.hip): detection, then the stem on the first kStemTc frames and
// the fill of x, all predicated on the device flag; the full stem stays enqueued behind them and returns at once when the flag
// is 1, so it never reads the (then stale) c1.  One span per trace class: bench.py indexes its table by their names.
int Fwd::stem(const float* mel) {
  const int Tin = e->cfg.t_in, C = e->cfg.n_mels, Kc1 = conv1_kpad(C);
  const size_t es = bf ? 2 : 4;
  auto conv1_direct = [&]() -> int {
    if (p.shortcut) {
      GWW_TRY(launch_stem_detect(mel, st_flag, (long)B * C, Tin, s));
      GWW_TRY(launch_conv1_mel(mel, e->c1w, e->c1b, c1s, B, kStemTc, d, s, Tin, st_flag, 1));
    }
    return launch_conv1_mel(mel, e->c1w, e->c1b, c1, B, Tin, d, s, 0, p.shortcut ? st_flag : nullptr, 0);
  };
  auto conv2_v4 = [&]() -> int {
    const int Np = (d + 255) / 256 * 256;
    if (p.shortcut) {
      GWW_TRY(launch_gemm_bf16_v4(c1s, 2L * d, e->c2w, e->c2b, nullptr, xs, (long)B * (kStemTt + 1), Np, 3 * d, EPI_CONV2, s, 0,
                                  e->pos_c, kStemTt + 1, d, st_dump, st_flag, 1, st_tr, kStemTt - 2));
      if (!p.x0_layer0) GWW_TRY(launch_stem_fill(xs, st_tr, e->pos, x, st_flag, B, T, d, s));
    }
    return launch_gemm_bf16_v4(c1, 2L * d, e->c2w, e->c2b, nullptr, x, (long)B * (T + 1), Np, 3 * d, EPI_CONV2, s, 0, e->pos,
                               T + 1, d, x + (((size_t)B * T + 255) / 256 * 256) * d, p.shortcut ? st_flag : nullptr, 0);
  };
  if (p.conv1 != CONV1_DIRECT) {   // the transposition kernel + a GEMM over its rows
    TR(TR_MEL, launch_mel_to_tokens(mel, melT, bf ? 1 : 0, B, C, Tin, s));
    GWW_HIP(hipMemsetAsync((char*)melT + (size_t)B * (Tin + 2) * C * es, 0, Kc1 * es, s));
    GWW_HIP(hipMemsetAsync(c1, 0, (size_t)d * es, s));   // zero row 0 of batch 0 (token -1)
  }
  if (p.conv1 == CONV1_DIRECT)
    TR(TR_CONV1, conv1_direct());
  else if (p.conv1 == CONV1_ASTAT)
    TR(TR_CONV1, launch_gemm_astat(melT, C, nullptr, nullptr, nullptr, nullptr, e->c1w, e->c1b, c1,
                                   (long)B * (Tin + 2), d, Kc1, EPI_CONV1, Tin + 2, s));
  else
    TR(TR_CONV1, gemm(melT, C, e->c1w, e->c1w32, e->c1b, nullptr, nullptr, c1, (long)B * (Tin + 2), d, Kc1,
                      EPI_CONV1, Tin + 2));
  if (p.conv2 == CONV2_V4)
    TR(TR_CONV2, conv2_v4());
  else if (p.conv2 == CONV2_FULLN)
    TR(TR_CONV2, launch_gemm_fulln(c1, 2L * d, e->c2w, e->c2b, e->pos, x, (long)B * (T + 1), d, 3 * d, EPI_CONV2, T + 1, s));
  else
    TR(TR_CONV2, gemm(c1, 2L * d, e->c2w, e->c2w32, e->c2b, nullptr, e->pos, x, (long)B * (T + 1), d, 3 * d, EPI_CONV2,
                      T + 1));
  return GWW_OK;
}

// The last layer when only the last token is wanted (Signal_vs_Noise/src/model.py:25-26): everything above the last
// attention is row-wise.  Attention for the one query tile that holds token T-1, then out_proj / LN2 / fc1 / GELU / fc2 /
// final LayerNorm on the B last-token rows.  x: the complete residual stream entering the layer; rows: 3 x [B, d] fp32
// of scratch (x rows (b, T-1) | x_mid | layer output); hb: [B, d] bf16 of scratch.
int Fwd::pooled_last_layer(const LayerW& L, const float* x, float* rows, void* hb) {
  TR(TR_ATTN, launch_attention_bf16(qkv, ctx, B, T, H, s, nullptr, /*last_tile_only=*/true, p.q_log2));
  float* xl = rows;
  float* xm = rows + (size_t)B * d;
  float* xf = rows + 2 * (size_t)B * d;
  GWW_HIP(hipMemcpy2DAsync(xl, (size_t)d * 4, x + (size_t)(T - 1) * d, (size_t)T * d * 4, (size_t)d * 4, B,
                           hipMemcpyDeviceToDevice, s));
  TR(TR_OUT, launch_gemm_bf16((const unsigned short*)ctx + (size_t)(T - 1) * d, (long)T * d, L.wo, L.bo, xl, nullptr,
                              xm, B, d, d, EPI_RESID, 0, s, 0));
  TR(TR_LNROWS, launch_layernorm(xm, L.ln2w, L.ln2b, hb, 1, B, d, s));
  TR(TR_FC1, launch_gemm_bf16(hb, d, L.w1, L.b1, nullptr, nullptr, f1, B, F, d, EPI_GELU, 0, s, 0));
  TR(TR_FC2, launch_gemm_bf16(f1, F, L.w2, L.b2, xm, nullptr, xf, B, d, F, EPI_RESID, 0, s, 0));
  TR(TR_LNROWS, launch_layernorm_rows(xf, d, e->lnw, e->lnb, last_token, B, d, s, nullptr));
  return GWW_OK;
}

// ---- final LayerNorm (HF:modeling_whisper.py:642), with the last pending delta folded in;
// callers pool token T-1 (Signal_vs_Noise/src/model.py:25-26): that row alone is a fast output
int Fwd::final_layernorm(const float* xc, const void* pending) {
  if (last_hidden) TR(TR_LN, launch_layernorm(xc, e->lnw, e->lnb, last_hidden, 0, M, d, s, pending));
  if (last_token)
    TR(TR_LNROWS, launch_layernorm_rows(xc + (long)(T - 1) * d, (long)T * d, e->lnw, e->lnb, last_token, B, d, s,
                                        pending ? (const char*)pending + (size_t)(T - 1) * d * 2 : nullptr));
  if (last_hidden) GWW_TRY(tap_final());
  return GWW_OK;
}

// ---- the A-stationary walk (bf16, K = d <= 512: A panel in registers, fused residual-add + LayerNorm prologue).
// Deferred residual: out_proj / fc2 emit a bf16 delta; the NEXT LayerNorm prologue does x_new = x + delta (written to the
// spare buffer), LN(x_new) -> GEMM operand.  What survives an iteration:
struct AstatState {
  float* xc;             // the residual stream, complete but for `pending`
  float* xn;             // the spare buffer: whoever adds a delta to xc writes the sum here (x_new), then swap()
  const void* pending;   // bf16 delta not yet added to xc
  bool qkv_ready;        // the previous block already left this layer's q / k / v in qkv (then nothing is pending)
  void swap() { std::swap(xc, xn); }
};

int Fwd::walk_astat() {
  AstatState st{x, x2, nullptr, false};
  void* const d1 = h;   // out_proj delta, where it is a launch of its own
  auto args = [&]() { MlpFusedArgs a; a.who = "gww_encoder_forward"; a.M = M; a.d = d; return a; };
  auto with_qkv = [&](MlpFusedArgs& a, const LayerW& W) { a.qkv_u = W.uqkv; a.qkv_cb = W.cbqkv; a.qkv_out = qkv; a.NQ = 3 * d; };
  for (int i = 0; i < n_layers; ++i) {
    const LayerW& L = e->layers[i];
    const bool last = i == n_layers - 1, from_x0 = i == 0 && p.x0_layer0;
    // -- q / k / v, unless the previous block made it
    if (!st.qkv_ready) {
      if (i == 0 && p.lnqkv0) {
        // layer 0 (no delta pending behind the conv stem): the fused kernel's panel prologue + q / k / v tail
        MlpFusedArgs a = args();
        a.x = st.xc; a.Wt = L.wqkv_st;
        with_qkv(a, L);
        if (from_x0) a.x0 = &x0;
        TR(TR_QKV, launch_mlp_fused(a, s));
      } else {
        TR(TR_QKV, launch_gemm_astat(st.xc, d, st.pending, st.pending ? st.xn : nullptr, L.uqkv, L.cbqkv, L.wqkv_ln, nullptr, qkv,
                                     M, 3 * d, d, EPI_BIAS, 0, s));
        if (st.pending) st.swap();
        st.pending = nullptr;
      }
    }
    st.qkv_ready = false;
    // (xc is complete here: the q / k / v step folded any pending delta in; the spare buffer is free)
    GWW_TRY(tap_hidden(i, st.xc));
    if (i == 0 && skew_event) GWW_HIP(hipEventRecord(skew_event, s));   // the other half batch starts here
    if (p.pooled && last) return pooled_last_layer(L, st.xc, st.xn, d1);
    // -- attention
    TR(TR_ATTN, launch_attention_bf16(qkv, ctx, B, T, H, s, nullptr, false, p.q_log2));
    GWW_TRY(tap_attn(i));   // before the fused block below writes the next layer's q / k / v over qkv
    // -- one block step.  p.op: out_proj fused in front of the MLP block (ctx is the A operand of a GEMM into the block's idle
    // output accumulators; the bf16 delta never reaches HBM); it needs no delta pending on xc, which fuse_qkv guarantees
    if (!p.op)
      TR(TR_OUT, launch_gemm_astat(ctx, d, nullptr, nullptr, nullptr, nullptr, L.wo, L.bo, d1, M, d, d, EPI_BIAS, 0, s));
    // (layer 0 behind the compact stem forms x in registers and has no x_new: xs / tr live in that buffer until it has run)
    MlpFusedArgs a = args();
    a.x = st.xc; a.x_new = from_x0 ? nullptr : st.xn; a.ln_u = L.u1; a.ln_cb = L.cb1; a.b2 = L.b2; a.F = F;
    // (x_native: a block reads what the block before it left in accumulator order; layer 0 reads the stem's rows, and where it
    // forms them itself -- from_x0, an instantiation without that order -- it also writes rows and layer 1 starts the order)
    a.x_native_in = p.x_native && i > (p.x0_layer0 ? 1 : 0);
    if (p.op) { a.ctx = ctx; a.bo = L.bo; a.Wt = L.wmlp_op; }
    else { a.delta = d1; a.Wt = L.wmlp; }
    if (p.fuse_qkv && !last) {
      // fused + the next layer's LN1 + q / k / v: x_next comes back in xc itself (xn only held x_new), no delta is pending
      with_qkv(a, e->layers[i + 1]);
      if (from_x0) a.x0 = &x0;
      a.x_native_out = p.x_native && !from_x0;
      TR(TR_MLPQKV, launch_mlp_fused(a, s));
      st.qkv_ready = true;
    } else if (p.fuse_final) {
      // the LAST block with the encoder's final LayerNorm as its epilogue: last_hidden_state comes straight out of the
      // kernel (no bf16 delta, no second read of the residual stream, no LayerNorm launch); the pooled token is row
      // T - 1 of it, which the lanes that own it store to last_token as well
      a.lnf_w = e->lnw; a.lnf_b = e->lnb; a.y = last_hidden; a.last_token = last_token; a.T = T;
      TR(TR_MLPFIN, launch_mlp_fused(a, s));
      return tap_final();
    } else if (p.mlp_fused) {
      // fused plain: LN2 + fc1 + GELU + fc2 in one kernel, the [M, ffn] activation never leaves the CU
      a.C = d2; a.keep_x_new = true;   // (x_new becomes the residual stream)
      TR(TR_MLP, launch_mlp_fused(a, s));
      st.swap();
      st.pending = d2;
    } else {
      TR(TR_FC1, launch_gemm_astat(st.xc, d, d1, st.xn, L.u1, L.cb1, L.w1_ln, nullptr, f1, M, F, d, EPI_GELU, 0, s));
      st.swap();
      TR(TR_FC2, launch_gemm_fulln(f1, F, L.w2, L.b2, nullptr, d2, M, d, F, EPI_BIAS, 0, s));
      st.pending = d2;
    }
  }
  return final_layernorm(st.xc, st.pending);
}

// ---- the generic walk: fp32, and the bf16 widths without A-stationary kernels (e.g. whisper-small)
int Fwd::walk_generic() {
  for (int i = 0; i < n_layers; ++i) {
    const LayerW& L = e->layers[i];
    GWW_TRY(tap_hidden(i, x));
    TR(TR_LN, launch_layernorm(x, L.ln1w, L.ln1b, h, bf ? 1 : 0, M, d, s));
    TR(TR_QKV, gemm(h, d, L.wqkv, L.wqkv32, bf ? L.bqkv16 : L.bqkv, nullptr, nullptr, qkv, M, 3 * d, d, EPI_BIAS, 0));
    if (p.pooled && i == n_layers - 1) return pooled_last_layer(L, x, x2, h);
    if (bf) TR(TR_ATTN, launch_attention_bf16(qkv, ctx, B, T, H, s, nullptr, false, p.q_log2));
    else TR(TR_ATTN, launch_attention_f32((const float*)qkv, (float*)ctx, B, T, H, s));
    GWW_TRY(tap_attn(i));
    TR(TR_OUT, gemm(ctx, d, L.wo, L.wo32, L.bo, x, nullptr, x, M, d, d, EPI_RESID, 0));
    TR(TR_LN, launch_layernorm(x, L.ln2w, L.ln2b, h, bf ? 1 : 0, M, d, s));
    TR(TR_FC1, gemm(h, d, L.w1, L.w132, L.b1, nullptr, nullptr, f1, M, F, d, EPI_GELU, 0));
    TR(TR_FC2, gemm(f1, F, L.w2, L.w232, L.b2, x, nullptr, x, M, d, F, EPI_RESID, 0));
  }
  return final_layernorm(x, nullptr);
}
#undef TR

// the argument checks and the workspace carve-up; the stem and the layer walks run the plan and decide nothing themselves
static int forward_impl(gww_encoder* e, const float* mel, int batch, int precision, void* workspace,
                        size_t workspace_bytes, float* last_hidden, float* last_token, void* stream,
                        hipEvent_t skew_event = nullptr, float* hidden_slab = nullptr, float* attn_slab = nullptr,
                        size_t hs_stride = 0, size_t as_stride = 0) {
  GWW_REQUIRE(e && mel, "gww_encoder_forward: NULL argument");
  if (!e->ready) return fail(GWW_ERR_STATE, "gww_encoder_forward: weights not set");
  GWW_REQUIRE(precision == GWW_PREC_BF16 || precision == GWW_PREC_F32, "gww_encoder_forward: bad precision %d",
              precision);
  GWW_REQUIRE(batch >= 0, "gww_encoder_forward: batch < 0");
  GWW_REQUIRE(last_hidden || last_token, "gww_encoder_forward: no output requested");
  if (batch == 0) return GWW_OK;
  GWW_REQUIRE((((uintptr_t)mel) & 15) == 0 && (((uintptr_t)workspace) & 255) == 0,
              "gww_encoder_forward: mel must be 16-byte and workspace 256-byte aligned");
  const WsLayout w = ws_layout(e->cfg, batch, precision);
  if (!workspace || workspace_bytes < w.total)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_forward: workspace %zu bytes < required %zu", workspace_bytes,
                w.total);
  const gww_enc_cfg& c = e->cfg;
  char* base = (char*)workspace;
  const StemTailLayout st = stem_tail_layout(batch, c.d_model);
  char* const st_base = base + w.x2;
  Fwd f{};
  f.e = e;
  f.p = plan_forward(e, batch, precision, {last_hidden != nullptr, last_token != nullptr, hidden_slab != nullptr, attn_slab != nullptr});
  f.s = (hipStream_t)stream;
  f.tr = Tracer{e, f.s};
  f.bf = precision == GWW_PREC_BF16;
  f.B = batch; f.d = c.d_model; f.F = c.ffn; f.T = c.t_in / 2; f.H = c.n_heads; f.n_layers = c.n_layers;
  f.M = (long)batch * f.T;
  f.melT = base + w.melT; f.c1 = base + w.c1; f.h = base + w.h; f.d2 = base + w.d2; f.qkv = base + w.qkv; f.ctx = base + w.ctx;
  f.f1 = base + w.f1; f.x = (float*)(base + w.x); f.x2 = (float*)(base + w.x2);
  f.st_flag = (int*)f.melT; f.c1s = st_base + st.c1s; f.xs = (float*)(st_base + st.xs); f.st_tr = (float*)(st_base + st.tr);
  f.st_dump = (float*)(st_base + st.dump);
  f.x0 = MfX0{f.xs, f.st_tr, e->pos, f.st_flag, f.T, kStemTt};
  f.last_hidden = last_hidden; f.last_token = last_token; f.hidden_slab = hidden_slab; f.attn_slab = attn_slab;
  f.hs_stride = hs_stride; f.as_stride = as_stride; f.skew_event = skew_event;
  GWW_TRY(f.stem(mel));
  return f.p.astat ? f.walk_astat() : f.walk_generic();
}

// the plain forward and gww_encoder_forward_outputs: with the split on, both slabs are offset for the second half as
// last_hidden is (their layer strides stay those of the full batch)
static int forward_split(gww_encoder* e, const float* mel, int batch, int precision, void* workspace,
                         size_t workspace_bytes, float* last_hidden, float* last_token, float* hidden_slab,
                         float* attn_slab, void* stream) {
  GWW_REQUIRE(e && mel, "gww_encoder_forward: NULL argument");
  const size_t T_ = (size_t)(e->cfg.t_in / 2);
  const size_t hs_stride = (size_t)(batch > 0 ? batch : 0) * T_ * e->cfg.d_model;
  const size_t as_stride = (size_t)(batch > 0 ? batch : 0) * e->cfg.n_heads * T_ * T_;
  if (batch <= 0 || !use_split(e, batch))
    return forward_impl(e, mel, batch, precision, workspace, workspace_bytes, last_hidden, last_token, stream, nullptr,
                        hidden_slab, attn_slab, hs_stride, as_stride);
  // two independent half batches on two streams, forked from / joined to the caller's stream
  hipStream_t s = (hipStream_t)stream;
  const int d = e->cfg.d_model, T = e->cfg.t_in / 2;
  const int b[2] = {batch / 2, batch - batch / 2};
  const size_t w0 = ws_layout(e->cfg, b[0], precision).total, w1 = ws_layout(e->cfg, b[1], precision).total;
  if (!workspace || workspace_bytes < w0 + w1)
    return fail(GWW_ERR_WORKSPACE, "gww_encoder_forward: workspace %zu bytes < required %zu", workspace_bytes, w0 + w1);
  GWW_HIP(hipEventRecord(e->ev_fork, s));
  int off = 0;
  static const int skew = (int)lab_int("GWW_SPLIT_SKEW", 0);   // tuning aid (lab build)
  for (int i = 0; i < 2; ++i) {
    GWW_HIP(hipStreamWaitEvent(e->s2[i], e->ev_fork, 0));
    if (i == 1 && skew) GWW_HIP(hipStreamWaitEvent(e->s2[1], e->ev_skew, 0));
    const int rc = forward_impl(e, mel + (size_t)off * e->cfg.n_mels * e->cfg.t_in, b[i], precision,
                                (char*)workspace + (i ? w0 : 0), i ? w1 : w0,
                                last_hidden ? last_hidden + (size_t)off * T * d : nullptr,
                                last_token ? last_token + (size_t)off * d : nullptr, e->s2[i],
                                (i == 0 && skew) ? e->ev_skew : nullptr,
                                hidden_slab ? hidden_slab + (size_t)off * T * d : nullptr,
                                attn_slab ? attn_slab + (size_t)off * e->cfg.n_heads * T_ * T_ : nullptr, hs_stride, as_stride);
    if (rc != GWW_OK) return rc;
    GWW_HIP(hipEventRecord(e->ev_join[i], e->s2[i]));
    GWW_HIP(hipStreamWaitEvent(s, e->ev_join[i], 0));
    off += b[i];
  }
  return GWW_OK;
}

extern "C" int gww_encoder_forward(gww_encoder* e, const float* mel, int batch, int precision, void* workspace,
                                   size_t workspace_bytes, float* last_hidden, float* last_token,
                                   void* stream) {
  return forward_split(e, mel, batch, precision, workspace, workspace_bytes, last_hidden, last_token, nullptr, nullptr,
                       stream);
}

extern "C" int gww_encoder_forward_outputs(gww_encoder* e, const float* mel, int batch, int precision, void* workspace,
                                           size_t workspace_bytes, float* last_hidden, float* hidden_slab,
                                           float* attn_slab, void* stream) {
  GWW_REQUIRE(e && mel, "gww_encoder_forward_outputs: NULL argument");
  // last_hidden may be left NULL when hidden_slab is given: layer L of the slab is then last_hidden_state itself
  if (!last_hidden && hidden_slab && batch > 0)
    last_hidden = hidden_slab + (size_t)e->cfg.n_layers * batch * (e->cfg.t_in / 2) * e->cfg.d_model;
  GWW_REQUIRE(last_hidden != nullptr, "gww_encoder_forward_outputs: no last_hidden and no hidden_slab");
  return forward_split(e, mel, batch, precision, workspace, workspace_bytes, last_hidden, nullptr, hidden_slab, attn_slab,
                       stream);
}

