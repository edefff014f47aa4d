/*
 * gww.h -- C ABI of libgww.so, the MI355X (gfx950) hot path of GW-Whisper.
 *
 * The reference (chayanchatterjee/GW-Whisper) is pure Python; its hot path is
 * the object protocol of three third-party classes.
 * There is therefore no FFI in the reference to mirror symbol-for-symbol; each
 * entry point below names the reference call it replaces (file:line relative to
 * the reference tree, "HF:" = the transformers package the reference imports).
 * The Python shim in gw_whisper_amd/ binds these with ctypes and presents the
 * reference's own call surface (WhisperFeatureExtractor / WhisperEncoder /
 * peft get_peft_model); INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless said otherwise
 *   - every launch is asynchronous on the caller's hipStream_t (passed as void*)
 *   - return value: 0 = ok, negative = error (gww_last_error() has the text)
 *   - the library keeps no global mutable state besides the per-thread error
 *     string; handles are thread-compatible (one handle per thread/stream)
 *   - plain C types only: no torch, no C++ in the signatures
 */
#ifndef GWW_H
#define GWW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GWW_VERSION 108  /* 0.1.8: the glitch, detection and binary heads take their layers in gww_mlp_params / _acts / _grads, every head backward takes ws_bytes; 0.1.7 (additions are symbols only): + gww_encoder_train_forward_f32 / _backward_f32, gww_train_saved_bytes_f32 / gww_train_workspace_bytes_f32, gww_attention_lse_f32, gww_attention_bwd_f32 / _scratch_bytes, gww_adapter_grads_f32 / _scratch_bytes (exact-fp32 DoRA / LoRA training step); + gww_adapter_grads / _scratch_bytes, gww_train_workspace_bytes_adapters (adapter gradients of fc1 / fc2 and of ranks 1..64; gww_dora_target.proj 4 / 5); + gww_encoder_forward_outputs, gww_attention_probs_bf16 / _f32 (per-layer hidden states and attention maps); + gww_info_nce_forward_f32 / _backward_f32, gww_qadapter_tail_backward_f32 / _workspace_bytes, gww_assemble_batch_f32 (MLGWSC-1 training program); + gww_gemm_wgrad_bf16 / _workspace_bytes, gww_layernorm_param_grads / _workspace_bytes, gww_encoder_train_backward_full, gww_train_workspace_bytes_full (full fine-tuning: base-weight gradients); + gww_dora_merge_batch_f32 (all adapted projections of a step in one launch), gww_conv1_gelu_bf16 (conv1 read from the [B, 80, T] feature layout); + gww_frontend_create_nmel, gww_logmel_host_nmel_f32 (128-bin front end of whisper-large-v3), gww_encoder_create takes n_mels 128; 0.1.6: + gww_qadapter_cnn_backward_f32 / _workspace_bytes (the Q-adapter CNN's backward as HIP kernels); 0.1.5: + gww_gemm_bf16_v4_split (explicit column split; no environment switch is read by the library any more); 0.1.4: gww_mlp_fused_bf16 / gww_attn_out_mlp_fused_bf16 with the q / k / v tail return x_next over x (x_out keeps x_new); 0.1.3: + gww_logmel_host_f32 (fork-safe CPU twin of the front end); 0.1.2: + whitening kernels, gww_qadapter_tail_f32, gww_attention_bwd_log2q_bf16, gww_lnqkv_fused_bf16, gww_attn_out_mlp_fused_bf16, gww_mlp_pack_op_bf16; the gww_mlp_pack_bf16 stream carries W1 / 8 and 8 W2 */

#define GWW_OK 0
#define GWW_ERR_ARG (-1)      /* bad argument (shape, null pointer, unsupported size) */
#define GWW_ERR_HIP (-2)      /* a HIP runtime call failed */
#define GWW_ERR_WORKSPACE (-3)/* caller's workspace too small */
#define GWW_ERR_STATE (-4)    /* handle not ready (weights not set) */

/* compute precision of the encoder path */
#define GWW_PREC_BF16 0  /* bf16 MFMA operands, fp32 accumulate / LN / softmax / residual */
#define GWW_PREC_F32 1   /* fp32 MFMA (v_mfma_f32_16x16x4_f32): exact fp32, the parity gate */

int gww_version(void);
const char* gww_last_error(void);

/* --------------------------------------------------------------------------
 * Front end: log-mel features.
 * Replaces WhisperFeatureExtractor.__call__ as used at
 *   Signal_vs_Noise/src/dataset.py:20-21,40 ; Glitch_classification/src/dataset.py:46
 *   (impl HF:models/whisper/feature_extraction_whisper.py:135-168,193-346).
 * wave   [n_seg, wave_stride] fp32, the first n_samples of each row are the
 *        16 kHz samples (zero padded / truncated to 480000 like HF does)
 * out    [n_seg, n_mels, 3000] fp32  == input_features (n_mels of the handle: 80, or 128 for large-v3)
 * seg_max[n_seg] fp32 scratch (per-segment max of the raw log10 mel)
 * Exact shortcut: frames that only see zero padding are filled with the one
 * constant HF would produce; only ceil((n_samples+200)/160) frames run a DFT.
 * (The sizes above are those of Whisper's published configuration; a handle from
 * gww_frontend_create_cfg, below, brings its own: out is [n_seg, n_mels, n_frames].)
 * -------------------------------------------------------------------------- */
typedef struct gww_frontend gww_frontend;
int gww_frontend_create(gww_frontend** out);          /* uploads window / twiddle / filterbank tables; 80 mels */
/* n_mels 80 or 128: HF's mel_filter_bank(201, n_mels, 0, 8000, 16000, slaney, slaney) */
int gww_frontend_create_nmel(int n_mels, gww_frontend** out);
void gww_frontend_destroy(gww_frontend* fe);
int gww_logmel_f32(gww_frontend* fe, const float* wave, int n_seg, int n_samples,
                   long wave_stride, float* out, float* seg_max, void* stream);
/* The same front end on the HOST: wave and out are HOST pointers, nothing here touches the GPU (no HIP call, no
 * handle, no global mutable state), so it may be called from forked DataLoader worker processes -- where the
 * reference calls the extractor: Signal_vs_Noise/src/dataset.py:12,20-21 under src/train.py:224-225
 * (num_workers 12).  Same arithmetic and the same dead-frame shortcut; double-precision FFT, fp32 result. */
int gww_logmel_host_f32(const float* wave, int n_seg, int n_samples, long wave_stride, float* out);   /* 80 mels */
/* the same with n_mels 80 or 128; out [n_seg, n_mels, 3000] */
int gww_logmel_host_nmel_f32(const float* wave, int n_seg, int n_samples, long wave_stride, int n_mels, float* out);

/* Any configuration of HF's WhisperFeatureExtractor(feature_size, sampling_rate, hop_length, chunk_length, n_fft):
 * zero-pad / truncate to n_samples = chunk_length * sampling_rate -> reflect-pad n_fft / 2 -> periodic-Hann n_fft-point
 * DFT every hop_length -> |X|^2 of frames 0 .. n_samples / hop_length - 1 -> slaney mel [n_mels, n_fft / 2 + 1] ->
 * log10(max(., 1e-10)) -> per-segment max -> max(x, max - 8) -> (x + 4) / 4.
 * Supported (anything else: GWW_ERR_ARG, the message names the field): n_fft even in [16, 1024]; 1 <= hop_length <= n_fft;
 * n_mels 80 or 128; n_samples > n_fft / 2; 1 <= n_frames = n_samples / hop_length <= 3000; 0 <= min_frequency <
 * max_frequency.  max_frequency is the one extension over HF, which fixes 8000 Hz.
 * A handle of Whisper's published configuration (16 kHz, 400, 160, 480000, 0 .. 8000 Hz) runs the same kernels as one
 * from gww_frontend_create_nmel; every other one runs the general kernels (csrc/logmel_any.hip).  gww_logmel_f32 then
 * writes out [n_seg, n_mels, n_frames]. */
typedef struct {
    int   n_mels, sampling_rate, n_fft, hop_length, n_samples;
    float min_frequency, max_frequency;
} gww_frontend_cfg;
/* GWW_OK if cfg is in the supported set, else GWW_ERR_ARG and a message naming the field; plain C++, no GPU, no data */
int gww_frontend_validate_cfg(const gww_frontend_cfg* cfg);
int gww_frontend_create_cfg(const gww_frontend_cfg* cfg, gww_frontend** out);
int gww_frontend_frames(const gww_frontend* fe);                       /* n_frames of the handle */
int gww_frontend_mel_filters_f32(const gww_frontend* fe, float* out);  /* HOST out [n_mels, n_fft / 2 + 1]; for tests */
/* the same filterbank without a handle or a GPU (plain C++, as the host twin below) */
int gww_frontend_mel_filters_host_f32(const gww_frontend_cfg* cfg, float* out);
/* for tests: on != 0 sends a handle of the published configuration through the general kernels too */
int gww_frontend_set_general(gww_frontend* fe, int on);
/* the host twin (see gww_logmel_host_f32: no HIP call, fork-safe); wave [n_seg] rows of n_samples_in samples, wave_stride
 * apart; out [n_seg, n_mels, n_frames].  The published configuration gives gww_logmel_host_nmel_f32's result bit for bit. */
int gww_logmel_host_cfg_f32(const gww_frontend_cfg* cfg, const float* wave, int n_seg, int n_samples_in, long wave_stride,
                            float* out);

/* The windows of a series: window w covers samples [w * step, w * step + cfg.n_samples) of every row of series
 * [n_rows, n_series] (rows row_stride apart); out [n_windows, n_rows, n_mels, n_frames], or [n_rows, n_windows, ...] with
 * out_rows_major, holds for windows w0 .. w0 + n_windows - 1 what gww_logmel_f32 gives for the materialised window, bit
 * for bit (csrc/logmel_windows.hip).  Frame t of a window is an EDGE frame when t * hop_length < n_fft / 2 or
 * t * hop_length + n_fft / 2 > n_samples (it sees the reflect padding), else INTERIOR.  On the shared route
 * (step % hop_length == 0 and dft_frames_shared < dft_frames_per_window) an interior frame that several windows hold is
 * computed once per call; the per-window route runs the general kernels on the windows in place.
 * gww_logmel_windows_plan: plain C++, no GPU; step < 1 and n_windows < 1 are GWW_ERR_ARG naming the argument. */
#define GWW_WINDOWS_PER_WINDOW 0
#define GWW_WINDOWS_SHARED 1
typedef struct {
    int  route;                  /* GWW_WINDOWS_SHARED / GWW_WINDOWS_PER_WINDOW: what gww_logmel_windows_f32 runs */
    int  edge_lo, edge_hi;       /* edge frames per window at its start and at its end */
    int  interior;               /* n_frames - edge_lo - edge_hi */
    long stream_frames;          /* distinct interior frames of the n_windows windows (per-window count when step is no
                                    multiple of hop_length: nothing is shared then) */
    long dft_frames_shared;      /* stream_frames + n_windows * (edge_lo + edge_hi), per row */
    long dft_frames_per_window;  /* n_windows * n_frames, per row */
    long workspace_bytes;        /* of the chosen route, PER ROW (a multiple of 16): the call needs n_rows times this */
} gww_windows_plan;
int gww_logmel_windows_plan(const gww_frontend_cfg* cfg, int step, int n_windows, gww_windows_plan* out);
/* fe: a handle whose n_samples is the window length; series, out, workspace: device pointers, workspace 16-byte aligned
 * and at least n_rows * plan.workspace_bytes long (its contents before the call do not matter; nothing is allocated per
 * call).  A series too short for window w0 + n_windows - 1 is GWW_ERR_ARG.  n_windows * n_rows up to 2^31 - 1: the launcher
 * loops over the output's outer index where a grid dimension is 16 bits; more than 65535 rows (per-window route, rows
 * major: windows) per call are refused with a message, never truncated.  force_route: -1 the plan's route,
 * GWW_WINDOWS_PER_WINDOW to force the fallback, GWW_WINDOWS_SHARED is refused where the plan does not choose it. */
int gww_logmel_windows_f32(gww_frontend* fe, const float* series, int n_rows, int n_series, long row_stride, int step,
                           int w0, int n_windows, float* out, int out_rows_major, void* workspace, long workspace_bytes,
                           int force_route, void* stream);

/* --------------------------------------------------------------------------
 * Encoder.  Replaces WhisperEncoder.forward as built at
 *   Signal_vs_Noise/src/train.py:227-228,240 ; Glitch_classification/src/train.py:159 ;
 *   MLGWSC-1/train.py:660-663 ; MLGWSC-1/inference.py:408-410
 *   (impl HF:models/whisper/modeling_whisper.py:592-646, layers :379-413,
 *    attention :284-356 / :215-238).
 * -------------------------------------------------------------------------- */
typedef struct {
  int d_model;   /* 384 / 512 / 768 ... multiple of 64 */
  int n_layers;
  int n_heads;   /* d_model / 64 (head_dim is 64 for every Whisper size) */
  int ffn;       /* 4 * d_model */
  int n_mels;    /* 80, or 128 (whisper-large-v3 / -large-v3-turbo) */
  int t_in;      /* 3000 mel frames  -> t_in/2 tokens */
} gww_enc_cfg;

/* fp32 master weights, HF layout ([out,in] linears, [out,in,3] convs). */
typedef struct {
  const float* conv1_w; const float* conv1_b;   /* [d,n_mels,3] [d] */
  const float* conv2_w; const float* conv2_b;   /* [d,d,3]  [d] */
  const float* pos;                             /* [t_in/2, d] embed_positions.weight */
  const float* ln_w; const float* ln_b;         /* final layer_norm */
} gww_enc_globals;

typedef struct {
  const float* ln1_w; const float* ln1_b;       /* self_attn_layer_norm */
  const float* q_w; const float* q_b;           /* [d,d] [d]  (DoRA-merged when adapted) */
  const float* k_w;                             /* [d,d], no bias (HF:modeling_whisper.py:279) */
  const float* v_w; const float* v_b;
  const float* o_w; const float* o_b;           /* out_proj */
  const float* ln2_w; const float* ln2_b;       /* final_layer_norm */
  const float* fc1_w; const float* fc1_b;       /* [ffn,d] [ffn] */
  const float* fc2_w; const float* fc2_b;       /* [d,ffn] [d] */
} gww_enc_layer;

typedef struct gww_encoder gww_encoder;

int gww_encoder_create(const gww_enc_cfg* cfg, gww_encoder** out);
void gww_encoder_destroy(gww_encoder* enc);
/* (Re)pack the weights into the library-owned kernel layouts (bf16 [N,K] panels,
 * q scale folded in, conv taps flattened).  Call again after an optimizer step /
 * DoRA merge.  Asynchronous on `stream`. */
int gww_encoder_set_weights(gww_encoder* enc, const gww_enc_globals* g,
                            const gww_enc_layer* layers, int n_layers, void* stream);
/* Re-pack only the weight groups that changed since the last full gww_encoder_set_weights (an optimizer step on
 * the DoRA parameters touches the q / k / v / out projections only).  globals_or_null: stem / positions / final
 * LayerNorm, NULL if unchanged.  layer_dirty[i]: bit 0 = q, k, v projections + self_attn_layer_norm, bit 1 =
 * out_proj, bit 2 = fc1 + final_layer_norm, bit 3 = fc2; pointers of clean groups are not read. */
int gww_encoder_update_weights(gww_encoder* enc, const gww_enc_globals* globals_or_null,
                               const gww_enc_layer* layers, int n_layers, const unsigned* layer_dirty,
                               void* stream);
/* bytes of caller-owned scratch gww_encoder_forward needs for `batch` segments */
size_t gww_encoder_workspace_bytes(const gww_encoder* enc, int batch, int precision);
/* mel [batch,n_mels,3000] fp32 (== input_features).  Either output may be NULL:
 *   last_hidden [batch, 1500, d] fp32 (== .last_hidden_state)
 *   last_token  [batch, d]       fp32 (== .last_hidden_state[:, -1, :],
 *                Signal_vs_Noise/src/model.py:25-26) */
int gww_encoder_forward(gww_encoder* enc, const float* mel, int batch, int precision,
                        void* workspace, size_t workspace_bytes,
                        float* last_hidden, float* last_token, void* stream);
/* The forward with HF's per-layer outputs (output_hidden_states / output_attentions), inference only.  Same
 * workspace as gww_encoder_forward; last_hidden is bit-identical to what gww_encoder_forward writes (this entry only
 * adds stores and launches; the pooled last-layer shortcut does not apply).  Each slab may be NULL:
 *   hidden_slab [L+1, batch, 1500, d] fp32: [0] stem output + positions, [l] (0 < l < L) the residual stream
 *               leaving layer l-1 (before any LayerNorm), [L] last_hidden_state.  last_hidden may be NULL when
 *               hidden_slab is given: slab layer L is then written directly; otherwise it receives a copy.
 *   attn_slab   [L, batch, n_heads, 1500, 1500] fp32: layer l's softmax(q k^T / 8) before dropout (HF eager
 *               attn_weights), from gww_attention_probs_* on the layer's qkv.
 * The layer strides are those of the full batch (also with the split on: the second half batch is offset). */
int gww_encoder_forward_outputs(gww_encoder* enc, const float* mel, int batch, int precision,
                                void* workspace, size_t workspace_bytes, float* last_hidden,
                                float* hidden_slab, float* attn_slab, void* stream);

/* Dual-stream split (off by default): batches of >= 64 segments are processed as two independent
 * half batches on two library-owned streams forked from / joined to the caller's stream, so the
 * HBM-bound kernels of one half overlap the MFMA-bound kernels of the other on different CUs.
 * Changes gww_encoder_workspace_bytes; results are bit-identical (segments are independent). */
int gww_encoder_set_split(gww_encoder* enc, int on);

/* Constant-tail shortcut of the bf16 inference stem (on by default where it applies: 80 mels, d = 384 / 512 / 768 /
 * 1024, t_in = 3000).  The log-mel of a short segment zero-padded to 30 s is one constant per mel bin behind its live
 * frames; every forward tests that on the device (bitwise, frames 250 .. t_in - 1 of every mel row) and then runs the conv
 * stem on the first 256 frames only, expanding the shared token row under the position table.  Features that do not
 * qualify take the full stem; the choice is made per forward (per half batch with the split on) without a host
 * synchronisation, and last_hidden / last_token are bit-identical either way.  `on` = 0 always runs the full stem.
 * gww_encoder_stem_shortcut_flags reads back what the last forward in `workspace` (same batch and precision) decided:
 * flags[0 .. 1] = 1 (shortcut taken), 0 (full stem) or -1 (does not apply / no second half batch).  It blocks;
 * synchronise the forward's stream first. */
int gww_encoder_set_stem_shortcut(gww_encoder* enc, int on);
int gww_encoder_stem_shortcut_flags(const gww_encoder* enc, int batch, int precision, const void* workspace, int* flags);

/* The residual stream in accumulator order between the fused blocks (on by default where it applies: bf16, d = 384, every
 * block fused with out_proj in front, last_hidden wanted, no per-layer hidden states, more than one layer).  Between two
 * blocks the stream has one reader, the lanes that wrote it, so each 32-row slice of a 128-row panel keeps its 48 KiB of the
 * workspace but holds them as the 48 one-KiB pieces of the wave that owns it; last_hidden / last_token stay in row order and
 * are bit-identical either way.  `on` = 0 keeps row order everywhere.  gww_x_native_offset is the layout itself (host only,
 * no GPU): the byte offset of element (row, col) of an [M, 384] fp32 stream, a row past M clamped to M - 1;
 * gww_x_native_bytes(M) the bytes it spans (whole panels).  (size_t) -1 on a bad argument. */
int gww_encoder_set_x_native(gww_encoder* enc, int on);
size_t gww_x_native_offset(long row, int col, long M);
size_t gww_x_native_bytes(long M);

/* Optional per-kernel timing of the forward (hipEvents on the caller's stream around every
 * launch; ~30 events per forward).  Classes: gww_encoder_trace_classes() entries named by
 * gww_encoder_trace_class_name(i).  gww_encoder_trace_read sums elapsed ms and launch counts per
 * class since the last read (it blocks until the recorded events completed). */
int gww_encoder_trace_enable(gww_encoder* enc, int on);
int gww_encoder_trace_read(gww_encoder* enc, float* ms, int* counts);
int gww_encoder_trace_classes(void);
const char* gww_encoder_trace_class_name(int i);

/* --------------------------------------------------------------------------
 * DoRA.  Replaces peft's DoRA Linear (peft 0.12.0 tuners/lora/dora.py) created at
 *   Signal_vs_Noise/src/train.py:263-264 ; MLGWSC-1/train.py:695-696.
 *   W' = W0 + s B A ; n = ||W'|| per output row ; W_eff = (m/n)[:,None] W'
 * w0 [d_out,d_in], a [r,d_in], b [d_out,r], m [d_out]  ->  w_eff [d_out,d_in],
 * norm_out [d_out] (may be NULL).  All fp32.
 * -------------------------------------------------------------------------- */
int gww_dora_merge_f32(const float* w0, const float* a, const float* b, const float* m,
                       float scaling, int d_out, int d_in, int r,
                       float* w_eff, float* norm_out, void* stream);

/* --------------------------------------------------------------------------
 * conv1 of the stem straight from the HF feature layout (bf16 path, kernel-level entry; the encoder calls the same
 * kernel).  Replaces  nn.functional.gelu(self.conv1(input_features))  of HF:models/whisper/modeling_whisper.py:619-620
 * (reached from Signal_vs_Noise/src/model.py:25, Glitch_classification/src/model.py, MLGWSC-1/inference.py:353-392).
 *   mel [B, 80, T] fp32, conv1_w [d, 80, 3] fp32, conv1_b [d] fp32; w_scratch_bf16: d * 256 bf16 of scratch (packed
 *   taps); c1_out [B, T + 2, d] bf16 token-major, rows 0 and T + 1 of every segment zero (the padding conv2 reads).
 *   d in {384, 512, 768, 1024}, 80 mels only.  The encoder runs other (n_mels, d) pairs -- 128 mels, d = 1280 -- on the
 *   transposition kernel + a GEMM over overlapping rows with K = 3 n_mels padded to a multiple of 64 (256 / 384).
 * -------------------------------------------------------------------------- */
int gww_conv1_gelu_bf16(const float* mel, const float* conv1_w, const float* conv1_b, void* w_scratch_bf16,
                        void* c1_out, int B, int T, int d, void* stream);

/* The same merge for every adapted projection of a model in ONE launch: an optimizer step changes all of them at once
 * (12 modules on whisper-tiny, 36 on whisper-small: Signal_vs_Noise/src/train.py:263-264 targets q, k, v of every
 * layer), and a launch per 384 x 384 matrix is launch-bound.  Items are independent; pointers as above. */
typedef struct {
  const float* w0;      /* [d_out, d_in] frozen base weight */
  const float* a;       /* [r, d_in]     lora_A.weight */
  const float* b;       /* [d_out, r]    lora_B.weight */
  const float* m;       /* [d_out]       lora_magnitude_vector (ones for plain LoRA) */
  float* w_eff;         /* [d_out, d_in] out */
  float* norm_out;      /* [d_out] out, may be NULL */
  float scaling;        /* lora_alpha / r */
  int d_out, d_in, r;
} gww_dora_merge_item;
int gww_dora_merge_batch_f32(const gww_dora_merge_item* items, int n, void* stream);

/* --------------------------------------------------------------------------
 * DoRA training step (bf16).  Replaces loss.backward() through the frozen encoder with DoRA
 * adapters (Signal_vs_Noise/src/train.py:163-168 with the model of :263-269): the forward keeps
 * the activations in a caller-owned arena, the backward returns the A / B / magnitude gradients
 * of the listed projections (peft 0.12.0 dora.py semantics: the weight norm is detached) and,
 * optionally, the gradient w.r.t. the conv-stem output.  The MLP head, the loss and the
 * optimizer stay in torch on the GPU.
 * -------------------------------------------------------------------------- */
typedef struct {
  int layer;            /* encoder layer index */
  int proj;             /* 0 q_proj, 1 k_proj, 2 v_proj, 3 out_proj, 4 fc1 [ffn, d], 5 fc2 [d, ffn] */
  int r;                /* LoRA rank, 1..64 */
  float scaling;        /* lora_alpha / r */
  const float* A;       /* [r, d_in]   lora_A.weight */
  const float* B;       /* [d_out, r]  lora_B.weight */
  const float* mag;     /* [d_out]     lora_magnitude_vector */
  const float* nrm;     /* [d_out]     ||W0 + s B A|| rows (norm_out of gww_dora_merge_f32) */
  float* dA;            /* gradients, ACCUMULATED into: zero them once per step */
  float* dB;
  float* dm;
} gww_dora_target;
/* The three backward entry points below check a target array the same way and in the same order: first the targets' own
 * fields (rank 1..64, none of the seven pointers NULL) and that no (layer, proj) is named twice -- nothing of the
 * handle is read for these --, then the layer / proj range against the handle, then the workspace and arena sizes.
 * Two targets with the same (layer, proj) are refused with GWW_ERR_ARG (the message names both indices); with several
 * faults in one call the first in that order is the one reported. */

size_t gww_train_saved_bytes(const gww_encoder* enc, int batch);
size_t gww_train_workspace_bytes(const gww_encoder* enc, int batch);
/* Workspace of a step with fc1 / fc2 targets or ranks other than 8 (at most max_r): gww_train_workspace_bytes plus the
 * adapter-gradient scratch (gww_adapter_grads_scratch_bytes of the largest target shape).  With a smaller workspace the
 * backward allocates that scratch stream-ordered on every such target. */
size_t gww_train_workspace_bytes_adapters(const gww_encoder* enc, int batch, int max_r);
int gww_encoder_train_forward(gww_encoder* enc, const float* mel, int batch, void* workspace,
                              size_t workspace_bytes, void* saved, size_t saved_bytes,
                              float* last_hidden, int pooled, void* stream);
int gww_encoder_train_backward(gww_encoder* enc, int batch, void* workspace, size_t workspace_bytes,
                               const void* saved, size_t saved_bytes, const float* d_last_hidden,
                               const gww_dora_target* targets, int n_targets, float* d_x0, float* d_mel,
                               int pooled, void* stream);
/* pooled != 0: the caller only uses token T-1 of the output, as every classifier of the reference does
 * (Signal_vs_Noise/src/model.py:25-26 `last_hidden_state[:, -1, :]`).  last_hidden and d_last_hidden are then
 * [batch, d]; everything above the last layer's attention (out_proj, LN2, fc1, GELU, fc2, final LN and their
 * backward) runs on those `batch` rows instead of batch*T, and the attention backward skips the query tiles
 * without gradient.  The forward and the backward of one step must use the same `pooled`. */
/* d_x0 (optional): fp32 [batch*T, d] gradient w.r.t. the conv-stem output.  d_mel (optional): fp32
 * [batch, n_mels, t_in] gradient w.r.t. the input features through the conv stem -- the encoder call is
 * differentiable w.r.t. its input, as MLGWSC-1/train.py:494-504 (trainable Q-adapter in front of the frozen
 * encoder) requires. */
/* workspace / saved between the two calls of a step: `saved` carries the activations and goes to the backward unmodified.
 * `workspace` is scratch -- its contents need not survive from the forward to the backward -- EXCEPT when the backward is
 * asked for d_mel or (gww_encoder_train_backward_full) for a conv1 / conv2 gradient: those are formed from the stem's
 * transposed input and conv1 output, which the forward leaves at the front of ITS workspace and does not copy into
 * `saved`.  Such a backward must be handed the forward's workspace with those bytes untouched (the Python shim keeps the
 * forward's workspace on the autograd node for every step).  The same holds for the fp32 twins below. */

/* --------------------------------------------------------------------------
 * Full fine-tuning (bf16): the same backward, plus the gradients of the base parameters
 * (Signal_vs_Noise/src/train.py:243-247 `--method full_finetune`, Glitch_classification/src/
 * train_full_finetune.py).  Every pointer is an fp32 buffer in the parameter's HF layout
 * (conv weights [out, in, 3]); NULL = gradient not wanted.  Gradients are ACCUMULATED into.
 * -------------------------------------------------------------------------- */
typedef struct {
  float* ln1_w; float* ln1_b;
  float* q_w; float* q_b;
  float* k_w;
  float* v_w; float* v_b;
  float* o_w; float* o_b;
  float* ln2_w; float* ln2_b;
  float* fc1_w; float* fc1_b;
  float* fc2_w; float* fc2_b;
} gww_enc_layer_grads;
typedef struct {
  float* conv1_w; float* conv1_b;
  float* conv2_w; float* conv2_b;
  float* pos;
  float* ln_w; float* ln_b;
  const gww_enc_layer_grads* layers;   /* n_layers entries, or NULL: no per-layer gradient */
} gww_enc_grads;
/* workspace of a backward with base gradients (>= gww_train_workspace_bytes; the saved arena is unchanged) */
size_t gww_train_workspace_bytes_full(const gww_encoder* enc, int batch);
/* gww_encoder_train_backward + base-parameter gradients (grads may be NULL: then identical to it).  The workspace must
 * hold gww_train_workspace_bytes_full bytes whenever grads requests anything. */
int gww_encoder_train_backward_full(gww_encoder* enc, int batch, void* workspace, size_t workspace_bytes,
                                    const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                    const gww_dora_target* targets, int n_targets, float* d_x0, float* d_mel,
                                    int pooled, const gww_enc_grads* grads, void* stream);
/* The same step in exact fp32 (precision="fp32": every saved activation fp32, every contraction on the fp32 MFMA; the
 * per-op path at every width).  Same arguments and contract as gww_encoder_train_forward / _backward, on an arena and a
 * workspace sized by the two queries below (the workspace includes the adapter-gradient scratch for ranks up to 64).
 * LN1 / LN2 outputs and the fc1 pre-activation are recomputed in the backward, not saved.  No base-parameter gradients
 * (full fine-tuning stays bf16).  workspace and saved 256-byte aligned, mel and d_last_hidden 16-byte aligned. */
size_t gww_train_saved_bytes_f32(const gww_encoder* enc, int batch);
size_t gww_train_workspace_bytes_f32(const gww_encoder* enc, int batch);
int gww_encoder_train_forward_f32(gww_encoder* enc, const float* mel, int batch, void* workspace,
                                  size_t workspace_bytes, void* saved, size_t saved_bytes,
                                  float* last_hidden, int pooled, void* stream);
int gww_encoder_train_backward_f32(gww_encoder* enc, int batch, void* workspace, size_t workspace_bytes,
                                   const void* saved, size_t saved_bytes, const float* d_last_hidden,
                                   const gww_dora_target* targets, int n_targets, float* d_x0, float* d_mel,
                                   int pooled, void* stream);

/* Weight-gradient GEMM (csrc/wgrad.hip): dW[N,K] += alpha * sum_m dY[m,n] X[m,k], db[N] += alpha * sum_m dY[m,n]
 * (db may be NULL).  dY [M, ldy] and X [M, ldx] bf16 row-major, 16-byte aligned; dW, db fp32.  The reduction over M
 * is split across workgroups into fp32 partial slabs summed in a fixed order: two identical calls give identical
 * bits.  N % 64 == 0, K % 16 == 0, ldy and ldx multiples of 8; X may be a strided (overlapping) view, e.g. the
 * im2col view of a conv input (ldx < K).  workspace: gww_gemm_wgrad_workspace_bytes(M, N, K) bytes. */
size_t gww_gemm_wgrad_workspace_bytes(long M, int N, int K);
int gww_gemm_wgrad_bf16(const void* dY, long ldy, const void* X, long ldx, long M, int N, int K, float alpha,
                        float* dW, float* db_or_null, void* workspace, size_t ws_bytes, void* stream);
/* LayerNorm gain / bias gradients: dgamma += sum_m dy * xhat, dbeta += sum_m dy (x fp32 [M, d], dy fp32 or bf16;
 * eps 1e-5; either output may be NULL; fixed-order reduction).  d % 128 == 0, d <= 1280. */
size_t gww_layernorm_param_grads_workspace_bytes(long M, int d);
int gww_layernorm_param_grads(const float* x, const void* dy, int dy_is_f32, long M, int d, float* dgamma,
                              float* dbeta, void* workspace, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Kernel-level entry points (used by the parity tests and by the Python
 * autograd shim; same conventions).
 * -------------------------------------------------------------------------- */
/* y[M,d] (bf16 if out_bf16 else fp32) = LayerNorm(x[M,d] fp32) * w + b, eps 1e-5 */
int gww_layernorm(const float* x, const float* w, const float* b, void* y, int out_bf16,
                  long M, int d, void* stream);
/* C[M,N] = A[M,K] @ W[N,K]^T + bias ; epilogue: 0 none, 1 exact GELU, 2 += resid (fp32 out).
 * bf16 variant: A, W bf16; C bf16 (epilogue 0/1) or fp32 (epilogue 2).
 * f32 variant : everything fp32. */
int gww_gemm_bf16(const void* A, const void* W, const float* bias, const float* resid, void* C,
                  long M, int N, int K, int epilogue, void* stream);
/* The 256 x 256 x 64 kernel of the wide encoders (csrc/gemm_v4.hip; what gww_gemm_bf16 picks for N % 256 == 0,
 * N <= 3072, K % 128 == 0, M % 256 == 0) with the column split of its work items given explicitly: n_split = 0 is the
 * automatic choice, n_split > 0 must divide N / 256.  Results do not depend on n_split bit for bit (tests). */
int gww_gemm_bf16_v4_split(const void* A, const void* W, const float* bias, const float* resid, void* C,
                           long M, int N, int K, int epilogue, int n_split, void* stream);
/* A-stationary bf16 GEMM for K in {256, 384, 512}, N % 128 == 0 (QKV / fc1 / out_proj at
 * whisper-tiny/base): C = epi(f(A) @ W^T + bias), C bf16, epilogue 0 (bias), 1 (GELU) or 5 (GELU backward).
 *   ln_u == NULL : A is bf16 [M,K], W the plain bf16 [N,K] panel.
 *   ln_u != NULL : A is the fp32 residual stream x [M,K].  In ONE pass the kernel forms
 *                  x_new = x + delta (delta bf16 [M,K] or NULL), writes it to x_out (fp32 [M,K],
 *                  may be NULL, must not alias A) and applies LayerNorm (eps 1e-5,
 *                  HF:modeling_whisper.py:392,402) algebraically: W must be the gain-folded
 *                  panel and ln_u / ln_cb the vectors produced by gww_ln_fold_weights; `bias`
 *                  is ignored (it is inside ln_cb).
 *   epilogue 5   : the backward of fc1's GELU, C = delta * gelu'(A @ W^T + bias) (each factor rounded to
 *                  bf16): A bf16 [M,K], `delta` the incoming gradient, bf16 [M,N] row-major, x_out and ln_u
 *                  NULL.  C may alias delta (in place); delta rows >= M are never read.
 * Rows of C must be ALLOCATED up to the next multiple of 256: whole 256-row panels are stored
 * unconditionally (rows >= M are scratch). */
int gww_gemm_astat_bf16(const void* A, const void* delta, float* x_out, const float* ln_u,
                        const float* ln_cb, const void* W, const float* bias, void* C, long M, int N,
                        int K, int epilogue, void* stream);
/* Fold a LayerNorm into the Linear that follows it: w fp32 [N,K], ln_w / ln_b [K], bias [N] or NULL
 *   w_folded[n][k] = bf16(scale * ln_w[k] * w[n][k]),   u[n] = sum_k w_folded[n][k],
 *   cb[n] = scale * (bias[n] + sum_k ln_b[k] * w[n][k]). */
int gww_ln_fold_weights(const float* w, const float* ln_w, const float* ln_b, const float* bias, float scale,
                        int N, int K, void* w_folded_bf16, float* u, float* cb, void* stream);
/* Full-N bf16 GEMM for the long-K, N = d contractions (fc2, conv2): one workgroup owns complete
 * 128-row x N output panels, so A is read from HBM once.  N in {384, 512}, K % 32 == 0, C bf16
 * [M,N] with rows allocated up to the next multiple of 128; epilogue 0 (bias) or 1 (GELU). */
int gww_gemm_fulln_bf16(const void* A, const void* W, const float* bias, void* C, long M, int N, int K,
                        int epilogue, void* stream);
/* Fused MLP block at d_model = 384 (HF:modeling_whisper.py:401-407, residual add deferred to the consumer):
 *   x_out = x + delta;   C = bf16( fc2( gelu( fc1( LayerNorm(x_out) ) ) ) + b2 )
 * x fp32 [M,384], delta bf16 [M,384], x_out fp32 [M,384] (must not alias x); ln_u / ln_cb [F] from
 * gww_ln_fold_weights of fc1; Wt = gww_mlp_pack_bf16 stream; C bf16 with rows allocated up to the next multiple of
 * 128.  F % 128 == 0, F <= 1536.  The [M,F] activation never leaves the CU; GELU is x * sigmoid(odd quintic),
 * |err| <= 2.6e-5 against the erf form.
 * With qkv_out != NULL the NEXT layer's self_attn_layer_norm + q / k / v projection (HF:modeling_whisper.py:392,
 * 303-318) is appended: x_next = x + delta + bf16(C) (the residual stream entering the next layer) is then written
 * BACK OVER x (every 128-row panel has finished reading its rows of x by then; x_out keeps x + delta, the block's
 * intermediate stream -- the kernel's second residual seam must not run in place), C is not written, and qkv_out bf16 [M (rows padded to 128), NQ] = LayerNorm(x_next) Wqkv'^T + cb with
 * qkv_u / qkv_cb from gww_ln_fold_weights of that projection (its panel appended to the stream by
 * gww_mlp_pack_bf16).  NQ % 128 == 0, NQ <= 1536. */
int gww_mlp_fused_bf16(float* x, const void* delta, float* x_out, const float* ln_u, const float* ln_cb,
                       const void* Wt, const float* b2, void* C, long M, int d, int F, const float* qkv_u,
                       const float* qkv_cb, void* qkv_out, int NQ, void* stream);
/* Pre-tile the weights of gww_mlp_fused_bf16: w1_folded bf16 [F,384] (gww_ln_fold_weights), w2 bf16 [384,F],
 * optionally the next layer's folded q / k / v panel bf16 [NQ,384] -> out bf16, 2*384*F (+ NQ*384) elements, as the
 * sequence of swizzled 16-KiB LDS images the kernel streams. */
int gww_mlp_pack_bf16(const void* w1_folded, const void* w2, const void* wqkv_folded_or_null, void* out, int d, int F,
                      int NQ, void* stream);
/* The attention output projection fused IN FRONT of gww_mlp_fused_bf16 (HF:modeling_whisper.py:353-356, 396-398): ctx bf16
 * [M,384] is the attention context, x_out = x + bf16(ctx W_o^T + bo) (the value the stand-alone out_proj + deferred
 * residual add produce), then the block as gww_mlp_fused_bf16 describes, incl. the optional q / k / v tail.  Wt =
 * gww_mlp_pack_op_bf16: the 18 tiles of W_o bf16 [384,384] in front of the gww_mlp_pack_bf16 stream. */
int gww_attn_out_mlp_fused_bf16(float* x, const void* ctx, const float* bo, float* x_out, const float* ln_u,
                                const float* ln_cb, const void* Wt, const float* b2, void* C, long M, int d, int F,
                                const float* qkv_u, const float* qkv_cb, void* qkv_out, int NQ, void* stream);
/* ... and, for the LAST layer, with the encoder's final LayerNorm (HF:modeling_whisper.py:642) as the epilogue:
 * y fp32 [M,384] = LayerNorm(x_mid + bf16(mlp(LayerNorm2(x_mid)) + b2); lnf_w, lnf_b), x_mid = x + bf16(ctx W_o^T + bo)
 * (x_mid fp32 [M,384] is written too; it aliases neither x nor y).  Wt = gww_mlp_pack_op_bf16 without a q / k / v panel. */
int gww_attn_out_mlp_final_bf16(const float* x, const void* ctx, const float* bo, float* x_mid, const float* ln_u,
                                const float* ln_cb, const void* Wt, const float* b2, const float* lnf_w, const float* lnf_b,
                                float* y, long M, int d, int F, void* stream);
int gww_mlp_pack_op_bf16(const void* wo, const void* w1_folded, const void* w2, const void* wqkv_folded_or_null, void* out,
                         int d, int F, int NQ, void* stream);
/* self_attn_layer_norm + q / k / v projection of a residual stream with no pending delta (layer 0, fed by the conv stem;
 * HF:modeling_whisper.py:392, 303-318) at d_model = 384, on the panel prologue and the q / k / v tail of
 * gww_mlp_fused_bf16:  qkv_out bf16 [M (rows padded to 128), NQ] = LayerNorm(x) Wqkv'^T + cb.  x fp32 [M,384] is only read;
 * qkv_u / qkv_cb from gww_ln_fold_weights; Wt = gww_mlp_pack_bf16(NULL, NULL, wqkv_folded, ., 384, 0, NQ).
 * NQ % 128 == 0, NQ <= 1536. */
int gww_lnqkv_fused_bf16(const float* x, const float* qkv_u, const float* qkv_cb, const void* Wt, void* qkv_out, long M,
                         int d, int NQ, void* stream);
/* Layer 0 behind the compact conv stem (the constant tail of a padded log-mel, gww_encoder_set_stem_shortcut).  The stem leaves
 * xs fp32 [B,Tt,384] (compact conv2 output), tr fp32 [B,384] and the device flag; with pos fp32 [T,384] they describe the residual
 * stream x fp32 [B,T,384]:  x[b,j] = xs[b,j] for j <= Tt-3,  fma(xs[b,Tt-2], tr[b], pos[j]) for Tt-2 <= j <= T-2,  xs[b,Tt-1] for
 * j = T-1.  gww_stem_fill_f32 writes that stream to x (a no-op where *flag == 0).  The two x0 forms are gww_lnqkv_fused_bf16 and
 * gww_attn_out_mlp_fused_bf16 (with the q / k / v tail; x_new is not kept) on that stream WITHOUT it being written first: where
 * *flag == 1 they form their 128-row panels from xs / tr / pos in registers and never read x; where *flag == 0 they read x.
 * Results are bitwise those of the fill followed by the plain entry.  The block writes x_next to x.  M = B T, T >= 128. */
int gww_stem_fill_f32(const float* xs, const float* tr, const float* pos, const int* flag, float* x, int B, int T, int Tt, int d,
                      void* stream);
int gww_lnqkv_fused_x0_bf16(const float* xs, const float* tr, const float* pos, const int* flag, const float* x, int T, int Tt,
                            const float* qkv_u, const float* qkv_cb, const void* Wt, void* qkv_out, long M, int d, int NQ,
                            void* stream);
int gww_attn_out_mlp_fused_x0_bf16(const float* xs, const float* tr, const float* pos, const int* flag, float* x, int T, int Tt,
                                   const void* ctx, const float* bo, const float* ln_u, const float* ln_cb, const void* Wt,
                                   const float* b2, long M, int d, int F, const float* qkv_u, const float* qkv_cb, void* qkv_out,
                                   int NQ, void* stream);
/* Q-transform front end #2 (ml4gw QScan as used by MLGWSC-1/train.py:117-122,135-154; PARITY UNPINNED: ml4gw is not
 * vendored, pinned or installed -- the kernels follow oracle/qscan.py).  The host builds the static tiling once
 * (gw_whisper_amd/qscan.py): rows = int [n_rows][6] (plane, ntiles, windowsize, first data index, energy offset,
 * window offset) plane by plane in frequency order; order = row indices sorted by ntiles; class_ranges_host = [first,
 * last) positions in `order` for ntiles 128, 256, 512, 1024, 2048; window = the bisquare windows back to back.
 * fseries: fp32 [B, ld] (re, im) forward-normalised one-sided spectrum with the positive frequencies doubled (one
 * gww_gemm_f32 against the real-DFT matrix).  energy: fp32 [B, e_total] median-normalised tile energies; plane_max:
 * uint [n_planes] (float bits of each plane's largest energy over the whole batch; zeroed by the call). */
int gww_qscan_energy_f32(const float* fseries, int ld, int B, const int* rows, const int* order,
                         const int* class_ranges_host, const float* window, float* energy, long e_total,
                         unsigned int* plane_max, int n_planes, void* stream);
/* Select the plane with the largest energy over the batch (on the device) and resample it to out fp32 [B, F, T]
 * with PyTorch's bicubic rules (time per row, then frequency).  plane_rows: device int [n_planes][2] = first row,
 * row count.  chosen (optional): device int receiving the selected plane. */
int gww_qscan_interp_f32(const float* energy, long e_total, const int* rows, const int* plane_rows, int n_planes,
                         const unsigned int* plane_max, int B, int F, int T, float* out, int* chosen, void* stream);
/* Tail of the reference's QTransformAdapter (MLGWSC-1/train.py:146-153, inference.py:345-350) as ONE kernel:
 * AdaptiveAvgPool2d((F, T)) of the adapter CNN's output y fp32 [B, Hin, Win], then scale * y + bias, then
 * * film_gamma[i] + film_beta[i]; the result goes straight into the stacked [B, D, F, T] feature tensor: element
 * (b, f, t) at out[b * out_batch_stride + f * T + t] (the caller offsets `out` to detector i).  scale / bias / gamma_i /
 * beta_i are device scalars (no host sync).  T % 4 == 0, Win <= 4096. */
int gww_qadapter_tail_f32(const float* y, int B, int Hin, int Win, const float* scale, const float* bias,
                          const float* gamma_i, const float* beta_i, float* out, long out_batch_stride, int F, int T,
                          void* stream);
/* The adapter's small CNN (`self.freq_adapter`: Conv2d(1,c1,3,p1) ReLU MaxPool2d(2) Conv2d(c1,c2,3,p1) ReLU MaxPool2d(2)
 * Conv2d(c2,c3,3,p1) ReLU Conv2d(c3,1,1); MLGWSC-1/train.py:117-122 with c = 32 / 64 / 128, MLGWSC-1/inference.py:320-330
 * with c = 16 / 32 / 64) as three HIP launches: a VALU kernel for the one-channel input layer and an implicit-GEMM MFMA
 * kernel (bf16-pair operands, fp32 accumulation: about 1e-5 relative to the fp32 the reference computes in) with ReLU /
 * max-pool resp. ReLU + the 1 x 1 convolution in its epilogue.
 *   gww_qadapter_cnn_pack_f32: the torch parameters (device fp32: w1 [c1,1,3,3] b1 [c1] w2 [c2,c1,3,3] b2 [c2]
 *     w3 [c3,c2,3,3] b3 [c3] w4 [1,c3,1,1] b4 [1]) -> `packed` (gww_qadapter_cnn_packed_bytes bytes; 0 = channel widths
 *     the reference does not have)
 *   gww_qadapter_cnn_forward_f32: qspec fp32 [B, H, W] (the Q-scan map, H % 32 == 0, W % 128 == 0) -> y fp32
 *     [B, H/4, W/4] (the input of gww_qadapter_tail_f32); workspace: gww_qadapter_cnn_workspace_bytes, caller-owned */
size_t gww_qadapter_cnn_packed_bytes(int c1, int c2, int c3);
size_t gww_qadapter_cnn_workspace_bytes(int B, int H, int W, int c1, int c2);
int gww_qadapter_cnn_pack_f32(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                              const float* b3, const float* w4, const float* b4, int c1, int c2, int c3, void* packed,
                              void* stream);
int gww_qadapter_cnn_forward_f32(const float* qspec, int B, int H, int W, const void* packed, int c1, int c2, int c3,
                                 void* workspace, size_t workspace_bytes, float* y, void* stream);
/* The CNN's BACKWARD (the adapter is trained through the frozen encoder, MLGWSC-1/train.py:494-504; replaces torch
 * autograd through nn.Conv2d / nn.MaxPool2d, i.e. MIOpen): dy fp32 [B, H/4, W/4] = the gradient of
 * gww_qadapter_cnn_forward_f32's y -> the gradients of the eight torch parameters in their torch shapes (fp32, overwritten):
 * dw1 [c1,1,3,3] db1 [c1] dw2 [c2,c1,3,3] db2 [c2] dw3 [c3,c2,3,3] db3 [c3] dw4 [1,c3,1,1] db4 [1].  `packed` is the
 * forward's blob, w2 / w3 the raw fp32 parameters (packed here, transposed, for the data gradients).  Nothing was saved by
 * the forward: the activations are recomputed.  The Q-scan input needs no gradient (the reference computes it under
 * no_grad).  W <= 512. */
size_t gww_qadapter_cnn_backward_workspace_bytes(int B, int H, int W, int c1, int c2, int c3);
int gww_qadapter_cnn_backward_f32(const float* qspec, const float* dy, int B, int H, int W, const void* packed,
                                  const float* w2, const float* w3, int c1, int c2, int c3, void* workspace,
                                  size_t workspace_bytes, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                  float* db3, float* dw4, float* db4, void* stream);
/* Whitening of the search pipeline's strain (MLGWSC-1/inference.py:56-137 -> PyCBC 2.4.0 TimeSeries.psd / welch /
 * inverse_spectrum_truncation; PARITY UNPINNED -- PyCBC is not installed, the kernels follow oracle/whiten.py).
 * gww_welch_power_f32: |rDFT|^2 * scale of the windowed Welch segments from their (re, im) rows (a gww_gemm_f32 against
 * the windowed real-DFT matrix), DC / Nyquist halved.  gww_column_median_f32: numpy.median over the segments per
 * frequency bin (values >= 0).  gww_fir_f32: the inverse-spectrum-truncated whitening filter applied as a FIR in the
 * time domain, out[d][n] = sum_u g[d][u] xp[d][n + u] (xp circularly padded by the caller, taps zero-padded to a
 * multiple of 4).  gww_fir_f64: the same with fp64 samples, taps and sums and one rounding to the fp32 output (what
 * whitening uses: detector strain holds its in-band content at about 1e-5 of the sample peak); taps4 <= 8192, xp_stride
 * even. */
int gww_welch_power_f32(const float* spec, long ld, long n_seg, int n_bins, float scale, float* power, void* stream);
int gww_column_median_f32(const float* power, long n_seg, int n_bins, float* median, void* stream);
int gww_fir_f32(const float* xp, long xp_stride, const float* g, int taps4, int D, float* out, long out_stride,
                long n_out, void* stream);
int gww_fir_f64(const double* xp, long xp_stride, const double* g, int taps4, int D, float* out, long out_stride,
                long n_out, void* stream);
/* Trigger clustering on the device (MLGWSC-1/inference.py:140-166 `get_clusters` behind :484-487): windows whose score
 * exceeds trigger_threshold, in time order, join the running cluster unless they lie more than cluster_threshold seconds
 * behind the previous trigger; per cluster the time and value of its first maximum.  times fp64 [n] (the reference's
 * stamps), scores fp32 [n]; out_times fp64 / out_vals fp32 [max_clusters], *out_count = clusters found (may exceed
 * max_clusters: only the first max_clusters are stored).  One launch per trigger list (segment). */
int gww_cluster_triggers_f64(const double* times, const float* scores, long n, float trigger_threshold,
                             double cluster_threshold, double* out_times, float* out_vals, int* out_count,
                             int max_clusters, void* stream);
/* ---- search background from time slides (csrc/timeslide.hip) ----
 * The detectors of the search model only meet in its head, whose first Linear splits over the concatenated tokens.
 * P fp32 [D, N, 512]: the first layer's partial products per detector and window (P[g] = tok_g W1_g^T, the bias folded
 * into detector 0); w2 [256, 512], w3 [128, 256], w4 [64, 128], w5 [C, 64] and their biases: layers 2..5 of the head;
 * offsets int64 [S] on the device, each in [0, N) (the caller checks them before upload; the kernel reduces whatever
 * arrives modulo N, so no index leaves P).  scores fp32 [S, N], every element written:
 *   scores[s][i] = f(w5 relu(w4 relu(w3 relu(w2 relu(sum_g P[g][(i + g offsets[s]) mod N]) + b2) + b3) + b4) + b5)
 * with f(z) = z[0] (mode 0, the head without its Softmax) or softmax(z)[0] (mode 1, C >= 2; fp64 on the fp32 logits,
 * rounded once).  Detector 0 is never moved.  One launch, one workgroup per 16 consecutive windows of one slide; exact
 * fp32 (v_mfma_f32_16x16x4_f32 chains), no atomics: identical calls give identical bits, and a slide's row does not
 * depend on the other offsets of the launch.  N 1..2^31-1, D 2..4, S 1..65535, C 1..64; P, the weights and b2..b4
 * 16-byte aligned. */
int gww_slide_scores_f32(const float* P, const float* w2, const float* b2, const float* w3, const float* b3,
                         const float* w4, const float* b4, const float* w5, const float* b5, const long long* offsets,
                         long N, int D, int S, int C, int mode, float* scores, void* stream);
/* gww_cluster_triggers_f64 over every row of scores [S, N] in one launch, one wave per slide; times fp64 [N] is shared.
 * out_times fp64 / out_vals fp32 [S, max_clusters], out_count int32 [S] = the clusters found in each slide (may exceed
 * max_clusters: only the first max_clusters of a slide are stored, so the caller sees an overflow).  Slides never share
 * a cluster.  N 1..2^31-1, S 1..65535. */
int gww_cluster_slides_f64(const double* times, const float* scores, long N, int S, float trigger_threshold,
                           double cluster_threshold, double* out_times, float* out_vals, int* out_count,
                           int max_clusters, void* stream);
int gww_gemm_f32(const float* A, const float* W, const float* bias, const float* resid, float* C,
                 long M, int N, int K, int epilogue, void* stream);
/* softmax(q k^T) v per head, q pre-scaled; qkv [B,T,3*d] (q|k|v), ctx [B,T,d]; head_dim 64 */
int gww_attention_bf16(const void* qkv, void* ctx, int B, int T, int n_heads, void* stream);
int gww_attention_f32(const float* qkv, float* ctx, int B, int T, int n_heads, void* stream);
/* the kernel of the encoder's bf16 paths (k_attention_dma_bf16): q must be in log2 units, i.e. projected with
 * log2(e) / 8 instead of 1 / 8 (gww_encoder_set_weights folds that into every packed bf16 q panel); the running
 * reference enters the score accumulators through one extra MFMA, K / V tiles by LDS-DMA; lse optional, natural log */
int gww_attention_log2q_bf16(const void* qkv, void* ctx, float* lse_or_null, int B, int T, int n_heads, void* stream);
/* attention backward: dqkv [B,T,3d] from qkv, ctx (forward output), dctx and the forward's lse [B,H,T]
 * (gww_attention_lse_bf16 below); d_scratch: B * H * (T + ceil(T / 64)) fp32 words (row dots + live-tile flags:
 * query tiles whose dctx rows are all zero are skipped, which is most of them under last-token pooling) */
int gww_attention_bwd_bf16(const void* qkv, const void* ctx, const void* dctx, const float* lse,
                           float* d_scratch, void* dqkv, int B, int T, int n_heads, void* stream);
/* the same for a q section in log2 units (projected with log2(e) / 8, what gww_attention_log2q_bf16 takes): the q
 * section of dqkv is the gradient with respect to that stored q */
int gww_attention_bwd_log2q_bf16(const void* qkv, const void* ctx, const void* dctx, const float* lse,
                                 float* d_scratch, void* dqkv, int B, int T, int n_heads, void* stream);
/* forward attention that also returns the row log-sum-exp lse [B,H,T] */
int gww_attention_lse_bf16(const void* qkv, void* ctx, float* lse, int B, int T, int n_heads, void* stream);
/* fp32 twins (exact fp32 MFMA): the forward with lse -- ctx bit-identical to gww_attention_f32's -- and the backward.
 * qkv / ctx / dctx / dqkv fp32 with the layouts above, q as stored (pre-scaled by 1/8) and its gradient with respect to
 * that stored q; d_scratch: gww_attention_bwd_f32_scratch_bytes (row dots + live flags of 32-row query tiles: tiles
 * whose dctx rows are all zero are skipped).  No atomics: two identical calls give identical bits. */
int gww_attention_lse_f32(const float* qkv, float* ctx, float* lse, int B, int T, int n_heads, void* stream);
size_t gww_attention_bwd_f32_scratch_bytes(int B, int T, int n_heads);
int gww_attention_bwd_f32(const float* qkv, const float* ctx, const float* dctx, const float* lse,
                          float* d_scratch, float* dqkv, int B, int T, int n_heads, void* stream);
/* attention probabilities P[b,h,i,j] = softmax_j(q_i . k_j), fp32 [B, n_heads, T, T] (HF eager attn_weights) from
 * qkv [B*T, 3d] as the attention kernels read it (q pre-scaled by 1/8; bf16: times log2(e) when q_log2 != 0, the
 * encoder's packed bf16 q panels).  Scores by MFMA on the given operands (bf16: 32x32x16 bf16, fp32: 32x32x2 f32);
 * each workgroup takes the row max / sum over all keys, then recomputes and stores the normalised rows.  T % 4 == 0.
 * B == 0 is a no-op that accepts NULL buffers (after the shape checks). */
int gww_attention_probs_bf16(const void* qkv, int q_log2, float* probs, int B, int T, int n_heads, void* stream);
int gww_attention_probs_f32(const float* qkv, float* probs, int B, int T, int n_heads, void* stream);
/* LayerNorm backward: dx (+)= dLN/dx . dy   (dy fp32 or bf16; optional bf16 copy of the result) */
int gww_layernorm_bwd(const float* x, const float* gamma, const void* dy, int dy_is_f32, float* dx,
                      int accumulate, void* dx_bf16, long M, int d, void* stream);
/* bf16 GELU: out = gelu(z) (dgelu == NULL) or out = dgelu * gelu'(z); n % 8 == 0 */
int gww_gelu_bf16(const void* z, const void* dgelu_or_null, void* out, long n, void* stream);
/* DoRA parameter gradients of one [d,d] projection (see train_ops.hip): X [M,d] with row stride ldx, dY / Y
 * [M,d] sections with row stride ldy (e.g. one of the q / k / v column blocks of the packed [M,3d] qkv / dqkv),
 * bias_st in stored units, yscale = dy_true / dy_stored.  d in {128, 384, 512, 768, 1024, 1280}, r = 8 (other ranks
 * 1..64 go to gww_adapter_grads' kernel, its scratch allocated stream-ordered); gradients are accumulated. */
int gww_dora_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                   float yscale, float scaling, const float* A, const float* B, const float* mag,
                   const float* nrm, float* dA, float* dB, float* dm, long M, int d, int r, void* stream);
/* The same for np (1..3) projections that read the SAME X -- q, k and v of a layer (peft 0.12.0 dora.py; targets of
 * Signal_vs_Noise/src/train.py:230-237) -- in one pass on the matrix cores (dora_grads.hip); d in {384, 512}, r = 8.
 * Projection p reads dY / Y at column col_off[p] of rows with stride ldy; all arrays have np entries (host memory,
 * device pointers inside).  Gradients are accumulated. */
/* Adapter gradients of one adapted linear layer of any shape the encoder has -- [d, d], fc1 [4d, d], fc2 [d, 4d] -- and
 * rank 1..64 (dora_grads.hip, on the matrix cores): X [M, d_in] (row stride ldx), dY / Y [M, d_out] (row stride ldy),
 * bias_st [d_out], A [r, d_in], B [d_out, r], mag / nrm [d_out]; otherwise the contract of gww_dora_grads (plain LoRA:
 * mag = nrm = 1).  d_in, d_out multiples of 128; r > 64 is an error.  Partial sums go through per-workgroup slabs
 * summed in a fixed order: two identical calls give identical bits.  scratch (optional):
 * gww_adapter_grads_scratch_bytes(M, d_in, d_out, r) bytes of device memory, else it is allocated stream-ordered. */
size_t gww_adapter_grads_scratch_bytes(long M, int d_in, int d_out, int r);
int gww_adapter_grads(const void* X, long ldx, const void* dY, const void* Y, long ldy, const float* bias_st,
                      float yscale, float scaling, const float* A, const float* B, const float* mag, const float* nrm,
                      float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r, void* scratch,
                      size_t scratch_bytes, void* stream);
/* gww_adapter_grads in exact fp32 (train_f32.hip): X, dY, Y fp32 with the same strides and contract; d_in, d_out
 * multiples of 32, ranks 1..64, row strides multiples of 4.  u = x A^T and v = (g dy) B on the fp32 MFMA, dA / dB by a
 * row-reduction GEMM over fixed row slabs summed in slab order: two identical calls give identical bits.  scratch
 * (optional, 256-byte aligned): gww_adapter_grads_f32_scratch_bytes(M, d_in, d_out, r) bytes, else allocated
 * stream-ordered. */
size_t gww_adapter_grads_f32_scratch_bytes(long M, int d_in, int d_out, int r);
int gww_adapter_grads_f32(const float* X, long ldx, const float* dY, const float* Y, long ldy, const float* bias_st,
                          float yscale, float scaling, const float* A, const float* B, const float* mag, const float* nrm,
                          float* dA, float* dB, float* dm, long M, int d_in, int d_out, int r, void* scratch,
                          size_t scratch_bytes, void* stream);
int gww_dora_grads_multi(const void* X, long ldx, const void* dY, const void* Y, long ldy, int np,
                         const long* col_off, const float* const* bias_st, const float* yscale,
                         const float* scaling, const float* const* A, const float* const* B,
                         const float* const* mag, const float* const* nrm, float* const* dA, float* const* dB,
                         float* const* dm, long M, int d, void* stream);
/* MLGWSC-1 training program (contrastive.hip; fp32, no float atomics: two identical calls give identical bits).
 * InfoNCE of ContrastivePretrainer._info_nce (MLGWSC-1/train.py:410-424): z1, z2 fp32 [B, P] (B >= 1, P <= 1024), each
 * row L2-normalised as F.normalize does (z / max(|z|, 1e-12)); loss = (1/B) sum over the 2B rows of Z = [n1; n2] of
 * LSE_{j != r}(Z Z^T / tau)_rj - (Z Z^T / tau)_{r, pair(r)}, with a max-subtracted LSE (finite where the reference's fp32
 * exp overflows, tau < ~1/88.7).  The forward writes the device scalar `loss` and saves n [2B, P], nrm [2B] (|z| per row),
 * lse [2B] and term [2B] (lse - S_{r,pair}) for the backward.  The backward reads the upstream gradient from the device
 * scalar `dloss` (no host sync) and writes dz1, dz2 [B, P]. */
int gww_info_nce_forward_f32(const float* z1, const float* z2, int B, int P, float tau, float* n, float* nrm, float* lse,
                             float* term, float* loss, void* stream);
int gww_info_nce_backward_f32(const float* n, const float* nrm, const float* lse, const float* term, int B, int P,
                              float tau, const float* dloss, float* dz1, float* dz2, void* stream);
/* Backward of gww_qadapter_tail_f32 for one detector: g fp32, element (b, f, t) at g[b * g_batch_stride + f * T + t] (the
 * gradient of the stacked feature tensor at detector i); y fp32 [B, Hin, Win] as the forward read it.  Writes
 * d_y [B, Hin, Win] (the adaptive-pool backward as a fixed-order gather) and the device scalars d_scale, d_bias,
 * d_gamma_i, d_beta_i (not accumulated).  Win <= 4096, T <= 4096; workspace: gww_qadapter_tail_backward_workspace_bytes. */
size_t gww_qadapter_tail_backward_workspace_bytes(int B, int Hin);
int gww_qadapter_tail_backward_f32(const float* g, long g_batch_stride, const float* y, int B, int Hin, int Win, int F,
                                   int T, const float* scale, const float* bias, const float* gamma_i, float* d_y, void* ws,
                                   size_t ws_bytes, float* d_scale, float* d_bias, float* d_gamma_i, float* d_beta_i,
                                   void* stream);
/* Batch assembly of BinaryGWDataset / PretrainDataset (MLGWSC-1/train.py:262-273, 342-351): row r of out [R, row_len] is
 * noise[idx_noise[r]] + snr[r] * wave[idx_wave[r]] (fp32 product rounded, then fp32 sum rounded: torch's bits), or the
 * noise row alone when idx_wave[r] < 0.  noise [n_noise, row_len], wave [n_wave, row_len]; idx_noise, idx_wave (int32)
 * and snr (fp32) are device arrays of R entries.  A row with an index outside its array is written NaN. */
int gww_assemble_batch_f32(const float* noise, long n_noise, const float* wave, long n_wave, long row_len,
                           const int* idx_noise, const int* idx_wave, const float* snr, int R, float* out, void* stream);
/* The layers of an MLP head (head_chain.h): x [B, d_in] -> Linear -> ReLU -> ... -> Linear C.  The glitch, detection and
 * binary heads take them in these blocks, by pointer; the blocks are host memory, the pointers in them device memory.
 * n_layers is the number of nn.Linear layers of the head the entry runs (4 or 5; any other count is refused, the text
 * names both); layer i (0-based) has w[i] [out_i, in_i] and b[i] [out_i] as nn.Linear stores them, writes its activation
 * h[i] [B, out_i] (the last one: logits [B, C]) and has the gradients dw[i], db[i] of those shapes.  Slots past n_layers
 * are ignored.  x, every w[i], h[i] and dw[i] and the hidden layers' b[i] are 16-byte aligned; the last bias, the logits
 * and db[i] need no alignment.  A forward reads params and writes acts, a scores entry reads params, a backward reads
 * params->w and acts->h (not b, not logits) and writes grads. */
#define GWW_MLP_MAX_LAYERS 5
typedef struct gww_mlp_params {
  int n_layers;
  const float* w[GWW_MLP_MAX_LAYERS];
  const float* b[GWW_MLP_MAX_LAYERS];
} gww_mlp_params;
typedef struct gww_mlp_acts {
  float* h[GWW_MLP_MAX_LAYERS - 1];
  float* logits;
} gww_mlp_acts;
typedef struct gww_mlp_grads {
  float* dw[GWW_MLP_MAX_LAYERS];
  float* db[GWW_MLP_MAX_LAYERS];
} gww_mlp_grads;
/* Glitch-classification head step (classify.hip; fp32 on the exact fp32 MFMA, no float atomics: two identical calls give
 * identical bits).  The head is models.glitch_classifier's nn.Sequential (Glitch_classification/src/model.py:4-39):
 * x [B, d_in] -> Linear 512 -> ReLU -> Dropout(p) -> Linear 256 -> ReLU -> Dropout -> Linear 128 -> ReLU -> Dropout ->
 * Linear C, CrossEntropyLoss (mean) against labels [B] (int64).  d_in a multiple of 128 in 128..1280, C 1..64, B 1..1024;
 * four layers in the blocks above.
 * Forward (2 launches): writes the post-dropout activations h[0] [B, 512], h[1] [B, 256], h[2] [B, 128], logits [B, C],
 * row_loss [B] (lse - z[y]; NaN for a label outside [0, C)), pred [B] (int64 argmax: a NaN logit is the maximum, ties go
 * to the lowest index), dz [B, C] = (softmax - onehot) / B and the device scalar loss = mean(row_loss).  train != 0
 * applies dropout: element e = row * width + col of layer l (0..2) is dropped when word e % 4 of
 * Philox4x32-10(counter = (e / 4, l, offset lo, offset hi), key = (seed lo, seed hi)) is below p * 2^32, kept values are
 * scaled by 1 / (1 - p); gww_head_dropout_mask_f32 returns that mask (1 kept / 0 dropped) for a [B, width] activation.
 * Backward (2 launches): reads the upstream gradient of the loss from the device scalar dloss (NULL: 1), writes
 * dx [B, d_in] and the eight parameter gradients (not accumulated); ws: gww_head_workspace_bytes(B, C) bytes, refused
 * before any launch when ws_bytes is smaller. */
int gww_head_forward_f32(const float* x, const gww_mlp_params* params, const long long* labels, int B, int d_in, int C,
                         float p, int train, unsigned long long seed, unsigned long long offset, const gww_mlp_acts* acts,
                         float* row_loss, long long* pred, float* dz, float* loss, void* stream);
size_t gww_head_workspace_bytes(int B, int C);
int gww_head_backward_f32(const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts, const float* dz,
                          const float* dloss, int B, int d_in, int C, float p, int train, float* ws, size_t ws_bytes,
                          float* dx, const gww_mlp_grads* grads, void* stream);
int gww_head_dropout_mask_f32(unsigned long long seed, unsigned long long offset, int layer, int B, int width, float p,
                              float* mask, void* stream);
/* Evaluation accumulate, one one-workgroup launch per batch: confusion [C, C] (int64, rows = true class) += 1 at
 * (labels[r], argmax logits[r]) with gww_head_forward_f32's argmax rule, loss_sum (fp64) += sum of row_loss in a fixed
 * order, n (int64) += B; all three are device buffers the host reads once per epoch.  C 1..64, B 1..65536. */
int gww_eval_accumulate(const float* logits, const long long* labels, const float* row_loss, int B, int C,
                        long long* confusion, double* loss_sum, long long* n, void* stream);
/* Detection head step (detect.hip; the conventions of the glitch head: exact fp32 MFMA chains, no float atomics, identical
 * calls give identical bits, plain launches, no synchronisation).  The head is models.efficiency_classifier's
 * nn.Sequential (Signal_vs_Noise/Efficiency_test/src/network.py:69-90; GWWhisperClassifier has the same stack):
 * x [B, d_in] -> Linear 512 -> ReLU -> Linear 256 -> ReLU -> Linear 128 -> ReLU -> Linear 64 -> ReLU -> Linear C ->
 * Softmax(dim=1), reg_BCELoss(dim=C, epsilon) (tools.py:181-191) against targets [B, C] (float in [0, 1]).
 * d_in a multiple of 128 in 128..1280, C 2..64, B 1..65536, 0 <= epsilon < 1 / C; five layers in the blocks above; ws and
 * dx 16-byte aligned.
 * Forward (2 launches): writes h[0] [B, 512] .. h[3] [B, 64] (post-ReLU), logits [B, C], probs [B, C],
 * row_loss [B] = sum over c of -[t log q + (1 - t) log(1 - q)] with q = epsilon + (1 - C epsilon) p and both logs clamped
 * at -100 as nn.BCELoss clamps them, the device scalar loss = sum(row_loss) / (B C) (fp64 partial sums in a fixed tree),
 * and dz [B, C] = d loss / d logits through the softmax, with torch's (q - t) / max((1 - q) q, 1e-12) / (B C) as the q
 * derivative.  1 - p_c and 1 - q_c are formed from the sum of the other classes' exponentials, never by subtraction;
 * everything behind the fp32 logits is evaluated in fp64 and rounded to fp32 once per output.
 * Backward (2 launches): reads the upstream gradient of the loss from the device scalar dloss (NULL: 1), writes
 * dx [B, d_in] and the ten parameter gradients (not accumulated); ws: gww_det_head_workspace_bytes(B, C) bytes, refused
 * before any launch when ws_bytes is smaller.
 * Scores (1 launch, inference only): out[r * out_stride] = probs[r, 0] (mode 0) or z0 - z1 (mode 1, C = 2 only: column 0
 * of the reference's remove_softmax layer [[1, -1], [-1, 1]]), bit for bit what the forward gives. */
int gww_det_head_forward_f32(const float* x, const gww_mlp_params* params, const float* targets, int B, int d_in, int C,
                             float epsilon, const gww_mlp_acts* acts, float* probs, float* row_loss, float* dz, float* loss,
                             void* stream);
size_t gww_det_head_workspace_bytes(int B, int C);
int gww_det_head_backward_f32(const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts, const float* dz,
                              const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes, float* dx,
                              const gww_mlp_grads* grads, void* stream);
int gww_det_head_scores_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, int mode, float* out,
                            long out_stride, void* stream);
/* Evaluation accumulate, one one-workgroup launch per batch: correct (int64) += the rows with argmax(targets) ==
 * argmax(probs) (a NaN is the maximum, ties go to the lowest index), loss_sum (fp64) += the batch's mean loss
 * (float)(sum(row_loss) / (B C)), one writer, n (int64) += B, batches (int64) += 1: the reference's validation loss is
 * loss_sum / batches (train.py:150).  C 2..64, B 1..65536. */
int gww_det_eval_accumulate(const float* probs, const float* targets, const float* row_loss, int B, int C,
                            long long* correct, double* loss_sum, long long* n, long long* batches, void* stream);
/* thr[f] = sorted_ascending(scores)[N - ranks[f]] for 1 <= ranks[f] <= N, sorted[0] for ranks[f] == 0 (the reference's
 * noise_outputs[-0], tools.py:354); a NaN orders as the largest value, as torch.sort orders it.  Radix select over the
 * order-preserving integer image of fp32: four histogram passes for all F <= 8 ranks together (9 launches, integer
 * atomics only).  scores [N] fp32, ranks [F] int64 and thr [F] on the device; ws: gww_score_thresholds_workspace_bytes()
 * bytes, 8-byte aligned, refused before any launch when ws_bytes is smaller.  N 1..2^31-1. */
size_t gww_score_thresholds_workspace_bytes(void);
int gww_score_thresholds_f32(const float* scores, long N, const long long* ranks, int F, float* thr, void* ws,
                             size_t ws_bytes, void* stream);
/* counts[f] (int64, device) += #{i < n: scores[i] > thr[f]}, the strict comparison of tools.py:365; F 1..8. */
int gww_detection_counts_f32(const float* scores, long n, const float* thr, int F, long long* counts, void* stream);
/* ---- signal-vs-noise evaluation: ROC curve, AUC and the bootstrap band (csrc/roc.hip) ----
 * Device pointers throughout, plain launches, no host synchronisation.  N is the size of the test set, 2..2^24.  A
 * workspace is refused before any launch when it is smaller than its *_workspace_bytes function says. */
#define GWW_ROC_TILE 16384   /* sorted positions of one LDS tile of the bootstrap kernel */
int gww_roc_tile(void);      /* = GWW_ROC_TILE */
/* Stable descending sort of the scores (LSD radix sort over the order-preserving integer image; -0.0 and +0.0 are one
 * value, +-inf ordinary values).  order [N] int32: the sample at each sorted position; rank [N] int32: its inverse;
 * pos [N] uint8: labels[order[p]] > 0.5; gend [N] int32, of which the first G entries are written: the sorted position of
 * the last element of each run of equal scores; G and n_nan (the number of NaN scores; they sort in front): int32 on the
 * device.  ws 16-byte aligned. */
size_t gww_roc_sort_workspace_bytes(long N);
int gww_roc_sort_f32(const float* scores, const float* labels, long N, int* order, int* rank, unsigned char* pos, int* gend,
                     int* G, int* n_nan, void* ws, size_t ws_bytes, void* stream);
/* sklearn.metrics.roc_curve(drop_intermediate=False): vertex 0 = (0, 0), vertex g + 1 at gend[g].  fps, tps int64 and
 * fpr = fps / Nneg, tpr = tps / P fp64 (one IEEE division each), G + 1 entries of buffers of N + 1; counts int64 [2] =
 * (P, Nneg); auc fp64 [1] = (sum_g (fps_g - fps_{g-1}) (tps_g + tps_{g-1})) / (2 P Nneg): an int64 sum and one division,
 * NaN when one class is absent. */
size_t gww_roc_curve_workspace_bytes(long N);
int gww_roc_curve_f64(const unsigned char* pos, const int* gend, const int* G, long N, long long* fps, long long* tps,
                      double* fpr, double* tpr, long long* counts, double* auc, void* ws, size_t ws_bytes, void* stream);
/* Rc bootstrap replicates, one workgroup each: idx [Rc, N] int32 holds N draws from 0..N-1 per replicate; tpr [Rc, Q]
 * fp64 = np.interp(grid, fpr_r, tpr_r) of the replicate's ROC curve, bit for bit; grid [Q] fp64 ascending in (0, 1],
 * Q 1..1024, Rc 1..65535.  valid [Rc] uint8 = 0 and a row of NaN for a replicate without positives or without negatives
 * (or with a draw outside 0..N-1).  ws: Rc rows of N x 2 uint32, 8-byte aligned; a row is written and read by its own
 * workgroup only. */
size_t gww_roc_bootstrap_workspace_bytes(long Rc, long N);
int gww_roc_bootstrap_tpr_f64(const int* rank, const unsigned char* pos, const int* gend, const int* G, const int* idx, long Rc,
                              long N, const double* grid, int Q, double* tpr, unsigned char* valid, void* ws, size_t ws_bytes,
                              void* stream);
/* mean [Q], std [Q] (population, np.std) of tpr [R, Q] over the rows with valid[r] != 0, summed in row order by one thread
 * per column (numpy's axis-0 order); n_valid int32 [1].  Both NaN when no row is valid. */
int gww_roc_band_f64(const double* tpr, const unsigned char* valid, long R, int Q, double* mean, double* std, int* n_valid,
                     void* stream);
/* One batch of a binary classifier's evaluation, one one-workgroup launch: scores[offset .. offset + B) =
 * sigmoid(logits) (scores holds `capacity` floats), loss_sum (fp64) += the batch-mean BCEWithLogitsLoss rounded to fp32,
 * batches (int64) += 1, confusion (int64 [2][2], rows = the label > 0.5) += the rows by torch.round(sigmoid): a
 * probability of exactly 0.5 is class 0.  B 1..65536. */
int gww_binary_eval_accumulate(const float* logits, const float* labels, int B, float* scores, long offset, long capacity,
                               double* loss_sum, long long* batches, long long* confusion, void* stream);
/* ---- scoring a search: false-alarm rate and sensitive volume (csrc/score.hip) ----
 * The counterpart of MLGWSC-1/evaluate.py: get_stats.  Device pointers throughout, plain launches, no host
 * synchronisation; identical calls give identical bits.  Every count (events E, injections N, background events B, sort
 * elements n) is 1..2^27; more is refused before any launch, and so is a workspace smaller than its *_workspace_bytes
 * function says.  Where a function takes a count from the device (an int32 pointer), it clamps it into 0..capacity. */
/* Stable ascending sort of fp64 keys (LSD radix sort, eight 8-bit digits over the order-preserving 64-bit image; -0.0
 * and +0.0 are one value, +-inf ordinary values, NaNs sort last): order [n] int32 = np.argsort(keys, kind="stable"),
 * sorted [n] fp64 = keys[order]; n_nan int32 [1] = the number of NaN keys.  n_dev: NULL, or the device's element count
 * m <= n: then the first m keys are sorted and only the first m entries of order and sorted are written.  ws 16-byte
 * aligned. */
size_t gww_score_sort_workspace_bytes(long n);
int gww_score_sort_f64(const double* keys, long n, const int* n_dev, double* sorted, int* order, int* n_nan, void* ws,
                       size_t ws_bytes, void* stream);
/* find_closest_index (evaluate.py:66-97) of n values t in the ascending array tc [N]: idx [n] int32 -- an exact midpoint
 * goes to the right neighbour -- and diff [n] fp64 = |tc[idx] - t|. */
int gww_score_closest_f64(const double* tc, long N, const double* t, long n, int* idx, double* diff, void* stream);
/* Events against injections (evaluate.py:152-217).  events [3, E] fp64 (rows time, stat, var), order [E] int32 = the
 * stable argsort of the times, tc [N] fp64 ascending.  Written: fg_sorted [3, E] = events[:, order]; found_idx [E] int32 =
 * the closest injection of every sorted event; an event is a true positive iff |tc[found_idx] - time| <= var; tp_idx /
 * fp_idx [E] int32, tp_diff / fp_diff [E] fp64, tp_events / fp_events [3, E] fp64 (row pitch E): the sorted positions, the
 * |dt| and the events of the true / false positives in order, counts[0] / counts[1] entries (columns) of each;
 * found_inj [N] int32, found_stat [N] fp64: the injections whose run of events holds a true positive and the largest
 * statistic among those, in index order, counts[2] entries; missed [N] int32: the injections no event is closest to,
 * counts[3] entries.  counts int32 [5]: true positives, false positives, found, missed, and the number of events with a
 * NaN in time, stat or var (the caller refuses those).  ws 16-byte aligned. */
size_t gww_score_match_workspace_bytes(long E, long N);
int gww_score_match_f64(const double* events, const int* order, long E, const double* tc, long N, double* fg_sorted,
                        int* found_idx, int* tp_idx, int* fp_idx, double* tp_diff, double* fp_diff, double* tp_events,
                        double* fp_events, int* found_inj, double* found_stat, int* missed, int* counts, void* ws,
                        size_t ws_bytes, void* stream);
/* far[k] = (m - k - 1) / duration for k < m (evaluate.py:185-186, 193-194); m = n, or the device's count n_dev[0] <= n. */
int gww_score_far_f64(const int* n_dev, long n, double duration, double* far, void* stream);
/* Chirp-mass weighting (evaluate.py:250-263): cs1[p] = the sum of w1[found_inj[order[q]]] over q = p .. F - 1, cs2 the
 * same of w2, cs[F] = 0; F = F[0] on the device, w1, w2 [N] fp64 per injection, found_inj and order [N] int32, cs1 and
 * cs2 [N + 1] fp64 of which F + 1 entries are written.  One workgroup; the additions happen in one fixed order. */
int gww_score_suffix_f64(const double* w1, const double* w2, long N, const int* found_inj, const int* order, const int* F,
                         double* cs1, double* cs2, void* stream);
/* Per ascending background statistic (evaluate.py:244-276): fidx = searchsorted(found_sorted[:F], noise, 'right'),
 * nfound (int64) = F - fidx, fraction = nfound / Ninj; cs1 == cs2 == NULL: volume = prefactor * nfound, variance =
 * fraction - fraction^2; otherwise volume = prefactor * cs1[fidx], variance = cs2[fidx] / Ninj - (cs1[fidx] / Ninj)^2;
 * volume_err = prefactor * sqrt(Ninj * variance).  found_sorted [N] fp64 of which F[0] (device) entries are read. */
int gww_score_volume_f64(const double* found_sorted, const int* F, long N, const double* noise_sorted, long B, double Ninj,
                         double prefactor, const double* cs1, const double* cs2, long long* nfound, double* fraction,
                         double* volume, double* volume_err, void* stream);
/* ---- the efficiency study's test stage: triggers, events, false-alarm rate (csrc/trigger_stats.hip)
 * The counterpart of Efficiency_test/src/evaluate_test_data.py.  Device pointers throughout, plain launches, no host
 * synchronisation; identical calls give identical bits and no result depends on the launch geometry.  Every size and
 * capacity is 1..2^27; more is refused before any launch, and so is a workspace (16-byte aligned) smaller than its
 * *_workspace_bytes function says.  A count taken from the device (an int32 pointer) is clamped into 0..capacity. */
/* get_triggers: the samples with series[i] > threshold, compared in fp64 (series fp64, or fp32 when is_f64 == 0: widened
 * exactly; equality is no trigger, a NaN never is), in order: times[j] = double(i) * delta_t + epoch (two roundings, no
 * fused multiply-add), values[j] = series[i].  times, values [cap], cap <= n.  counts int32 [2] = (the number of
 * triggers -- of which the first cap are stored --, the number of NaN samples). */
size_t gww_trig_triggers_workspace_bytes(long n);
int gww_trig_triggers_f64(const void* series, int is_f64, long n, long cap, double delta_t, double epoch, double threshold,
                          double* times, double* values, int* counts, void* ws, size_t ws_bytes, void* stream);
/* Clusters and events over ascending trigger times: trigger j opens a cluster iff j == 0 or times[j] - times[j-1] >=
 * tolerance; per cluster, in order, the time and value of the FIRST maximum of its values (np.argmax), however many
 * workgroups the cluster spans.  times, values, ev_times, ev_values [cap] fp64; n_dev: NULL (cap triggers) or the device's
 * count.  counts int32 [2] = (events, NaN values). */
size_t gww_trig_events_workspace_bytes(long cap);
int gww_trig_events_f64(const double* times, const double* values, const int* n_dev, long cap, double tolerance,
                        double* ev_times, double* ev_values, int* counts, void* ws, size_t ws_bytes, void* stream);
/* True positive iff diff[j] <= tolerance (diff: the distance to the nearest injection, gww_score_closest_f64); the values
 * of the true and of the false positives in order into tp_values / fp_values [cap].  counts int32 [3] = (true positives,
 * false positives, NaN values). */
size_t gww_trig_split_workspace_bytes(long cap);
int gww_trig_split_f64(const double* values, const double* diff, const int* n_dev, long cap, double tolerance,
                       double* tp_values, double* fp_values, int* counts, void* ws, size_t ws_bytes, void* stream);
/* Ranking steps (evaluate_test_data.py:555-612) over the ascending false-positive values fp_sorted (n_fp[0] of cap) and
 * true-positive values tp_sorted (n_tp[0] of cap_tp): one step per run [a, b] of equal values; ranking = v[a]; count =
 * n_fp - b - 1, except n_fp for a first run of length one; far = count / duration * 2592000; tidx =
 * searchsorted(tp_sorted, ranking, 'right'); sens_frac = 1 - tidx / n_tp; s = n_tp - tidx, q = s / Ninj, sens_vol =
 * prefactor * s, sens_vol_err = prefactor * sqrt(Ninj * (q - q * q)).  Outputs [cap] fp64 of which n_steps[0] (int32,
 * device) entries are written.  duration > 0. */
size_t gww_trig_steps_workspace_bytes(long cap);
int gww_trig_steps_f64(const double* fp_sorted, const int* n_fp, long cap, const double* tp_sorted, const int* n_tp,
                       long cap_tp, double duration, double prefactor, double Ninj, double* ranking, double* far,
                       double* sens_frac, double* sens_vol, double* sens_vol_err, int* n_steps, void* ws, size_t ws_bytes,
                       void* stream);
/* Coincidences of two detectors' event lists at zero lag and under time slides (coinc.hip).  t0 fp64
 * ascending / v0 fp32: detector 0's events, n0 of them, or -- n0_dev != NULL, an int32 on the device -- the first
 * clamp(n0_dev[0], 0, n0); t1 / v1 / n1 / n1_dev likewise (t1 ascending over the events that count).  shifts fp64 [S] on
 * the device.  Events i and j are coincident in slide s iff fabs(d) <= window, d = (t1[j] + shifts[s]) - t0[i] in fp64, one
 * addition then one subtraction; i's partner is, of its coincident j, the one of the largest v1, then of the smallest
 * fabs(d), then the smallest j.  n0, n1 0..2^27 (0 is legal: no coincidences), S 1..65535, window >= 0.  Plain launches,
 * no atomics, no synchronisation, identical calls give identical bits.
 *   gww_coinc_blocks   the workgroups per slide, max(1, ceil(n0 / 256)): blocks is int64 [S * gww_coinc_blocks(n0)]
 *   gww_coinc_count    partner int32 [S, n0] = the partner of every detector-0 event (-1: none; rows behind the device's
 *                      count too); blocks = the coincidences of every (slide, workgroup)
 *   gww_coinc_offsets  blocks becomes its own exclusive scan in (slide, workgroup) order; offsets int64 [S + 1] = where
 *                      slide s starts in the ragged result, offsets[S] = the total
 *   gww_coinc_emit     per coincidence, slide after slide and in ascending i within a slide: time = t0[i], stat =
 *                      double(v0[i]) + double(v1[j]), dt = d(i, j), idx0 = i, idx1 = j, each [cap_total].  Nothing is
 *                      written at or beyond cap_total; offsets keeps the true totals, so a cut list is seen. */
size_t gww_coinc_blocks(long n0);
int gww_coinc_count_f64(const double* t0, const int* n0_dev, long n0, const double* t1, const float* v1, const int* n1_dev,
                        long n1, const double* shifts, int S, double window, int* partner, long long* blocks, void* stream);
int gww_coinc_offsets(long long* blocks, long n0, int S, long long* offsets, void* stream);
int gww_coinc_emit_f64(const double* t0, const float* v0, const int* n0_dev, long n0, const double* t1, const float* v1,
                       const int* n1_dev, long n1, const double* shifts, int S, const int* partner, const long long* blocks,
                       long cap_total, double* time, double* stat, double* dt, int* idx0, int* idx1, void* stream);
/* Both outputs of the detection head per row, inference only, one launch (test_network.py): out [B, C] fp32 with row
 * pitch out_stride >= C.  mode 0: the softmax, the bits of gww_det_head_forward_f32's probs; mode 1 (C = 2): (z0 - z1,
 * z1 - z0), the reference's --remove-softmax layer.  Operands as gww_det_head_scores_f32. */
int gww_det_head_scores2_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, int mode, float* out,
                             long out_stride, void* stream);
/* CNN decoder head of the two-detector model (cnn_head.hip; models.TwoChannelLIGOBinaryClassifierCNN, the reference's
 * Signal_vs_Noise/src/model.py:57-85): per sample x [2, d] -> Conv1d(2, 64, 3, pad 1) -> ReLU -> Conv1d(64, 128, 3, pad 1)
 * -> ReLU -> Conv1d(128, 256, 3, pad 1) -> ReLU -> mean over d -> Linear(256, C).  Exact fp32 (the wide convolutions are
 * v_mfma_f32_16x16x4_f32 chains), no float atomics, every reduction in a fixed order: identical calls give identical
 * bits, and a sample's logits and dx depend neither on B nor on its index.  Parameters are torch's own tensors, device
 * fp32: w1 [64,2,3] b1 [64] w2 [128,64,3] b2 [128] w3 [256,128,3] b3 [256] w4 [C,256] b4 [C]; w2, w3, b2, b3 16-byte
 * aligned.  d: an encoder width (128, 384, 512, 768, 1024, 1280); C 1..64; B 1..65535.
 * Forward (1 launch): x fp32 [B, 2, d] -> logits [B, C].  saved == NULL: no activation leaves the chip.  Otherwise saved
 * (gww_cnn_head_saved_bytes) receives the three post-ReLU activations, [B, 64 + 128 + 256, d]; the logits have the same
 * bits either way.
 * Backward (10 launches): dlogits [B, C] -> dx [B, 2, d] and the eight parameter gradients in torch's shapes
 * (overwritten).  workspace: gww_cnn_head_workspace_bytes (0 = unsupported geometry), 16-byte aligned, scratch: its
 * contents before the call do not matter.  GWW_ERR_WORKSPACE when it is smaller. */
size_t gww_cnn_head_saved_bytes(int B, int d);
size_t gww_cnn_head_workspace_bytes(int B, int d, int C);
int gww_cnn_head_forward_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* w3, const float* b3, const float* w4, const float* b4, int B, int d, int C,
                             float* logits, float* saved, void* stream);
int gww_cnn_head_backward_f32(const float* x, const float* saved, const float* dlogits, const float* w1, const float* w2,
                              const float* w3, const float* w4, int B, int d, int C, float* dx, float* dw1, float* db1,
                              float* dw2, float* db2, float* dw3, float* db3, float* dw4, float* db4, void* workspace,
                              size_t workspace_bytes, void* stream);
/* fp32 -> bf16 (round to nearest even), n elements */
int gww_cast_f32_bf16(const float* x, void* y, long n, void* stream);
/* Binary head step of the signal-vs-noise trainers (binary_head.hip; the conventions of the detection head: exact fp32
 * MFMA chains, no float atomics, identical calls give identical bits, plain launches, no synchronisation).  Two layouts of
 * the reference's Signal_vs_Noise/src/model.py, ReLU between the layers, BCEWithLogitsLoss against targets [B, C] (float in
 * [0, 1]):
 *   GWW_BIN_HEAD_ONE  one_channel_ligo_binary_classifier: x [B, d_in] -> 512 -> 256 -> 128 -> 64 -> C, five layers,
 *                     d_in a multiple of 128 in 128..1280
 *   GWW_BIN_HEAD_TWO  two_channel_ligo_binary_classifier: x [B, d_in] -> 1024 -> 512 -> 256 -> C, four layers, d_in a
 *                     multiple of 256 in 256..2560
 * C 1..64, B 1..65536; the layers in the blocks above (n_layers 5 or 4, as the layout has them); ws and dx 16-byte aligned.
 * Forward (2 launches): writes the post-ReLU activations h[i] [B, width_i], logits [B, C], probs [B, C] = sigmoid(z),
 * row_loss [B] = sum over c of max(z, 0) - z t + log1p(exp(-|z|)) (torch's form), the device scalar loss = sum(row_loss) /
 * (B C) (fp64 partial sums in a fixed tree, rounded once) and dz [B, C] = (sigmoid(z) - t) / (B C), formed as
 * ((1 - t) p - t (1 - p)) / (B C) with 1 - p from the exponential, never by subtraction.  Everything behind the fp32
 * logits is evaluated in fp64 and rounded to fp32 once per output.  At equal weights and C the logits of GWW_BIN_HEAD_ONE
 * are the bits of gww_det_head_forward_f32's, and its backward is the detection head's own kernels.
 * Backward (2 launches): reads the upstream gradient of the loss from the device scalar dloss (NULL: 1), writes
 * dx [B, d_in] and every parameter gradient (not accumulated); ws: gww_bin_head_workspace_bytes(layout, B, C) bytes (0 for
 * an unknown layout), refused before any launch when ws_bytes is smaller.
 * Scores (1 launch, inference only): logits [B, C], bit for bit the forward's. */
#define GWW_BIN_HEAD_ONE 1
#define GWW_BIN_HEAD_TWO 2
int gww_bin_head_forward_f32(int layout, const float* x, const gww_mlp_params* params, const float* targets, int B, int d_in,
                             int C, const gww_mlp_acts* acts, float* probs, float* row_loss, float* dz, float* loss,
                             void* stream);
size_t gww_bin_head_workspace_bytes(int layout, int B, int C);
int gww_bin_head_backward_f32(int layout, const float* x, const gww_mlp_params* params, const gww_mlp_acts* acts,
                              const float* dz, const float* dloss, int B, int d_in, int C, float* ws, size_t ws_bytes,
                              float* dx, const gww_mlp_grads* grads, void* stream);
int gww_bin_head_scores_f32(int layout, const float* x, const gww_mlp_params* params, int B, int d_in, int C, float* logits,
                            void* stream);
/* ---- glitch scan (csrc/glitch_scan.hip) ----
 * gww_head_scan_f32: the glitch head of gww_head_forward_f32 in eval mode (no dropout, no labels, nothing saved), ONE launch:
 * x fp32 [B, d_in] -> for row r of the batch, at element row_offset + r of the caller's arrays, cls (int32: the argmax of
 * the logits by gww_head_forward_f32's rule -- a NaN is the maximum, ties go to the lowest index), prob (fp32: the softmax
 * probability of that class, 1 / sum_j expf(z_j - z_max)) and, when probs is not NULL, probs [., C] = expf(z_j - z_max) /
 * sum.  The logits are the bits gww_head_forward_f32(train = 0) writes.  Shapes as there: d_in a multiple of 128 in
 * 128..1280, C 1..64, B 1..1024; params holds four layers, acts are not needed.
 * gww_glitch_events: the events of every class from the per-window results of one series, on the device, no host
 * synchronisation: times fp64 [n] (the slicer's stamps), cls int32 [n], prob fp32 [n].  Window i triggers when
 * 0 <= cls[i] < 64, bit cls[i] of ignore is clear and prob[i] > prob_threshold (a NaN never triggers).  The triggers of one
 * class, in order, join the class's running event unless times[i] - (the event's last stamp) > gap (fp64, strict); classes
 * do not see each other, so events of different classes may overlap.  Event e, ordered by its first window: ev_cls,
 * ev_first (that window), ev_n (its windows), ev_t_start / ev_t_end (first / last stamp), ev_t_peak / ev_p_peak (stamp and
 * probability of its FIRST maximum).  The arrays hold cap entries; *count = the events found and counts on past cap.
 * ws: gww_glitch_events_workspace_bytes(n) bytes, 16-byte aligned, refused before any launch when smaller.  n 0..2^31-65.
 * Two launches (one for n = 0); identical calls give identical bits. */
int gww_head_scan_f32(const float* x, const gww_mlp_params* params, int B, int d_in, int C, long row_offset, int* cls,
                      float* prob, float* probs, void* stream);
size_t gww_glitch_events_workspace_bytes(long n);
int gww_glitch_events(const double* times, const int* cls, const float* prob, long n, float prob_threshold, double gap,
                      unsigned long long ignore, int cap, int* ev_cls, int* ev_first, int* ev_n, double* ev_t_start,
                      double* ev_t_end, double* ev_t_peak, float* ev_p_peak, int* count, void* ws, size_t ws_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GWW_H */
