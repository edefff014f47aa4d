"""Autograd bridge of the DoRA training step.

``encoder_train_forward(encoder, mel)`` runs the HIP training forward (activations kept in an
arena) and returns ``last_hidden_state`` as a tensor that participates in torch autograd; its
backward calls ``gww_encoder_train_backward`` and hands the A / B / magnitude gradients of every
DoRA-wrapped linear layer (q / k / v / out_proj, fc1 / fc2) to autograd, so the reference's step

    loss = criterion(model(h1, l1), labels); loss.backward(); optimizer.step()
    (Signal_vs_Noise/src/train.py:163-168)

works with the MLP head, the loss and AdamW in plain torch on the GPU and everything inside the
encoder in libgww.  The DoRA weight norm is detached exactly like peft 0.12.0 ``dora.py``.

An encoder built with ``precision="fp32"`` runs the exact-fp32 twin of the step (``gww_encoder_train_forward_f32`` /
``_backward_f32``): the reference's own training arithmetic, with no autocast anywhere.

With ``WhisperEncoder.enable_full_finetune()`` the base parameters that require grad are inputs of the same autograd
node, and the backward is ``gww_encoder_train_backward_full`` with their fp32 gradient buffers.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import encoder as _encoder
from ._lib import check, lib
from .peft import DoraLinear

_PROJ = {"q_proj": 0, "k_proj": 1, "v_proj": 2, "out_proj": 3}
_MLP = {"fc1": 4, "fc2": 5}   # gww_dora_target.proj of the MLP projections (include/gww.h)


# base parameters in the order of gww_enc_grads / gww_enc_layer_grads (include/gww.h)
_GLOBAL_GRADS = (("conv1_w", "conv1.weight"), ("conv1_b", "conv1.bias"), ("conv2_w", "conv2.weight"),
                 ("conv2_b", "conv2.bias"), ("pos", "embed_positions.weight"), ("ln_w", "layer_norm.weight"),
                 ("ln_b", "layer_norm.bias"))
_LAYER_GRADS = (("ln1_w", "self_attn_layer_norm.weight"), ("ln1_b", "self_attn_layer_norm.bias"),
                ("q_w", "self_attn.q_proj.weight"), ("q_b", "self_attn.q_proj.bias"), ("k_w", "self_attn.k_proj.weight"),
                ("v_w", "self_attn.v_proj.weight"), ("v_b", "self_attn.v_proj.bias"),
                ("o_w", "self_attn.out_proj.weight"), ("o_b", "self_attn.out_proj.bias"),
                ("ln2_w", "final_layer_norm.weight"), ("ln2_b", "final_layer_norm.bias"),
                ("fc1_w", "fc1.weight"), ("fc1_b", "fc1.bias"), ("fc2_w", "fc2.weight"), ("fc2_b", "fc2.bias"))


def base_targets(encoder):
    """[(field, layer index or None, parameter)] of the trainable base parameters (full fine-tuning only)."""
    if not encoder.full_finetune:
        return []
    out = []
    get = lambda mod, path: mod.get_parameter(path)
    for field, path in _GLOBAL_GRADS:
        p = get(encoder, path)
        if p.requires_grad:
            out.append((field, None, p))
    for li, layer in enumerate(encoder.layers):
        for field, path in _LAYER_GRADS:
            p = get(layer, path)
            if p.requires_grad:
                out.append((field, li, p))
    return out


def dora_targets(encoder):
    """[(layer index, proj id, DoraLinear)] of the adapted linear layers: q / k / v / out_proj (0..3), fc1 / fc2 (4, 5)."""
    out = []
    for li, layer in enumerate(encoder.layers):
        mods = [(getattr(layer.self_attn, name), pid) for name, pid in _PROJ.items()]
        mods += [(getattr(layer, name), pid) for name, pid in _MLP.items()]
        for mod, pid in mods:
            if isinstance(mod, DoraLinear):
                out.append((li, pid, mod))   # use_dora=False (plain LoRA, the reference's --method LoRA) included
    return out


class _EncoderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, encoder, mel, pooled, *params):
        enc = encoder
        c = enc.config
        x = mel.to(torch.float32).contiguous()
        B = x.shape[0]
        dev = x.device
        with torch.cuda.device(dev):
            enc._sync_weights()
            _encoder._note_training(enc)   # from now on the packed weights follow every optimizer step at once
            h = enc._ensure_handle()
            f32 = enc.precision == "fp32"   # the exact-fp32 step (gww_encoder_train_forward_f32): its own arena sizes
            full = bool(base_targets(enc))
            # fc1 / fc2 targets or ranks other than 8 run on the adapter-gradient kernel, whose scratch the attention-only
            # rank-8 step does not need
            wide = [t for t in dora_targets(enc) if t[1] > 3 or t[2].r != 8]
            if f32:
                ws_bytes = lib().gww_train_workspace_bytes_f32(h, B)
            elif full:
                ws_bytes = lib().gww_train_workspace_bytes_full(h, B)
            elif wide:
                ws_bytes = lib().gww_train_workspace_bytes_adapters(h, B, max(t[2].r for t in wide))
            else:
                ws_bytes = lib().gww_train_workspace_bytes(h, B)
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            saved_bytes = lib().gww_train_saved_bytes_f32(h, B) if f32 else lib().gww_train_saved_bytes(h, B)
            saved = torch.empty((saved_bytes,), dtype=torch.uint8, device=dev)
            shape = (B, c.d_model) if pooled else (B, c.max_source_positions, c.d_model)
            hidden = torch.empty(shape, dtype=torch.float32, device=dev)
            fwd = lib().gww_encoder_train_forward_f32 if f32 else lib().gww_encoder_train_forward
            check(fwd(h, x.data_ptr(), B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(), hidden.data_ptr(),
                      int(pooled), torch.cuda.current_stream().cuda_stream),
                  "gww_encoder_train_forward" + ("_f32" if f32 else ""))
        # the backward gets THIS workspace back: d_mel and the conv-stem gradients are formed from what the forward left
        # at its front (include/gww.h); everything else in it is scratch
        ctx.enc, ctx.B, ctx.ws, ctx.saved, ctx.pooled = enc, B, ws, saved, bool(pooled)
        ctx.n_params = len(params)
        ctx.mel_shape = tuple(x.shape)
        return hidden

    @staticmethod
    def backward(ctx, d_hidden):
        enc, B = ctx.enc, ctx.B
        dev = d_hidden.device
        d_hidden = d_hidden.to(torch.float32).contiguous()
        targets = dora_targets(enc)
        arr = (_lib.DoraTarget * max(len(targets), 1))()
        grads, keep = [], []
        def grad_buffer(param, like):
            # The HIP backward ACCUMULATES into the buffers it is given.  When the parameter already owns a dense fp32
            # .grad (optimizer.zero_grad(set_to_none=False), dist.FlatGradBucket views) it accumulates straight into
            # that and autograd gets None for this input -- no zeros_like + add kernel per tensor (96 tiny launches
            # per whisper-tiny step).  Otherwise: a fresh zero buffer handed back to autograd as usual.
            g = param.grad
            if (g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.device == like.device
                    and g.shape == like.shape and not g.requires_grad):
                return g, None
            z = torch.zeros_like(like)
            return z, z
        for i, (li, pid, mod) in enumerate(targets):
            pA, pB = mod.lora_A[mod.adapter].weight, mod.lora_B[mod.adapter].weight
            A = pA.detach().float().contiguous()
            Bm = pB.detach().float().contiguous()
            (dA, rA), (dB, rB) = grad_buffer(pA, A), grad_buffer(pB, Bm)
            if mod.use_dora:
                pm = mod.lora_magnitude_vector[mod.adapter].weight
                mag = pm.detach().float().contiguous()
                nrm = mod._last_norm
                dm, rm = grad_buffer(pm, mag)
                grads.append((rA, rB, rm))
            else:
                # plain LoRA (peft tuners/lora/layer.py, use_dora=False: W' = W0 + s B A) is the DoRA gradient with the
                # row gain g = m / ||W'|| == 1: magnitude and norm are both ones, the magnitude gradient is discarded
                mag = nrm = torch.ones(mod.out_features, dtype=torch.float32, device=dev)
                dm = torch.zeros_like(mag)
                grads.append((rA, rB))
            keep += [A, Bm, mag, nrm, dA, dB, dm]
            arr[i] = _lib.DoraTarget(li, pid, mod.r, float(mod.scaling), A.data_ptr(), Bm.data_ptr(), mag.data_ptr(),
                                     nrm.data_ptr(), dA.data_ptr(), dB.data_ptr(), dm.data_ptr())
        # gradient w.r.t. the input features (conv stem backward) only when autograd asks for it
        d_mel = torch.empty(ctx.mel_shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        base = base_targets(enc)
        base_ret = []
        if base:
            gl = _lib.EncGrads()
            layers = (_lib.EncLayerGrads * len(enc.layers))()
            gl.layers = layers
            for field, li, p in base:
                buf, ret = grad_buffer(p, p.detach())
                keep.append(buf)
                base_ret.append(ret)
                setattr(gl if li is None else layers[li], field, buf.data_ptr())
        with torch.cuda.device(dev):
            args = (enc._ensure_handle(), B, ctx.ws.data_ptr(), ctx.ws.numel(), ctx.saved.data_ptr(), ctx.saved.numel(),
                    d_hidden.data_ptr(), arr, len(targets), None, d_mel.data_ptr() if d_mel is not None else None,
                    int(ctx.pooled))
            stream = torch.cuda.current_stream().cuda_stream
            if enc.precision == "fp32":
                check(lib().gww_encoder_train_backward_f32(*args, stream), "gww_encoder_train_backward_f32")
            elif base:
                check(lib().gww_encoder_train_backward_full(*args, C.byref(gl), stream), "gww_encoder_train_backward_full")
            else:
                check(lib().gww_encoder_train_backward(*args, stream), "gww_encoder_train_backward")
        flat = []
        for g in grads:
            flat += list(g)
        flat += base_ret
        assert len(flat) == ctx.n_params
        ctx.ws = ctx.saved = None
        return (None, d_mel, None, *flat)


def encoder_train_forward(encoder, mel: torch.Tensor, pooled: bool = False) -> torch.Tensor:
    """last_hidden_state [B, 1500, d] -- or, with ``pooled``, its last token [B, d] (what every classifier of the
    reference reads, ``Signal_vs_Noise/src/model.py:25-26``; the last layer's row-wise ops and their backward then run
    on B rows instead of B * 1500) -- with autograd through the DoRA parameters and, when ``mel.requires_grad``,
    through the conv stem to the input features."""
    if encoder.precision not in ("bf16", "fp32"):
        raise _lib.GwwError(f"no training step for precision={encoder.precision!r}")
    if encoder.precision == "fp32" and base_targets(encoder):   # (enable_full_finetune refuses fp32 already)
        raise _lib.GwwError("full fine-tuning is implemented for precision='bf16'")
    params = []
    for _, _, mod in dora_targets(encoder):
        params += [mod.lora_A[mod.adapter].weight, mod.lora_B[mod.adapter].weight]
        if mod.use_dora:
            params.append(mod.lora_magnitude_vector[mod.adapter].weight)
    params += [p for _, _, p in base_targets(encoder)]   # full fine-tuning (enable_full_finetune)
    return _EncoderTrain.apply(encoder, mel, bool(pooled), *params)
