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


def base_targets(encoder, cache=None):
    """[(field, layer index or None, parameter)] of the trainable base parameters (full fine-tuning only), in the field
    order of gww_enc_grads / gww_enc_layer_grads (encoder._GLOBALS / _LAYER)."""
    if not encoder.full_finetune:
        return []
    c = cache or encoder._param_cache()
    out = [(f, None, getattr(encoder.get_submodule(path), attr)) for f, path, attr in _encoder._fields(_encoder._GLOBALS)]
    for li, mods in enumerate(c.modules):
        for mod, (_, w_field, b_field, _, _) in zip(mods, _encoder._LAYER):
            out += [(w_field, li, mod.weight)] + ([(b_field, li, mod.bias)] if b_field else [])
    return [t for t in out if t[2].requires_grad]


def dora_targets(encoder, cache=None):
    """[(layer index, proj id, DoraLinear)] of the adapted linear layers, layer-major and by proj id: q / k / v / out_proj
    (0..3), fc1 / fc2 (4, 5)."""
    c = cache or encoder._param_cache()
    # (use_dora=False, plain LoRA, the reference's --method LoRA, included)
    return [(li, r[4], mod) for li, mods in enumerate(c.modules) for mod, r in zip(mods, _encoder._LAYER)
            if r[4] is not None and isinstance(mod, DoraLinear)]


class _Plan:
    """What one training step runs, decided once per forward from (precision, base targets, wide adapter targets): the
    targets, the autograd inputs in the order the backward returns their gradients, the workspace query, the backward."""

    def __init__(self, enc, cache):
        self.cache, self.targets, self.base = cache, dora_targets(enc, cache), base_targets(enc, cache)
        self.f32 = enc.precision == "fp32"   # the exact-fp32 step (gww_encoder_train_forward_f32): its own arena sizes
        if self.f32 and self.base:           # (enable_full_finetune refuses fp32 already)
            raise _lib.GwwError("full fine-tuning is implemented for precision='bf16'")
        # fc1 / fc2 targets or ranks other than 8 run on the adapter-gradient kernel, whose scratch the attention-only
        # rank-8 step does not need
        wide = [t[2].r for t in self.targets if t[1] > 3 or t[2].r != 8]
        kind = "_f32" if self.f32 else "_full" if self.base else ""
        self.backward = "gww_encoder_train_backward" + kind
        if kind or not wide:
            self.ws_query, self.ws_args = "gww_train_workspace_bytes" + kind, ()
        else:
            self.ws_query, self.ws_args = "gww_train_workspace_bytes_adapters", (max(wide),)
        self.params = []
        for _, _, mod in self.targets:
            self.params += [mod.lora_A[mod.adapter].weight, mod.lora_B[mod.adapter].weight]
            if mod.use_dora:
                self.params.append(mod.lora_magnitude_vector[mod.adapter].weight)
        self.params += [p for _, _, p in self.base]   # full fine-tuning (enable_full_finetune)


class _EncoderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, encoder, mel, pooled, plan, *params):
        enc = encoder
        c = enc.config
        x = mel.to(torch.float32).contiguous()
        B = x.shape[0]
        dev = x.device
        sfx = "_f32" if plan.f32 else ""
        with torch.cuda.device(dev):
            enc._sync_weights(plan.cache)
            _encoder._note_training(enc)   # from now on the packed weights follow every optimizer step at once
            h = enc._ensure_handle()
            ws = torch.empty((getattr(lib(), plan.ws_query)(h, B, *plan.ws_args),), dtype=torch.uint8, device=dev)
            saved = torch.empty((getattr(lib(), "gww_train_saved_bytes" + sfx)(h, B),), dtype=torch.uint8, device=dev)
            shape = (B, c.d_model) if pooled else (B, c.max_source_positions, c.d_model)
            hidden = torch.empty(shape, dtype=torch.float32, device=dev)
            fwd = "gww_encoder_train_forward" + sfx
            check(getattr(lib(), fwd)(h, x.data_ptr(), B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(),
                                      hidden.data_ptr(), int(pooled), torch.cuda.current_stream().cuda_stream), fwd)
        # the backward gets THIS workspace back: d_mel and the conv-stem gradients are formed from what the forward left
        # at its front (include/gww.h); everything else in it is scratch
        ctx.enc, ctx.B, ctx.ws, ctx.saved, ctx.pooled, ctx.plan = enc, B, ws, saved, bool(pooled), plan
        ctx.mel_shape = tuple(x.shape)
        return hidden

    @staticmethod
    def backward(ctx, d_hidden):
        enc, B = ctx.enc, ctx.B
        dev = d_hidden.device
        d_hidden = d_hidden.to(torch.float32).contiguous()
        targets, base = ctx.plan.targets, ctx.plan.base
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
            if base:
                args += (C.byref(gl),)
            check(getattr(lib(), ctx.plan.backward)(*args, torch.cuda.current_stream().cuda_stream), ctx.plan.backward)
        flat = []
        for g in grads:
            flat += list(g)
        flat += base_ret
        assert len(flat) == len(ctx.plan.params)
        ctx.ws = ctx.saved = None
        return (None, d_mel, None, None, *flat)


def encoder_train_forward(encoder, mel: torch.Tensor, pooled: bool = False, cache=None) -> torch.Tensor:
    """last_hidden_state [B, 1500, d] -- or, with ``pooled``, its last token [B, d] (what every classifier of the
    reference reads, ``Signal_vs_Noise/src/model.py:25-26``; the last layer's row-wise ops and their backward then run
    on B rows instead of B * 1500) -- with autograd through the DoRA parameters and, when ``mel.requires_grad``,
    through the conv stem to the input features.  ``cache``: the encoder's parameter cache, when the caller validated it."""
    if encoder.precision not in ("bf16", "fp32"):
        raise _lib.GwwError(f"no training step for precision={encoder.precision!r}")
    plan = _Plan(encoder, cache or encoder._param_cache())
    return _EncoderTrain.apply(encoder, mel, bool(pooled), plan, *plan.params)
