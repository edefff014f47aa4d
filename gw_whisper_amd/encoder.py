"""``WhisperEncoder``-compatible module backed by libgww.so.

Mirrors the HuggingFace surface the reference uses:

* built like ``WhisperModel.from_pretrained(id).encoder``
  (reference ``Signal_vs_Noise/src/train.py:227-228``): here
  ``WhisperEncoder(WhisperConfig.named("tiny"))`` + ``load_state_dict`` of an HF
  encoder ``state_dict`` (same key names: ``conv1``, ``conv2``,
  ``embed_positions``, ``layers.N.self_attn.{k,v,q,out}_proj``,
  ``layers.N.self_attn_layer_norm``, ``layers.N.fc1/fc2``,
  ``layers.N.final_layer_norm``, ``layer_norm``);
* ``named_modules()`` yields the names the reference's ``fnmatch`` target search
  consumes (``src/train.py:230-237``);
* ``encoder(mel)`` takes ``[B, num_mel_bins, 3000]`` fp32 (80 mels, 128 for large-v3) on the GPU and returns an object
  with ``.last_hidden_state [B, 1500, d]`` (``src/model.py:25-26``);
  ``encoder.config.d_model`` exists (``src/model.py:11``);
* ``gradient_checkpointing_enable()`` is accepted (``MLGWSC-1/train.py:662``);
* ``encoder(mel, output_hidden_states=True, output_attentions=True)`` returns HF's per-layer outputs
  (``.hidden_states``: L + 1 tensors ``[B, 1500, d]``, ``.attentions``: L tensors ``[B, H, 1500, 1500]``, eager
  attention's ``attn_weights``), inference only; ``return_dict=False`` returns HF's plain tuple.

The context is HF's ``max_source_positions``: ``WhisperConfig(max_source_positions=T)`` for any ``T`` in [16, 1500] takes
``[B, num_mel_bins, 2 T]`` features (a ``WhisperFeatureExtractor`` of the matching ``chunk_length`` / ``hop_length`` makes
them) and returns ``[B, T, d]``; ``with_context(T)`` cuts a longer encoder to it.

The submodules hold parameters only; all arithmetic runs in the HIP library.
Calling the module with CPU tensors raises -- there is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import operator
import sys
import weakref
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _lib, synth
from ._lib import check, lib


@dataclass
class WhisperConfig:
    d_model: int = 384
    encoder_layers: int = 4
    encoder_attention_heads: int = 6
    encoder_ffn_dim: int = 1536
    num_mel_bins: int = 80
    max_source_positions: int = 1500
    dropout: float = 0.0
    # what forward() returns when its keyword is None (HF PretrainedConfig fields of the same names)
    output_hidden_states: bool = False
    output_attentions: bool = False
    return_dict: bool = True

    @staticmethod
    def named(name: str) -> "WhisperConfig":
        d, L, H, F = synth.ENCODER_SIZES[name]
        return WhisperConfig(d, L, H, F, num_mel_bins=synth.encoder_mels(name))

    @staticmethod
    def from_json_file(path: str) -> "WhisperConfig":
        """The encoder fields of an HF Whisper ``config.json`` (what ``save_pretrained`` writes); a missing
        ``num_mel_bins`` means 80, as in HF; so do the output flags that are absent."""
        import json
        with open(path) as f:
            j = json.load(f)
        return WhisperConfig(j["d_model"], j["encoder_layers"], j["encoder_attention_heads"], j["encoder_ffn_dim"],
                             num_mel_bins=j.get("num_mel_bins", 80),
                             max_source_positions=j.get("max_source_positions", 1500),
                             output_hidden_states=bool(j.get("output_hidden_states", False)),
                             output_attentions=bool(j.get("output_attentions", False)),
                             return_dict=bool(j.get("return_dict", True)))


@dataclass
class BaseModelOutput:
    """HF ``BaseModelOutput``: the tuple view (indexing, ``to_tuple()``, ``return_dict=False``) skips the fields that
    are None, so ``o[0]`` is always ``last_hidden_state``."""
    last_hidden_state: torch.Tensor
    hidden_states: tuple | None = None
    attentions: tuple | None = None

    def to_tuple(self) -> tuple:
        return tuple(v for v in (self.last_hidden_state, self.hidden_states, self.attentions) if v is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]


# THE description of the encoder's weights (include/gww.h); every list of them in this file and in training.py derives from it.
# One row per module of a layer, in the field order of gww_enc_layer / gww_enc_layer_grads: path below the layer, weight field,
# bias field (k_proj has no bias), dirty bit of gww_encoder_update_weights (bit 0 q/k/v + LN1, bit 1 out_proj, bit 2 fc1 + LN2,
# bit 3 fc2), gww_dora_target.proj of a linear layer (None: a LayerNorm).
_LAYER = (("self_attn_layer_norm", "ln1_w", "ln1_b", 1, None),
          ("self_attn.q_proj", "q_w", "q_b", 1, 0),
          ("self_attn.k_proj", "k_w", None, 1, 1),
          ("self_attn.v_proj", "v_w", "v_b", 1, 2),
          ("self_attn.out_proj", "o_w", "o_b", 2, 3),
          ("final_layer_norm", "ln2_w", "ln2_b", 4, None),
          ("fc1", "fc1_w", "fc1_b", 4, 4),
          ("fc2", "fc2_w", "fc2_b", 8, 5))
# ... and per global module, in the field order of gww_enc_globals / gww_enc_grads: path, weight field, bias field
_GLOBALS = (("conv1", "conv1_w", "conv1_b"), ("conv2", "conv2_w", "conv2_b"), ("embed_positions", "pos", None),
            ("layer_norm", "ln_w", "ln_b"))


def _fields(rows):
    """[(struct field, module path, "weight" | "bias")] of a table, in the struct's order."""
    return [(f, r[0], attr) for r in rows for f, attr in ((r[1], "weight"), (r[2], "bias")) if f]


class _ParamCache:
    """What one walk of the module tree below an encoder found.  The per-step host work of a training forward used to walk
    the tree five times (``parameters()`` / ``named_parameters()`` are recursive generators: ~0.3 ms per step with the GPU
    idle behind the loop's per-step sync); the lists are kept instead, and before they are trusted ``valid()`` compares
    every ``_modules`` / ``_parameters`` entry below the encoder with the object seen at build time (whisper-tiny with
    DoRA on q / k / v: 260 entries, ~25 us).  Only the cheap per-parameter fields (requires_grad, data_ptr, _version) are
    read fresh."""

    def __init__(self, enc):
        n = len(enc.layers)
        self.named = []                                   # list(enc.named_parameters())
        self.globals = []                                 # parameters of the weight groups: the globals' ...
        self.layers = [([], [], [], []) for _ in range(n)]   # ... and per layer one list per dirty bit
        group_of = {r[0]: self.globals for r in _GLOBALS}
        group_of.update({f"layers.{i}.{r[0]}": self.layers[i][r[3].bit_length() - 1] for i in range(n) for r in _LAYER})
        self._dicts, self._in, self._key, self._obj = [], [], [], []   # every _parameters / _modules dict, and its entries
        seen = set()

        def walk(mod, prefix, group):
            for d in (mod._parameters, mod._modules):
                self._dicts.append(d)
                self._in += [d] * len(d)
                self._key += d.keys()
                self._obj += d.values()
            for k, p in mod._parameters.items():
                if p is not None:
                    if group is not None:
                        group.append(p)
                    if id(p) not in seen:                 # (named_parameters() names a shared parameter once)
                        seen.add(id(p))
                        self.named.append((prefix + k, p))
            for k, m in mod._modules.items():
                if m is not None:
                    walk(m, prefix + k + ".", group_of.get(prefix + k, group))

        walk(enc, "", None)
        self.base = [(name, p) for name, p in self.named if "lora_" not in name]
        self.adapters = [p for name, p in self.named if "lora_" in name]
        # the modules of the rows of _LAYER, per layer; the A matrices of the adapted ones
        self.modules = [[layer.get_submodule(r[0]) for r in _LAYER] for layer in enc.layers]
        self.lora_A = [p for mods in self.modules for m in mods if hasattr(m, "lora_A") for p in m.lora_A.parameters()]

    def valid(self) -> bool:
        """Every entry is the object seen at build time and none was added (flat lists: a nested loop over the modules
        costs five times as much)."""
        try:
            return sum(map(len, self._dicts)) == len(self._obj) and \
                all(map(operator.is_, map(operator.getitem, self._in, self._key), self._obj))
        except KeyError:
            return False


class _Attention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=True)
        self.q_proj = nn.Linear(d, d, bias=True)
        self.out_proj = nn.Linear(d, d, bias=True)


class _EncoderLayer(nn.Module):
    def __init__(self, d, ffn):
        super().__init__()
        self.self_attn = _Attention(d)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.fc1 = nn.Linear(d, ffn)
        self.fc2 = nn.Linear(ffn, d)
        self.final_layer_norm = nn.LayerNorm(d)


# Encoders that have run a training forward.  An optimizer step changes their adapters, and the next forward would start by
# re-preparing the packed weights (DoRA merge, panel packs, LayerNorm folds: host work + a handful of launches) with the GPU
# idle behind the step's loss.item() / synchronize -- the reference loop syncs every step (Signal_vs_Noise/src/train.py:163-168).
# A global optimizer post-step hook does that work right behind optimizer.step(), while the GPU is still busy with the step's
# backward: the next forward finds its change keys equal and returns at once.  Nothing is assumed about the caller's loop: a
# weight changed later (load_state_dict, another optimizer) changes the keys again and is re-synced as before.
_TRAINED = weakref.WeakSet()
_HOOKED = False


def _post_step_sync(*_args, **_kw):
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return   # (the sync allocates tensors and records an event: both illegal inside a graph capture)
    for enc in list(_TRAINED):
        try:
            if enc._handle is None:
                continue
            c = enc._param_cache()
            dev = c.named[0][1].device
            if dev.type != "cuda" or not (enc._has_trainable_adapters(c) or enc.full_finetune):
                continue
            with torch.no_grad(), torch.cuda.device(dev):
                enc._sync_weights(c)
        except Exception:
            pass   # (a failed early sync is not an error: the next forward syncs and reports)


def _note_training(enc):
    global _HOOKED
    _TRAINED.add(enc)
    if not _HOOKED:
        from torch.optim.optimizer import register_optimizer_step_post_hook
        register_optimizer_step_post_hook(_post_step_sync)
        _HOOKED = True


def _effective_weight(linear) -> torch.Tensor:
    """Dense fp32 weight a (possibly DoRA-wrapped) projection currently represents."""
    if hasattr(linear, "effective_weight"):
        return linear.effective_weight()
    return linear.weight


def _bias(linear):
    base = getattr(linear, "base_layer", linear)
    return base.bias


class WhisperEncoder(nn.Module):
    """Parameter container + launcher for the HIP encoder forward."""

    MIN_CONTEXT, MAX_CONTEXT = 16, 1500   # supported max_source_positions (the route each (d, T) takes)

    def __init__(self, config: WhisperConfig, precision: str = "bf16"):
        super().__init__()
        T = config.max_source_positions
        if int(T) != T or not self.MIN_CONTEXT <= T <= self.MAX_CONTEXT:
            raise ValueError(f"WhisperEncoder: max_source_positions={T!r} must be an integer in "
                             f"[{self.MIN_CONTEXT}, {self.MAX_CONTEXT}]")
        self.config = config
        d = config.d_model
        self.conv1 = nn.Conv1d(config.num_mel_bins, d, kernel_size=3, padding=1)
        self.conv2 = nn.Conv1d(d, d, kernel_size=3, stride=2, padding=1)
        self.embed_positions = nn.Embedding(config.max_source_positions, d)
        self.embed_positions.requires_grad_(False)
        with torch.no_grad():
            self.embed_positions.weight.copy_(torch.from_numpy(synth.sinusoid_table(config.max_source_positions, d)))
        self.layers = nn.ModuleList([_EncoderLayer(d, config.encoder_ffn_dim) for _ in range(config.encoder_layers)])
        self.layer_norm = nn.LayerNorm(d)
        # The base is born frozen: no base-weight backward exists here, so a freshly built
        # encoder runs inference with or without torch.no_grad(); only an explicit un-freeze (the reference's
        # full_finetune, Signal_vs_Noise/src/train.py:244-250) meets the refusal in _wants_grad.
        self._freeze_parameters()
        self.full_finetune = False   # enable_full_finetune(): the HIP base-weight backward
        self.precision = precision
        self.gradient_checkpointing = False
        self._handle = None
        self._packed_key = None
        self._ws = None

    # ---- HF surface the reference touches
    def gradient_checkpointing_enable(self, *a, **k):
        self.gradient_checkpointing = True   # activations are recomputed-by-design in the HIP backward

    def enable_full_finetune(self) -> "WhisperEncoder":
        """Opt in to full fine-tuning (Signal_vs_Noise/src/train.py:243-247 ``--method full_finetune``,
        Glitch_classification/src/train_full_finetune.py): afterwards the base parameters that require grad get their
        gradients from the HIP base-weight backward (gww_encoder_train_backward_full); the others stay frozen.  Without
        this call an un-frozen base parameter is refused (_wants_grad).  DoRA / LoRA adapters cannot be combined with it
        -- the reference never mixes them.  Full fine-tuning is bf16-only: precision='fp32' has an adapter training
        step (training.py) but no fp32 base-weight backward."""
        if self.precision != "bf16":
            raise _lib.GwwError("full fine-tuning is implemented for precision='bf16'")
        if self._has_adapters():
            raise _lib.GwwError("enable_full_finetune(): the encoder carries DoRA / LoRA adapters; full fine-tuning "
                                "trains the base weights and does not combine with adapters")
        self.full_finetune = True
        return self

    def _has_adapters(self) -> bool:
        return bool(self._param_cache().adapters)

    def config_dict(self) -> dict:
        """The encoder's ``config.json`` with HF WhisperConfig field names (what :meth:`save_pretrained` writes and
        ``WhisperConfig.from_json_file`` reads)."""
        c = self.config
        return {"model_type": "whisper", "architectures": ["WhisperEncoder"], "d_model": c.d_model,
                "encoder_layers": c.encoder_layers, "encoder_attention_heads": c.encoder_attention_heads,
                "encoder_ffn_dim": c.encoder_ffn_dim, "num_mel_bins": c.num_mel_bins,
                "max_source_positions": c.max_source_positions, "dropout": c.dropout, "activation_function": "gelu",
                "scale_embedding": False, "torch_dtype": "float32"}

    def save_pretrained(self, save_directory: str):
        """HF ``WhisperEncoder.save_pretrained`` layout (Signal_vs_Noise/src/train.py:196 saves a fully fine-tuned
        encoder this way): ``config.json`` with WhisperConfig field names and ``model.safetensors`` whose keys are the
        HF encoder ``state_dict`` keys (what ``--encoder-weights`` / ``load_state_dict`` read back)."""
        import json
        import os

        from safetensors.torch import save_file
        if self._has_adapters():
            raise _lib.GwwError("save_pretrained() of an adapted encoder: save the adapter through the PeftModel")
        os.makedirs(save_directory, exist_ok=True)
        cfg = self.config_dict()
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
        sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in self.state_dict().items()}
        save_file(sd, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})

    def _freeze_parameters(self):
        for p in self.parameters():
            p.requires_grad = False

    @staticmethod
    def from_pretrained(save_directory: str, max_source_positions: int | None = None, **kw) -> "WhisperEncoder":
        """Load what :meth:`save_pretrained` wrote: ``config.json`` (geometry and ``num_mel_bins``) and
        ``model.safetensors``.  ``max_source_positions=T`` below the saved context builds the encoder of that context:
        rows 0 .. T - 1 of the saved position table (what HF users get from ``ignore_mismatched_sizes`` plus a slice)."""
        import dataclasses
        import os

        from safetensors.torch import load_file
        cfg = WhisperConfig.from_json_file(os.path.join(save_directory, "config.json"))
        if max_source_positions is not None:
            if max_source_positions > cfg.max_source_positions:
                raise ValueError(f"WhisperEncoder.from_pretrained: max_source_positions={max_source_positions} exceeds "
                                 f"the saved position table ({cfg.max_source_positions} rows)")
            cfg = dataclasses.replace(cfg, max_source_positions=int(max_source_positions))
        enc = WhisperEncoder(cfg, **kw)
        enc.load_state_dict(load_file(os.path.join(save_directory, "model.safetensors")))
        return enc

    def load_state_dict(self, state_dict, *args, **kwargs):
        """``nn.Module.load_state_dict``; a position table LONGER than this encoder's context is cut to its rows
        0 .. T - 1 (the sinusoids of a position do not depend on the table's length).  A shorter one is an error, as ever.
        The cut is silent, so it also takes a checkpoint loaded into the WRONG encoder -- a 1500-row table into a T = 100
        encoder built by mistake -- without a word: the context is this encoder's configuration, never the checkpoint's.
        Where the two are meant to agree, compare ``state_dict["embed_positions.weight"].shape[0]`` with
        ``config.max_source_positions`` before loading."""
        key = "embed_positions.weight"
        pos = state_dict.get(key) if hasattr(state_dict, "get") else None
        T = self.config.max_source_positions
        if pos is not None and getattr(pos, "ndim", 0) == 2 and pos.shape[0] > T:
            state_dict = dict(state_dict)
            state_dict[key] = pos[:T]
        return super().load_state_dict(state_dict, *args, **kwargs)

    def with_context(self, max_source_positions: int) -> "WhisperEncoder":
        """A new encoder of context ``max_source_positions`` <= this one's with the same weights (copies) and rows
        0 .. T - 1 of ``embed_positions``, on the same device and in the same precision; HF state-dict keys throughout.
        For an adapted encoder, cut the base first and attach the adapters to the result."""
        import dataclasses
        T = int(max_source_positions)
        if T > self.config.max_source_positions:
            raise ValueError(f"with_context({T}): this encoder's position table has {self.config.max_source_positions} rows")
        if self._has_adapters():
            raise _lib.GwwError("with_context() of an adapted encoder: cut the base encoder, then attach the adapters")
        enc = WhisperEncoder(dataclasses.replace(self.config, max_source_positions=T), precision=self.precision)
        enc.load_state_dict(self.state_dict())
        return enc.to(self.embed_positions.weight.device)

    @staticmethod
    def from_numpy_state_dict(sd: dict, config: WhisperConfig, **kw) -> "WhisperEncoder":
        enc = WhisperEncoder(config, **kw)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return enc

    # ---- library plumbing
    def __del__(self):
        try:
            h = self.__dict__.get("_handle")
            self.__dict__["_handle"] = None
            # at interpreter shutdown the HIP runtime may already be torn down: the process exit frees the
            # device memory, calling into the library then can block
            if h is not None and not sys.is_finalizing():
                lib().gww_encoder_destroy(h)
        except Exception:
            pass

    def _ensure_handle(self):
        if self._handle is None:
            c = self.config
            cfg = _lib.EncCfg(c.d_model, c.encoder_layers, c.encoder_attention_heads, c.encoder_ffn_dim,
                              c.num_mel_bins, 2 * c.max_source_positions)
            h = C.c_void_p()
            check(lib().gww_encoder_create(C.byref(cfg), C.byref(h)), "gww_encoder_create")
            self._handle = h
        return self._handle

    def _param_cache(self) -> _ParamCache:
        """The parameter lists of this encoder, rebuilt by one walk of the module tree when any module or parameter below it
        was assigned, replaced, added or removed since they were built.  Every entry into the encoder validates once and
        hands the result down; the helpers below validate only when they are called on their own."""
        c = self.__dict__.get("_pcache")
        if c is None or not c.valid():
            c = self.__dict__["_pcache"] = _ParamCache(self)
        return c

    def _group_keys(self, c=None):
        """Change keys per weight group -- (data_ptr, version) of every parameter of the group, DoRA wrappers included:
        globals, and per layer the four groups of gww_encoder_update_weights (the dirty bits of _LAYER)."""
        c = self._param_cache() if c is None else c
        key = lambda ps: tuple((p.data_ptr(), p._version) for p in ps)
        return key(c.globals), [tuple(key(ps) for ps in g) for g in c.layers]

    def _sync_weights(self, c=None):
        """Re-pack into the library's bf16/fp32 panels what changed since the last call (optimizer step,
        load_state_dict, DoRA update): everything the first time, afterwards only the dirty weight groups
        (a DoRA step touches the attention projections: the frozen fc1 / fc2 / stem panels are packed once)."""
        c = self._param_cache() if c is None else c
        # The panels may have been packed on ANOTHER stream (the optimizer post-step hook runs on whatever stream
        # optimizer.step() ran on): order this stream behind that work before anything packs into or reads a panel.
        stream = torch.cuda.current_stream()
        ev = self.__dict__.get("_packed_event")
        if ev is not None and ev[0] != stream.cuda_stream:
            stream.wait_event(ev[1])
        gkey, lkeys = self._group_keys(c)
        old = self._packed_key
        if old == (gkey, lkeys):
            return
        full = old is None
        masks = [15 if full else sum((1 << b) for b in range(4) if old[1][i][b] != lkeys[i][b])
                 for i in range(len(lkeys))]
        keep = []   # keep temporaries alive until the async packing kernels are enqueued

        def ptr(t):
            t = t.detach().to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        # every DoRA-wrapped projection of a dirty group merged by one launch
        wrapped = [x for mods, m in zip(c.modules, masks) for x, r in zip(mods, _LAYER)
                   if m & r[3] and hasattr(x, "effective_weights")]
        merged = {}
        if wrapped:
            merged = {id(x): w for x, w in zip(wrapped, type(wrapped[0]).effective_weights(wrapped))}
        eff = lambda lin: merged[id(lin)] if id(lin) in merged else _effective_weight(lin)

        g = None
        if full or old[0] != gkey:
            g = _lib.EncGlobals(**{f: ptr(getattr(self.get_submodule(path), attr)) for f, path, attr in _fields(_GLOBALS)})
        n = len(lkeys)
        arr = (_lib.EncLayer * n)()
        for lay, mods, m in zip(arr, c.modules, masks):
            for mod, (_, w_field, b_field, bit, _) in zip(mods, _LAYER):
                if m & bit:                                   # clean groups: pointers are not read
                    setattr(lay, w_field, ptr(eff(mod)))
                    if b_field:
                        setattr(lay, b_field, ptr(_bias(mod)))
        if full:
            check(lib().gww_encoder_set_weights(self._ensure_handle(), C.byref(g), arr, n, stream.cuda_stream),
                  "gww_encoder_set_weights")
        else:
            dirty = (C.c_uint * n)(*masks)
            check(lib().gww_encoder_update_weights(self._ensure_handle(), C.byref(g) if g is not None else None, arr, n,
                                                   dirty, stream.cuda_stream), "gww_encoder_update_weights")
        self._packed_key = (gkey, lkeys)
        ev = torch.cuda.Event()
        ev.record(stream)
        self.__dict__["_packed_event"] = (stream.cuda_stream, ev)

    def _workspace(self, batch: int, prec: int, device) -> torch.Tensor:
        need = lib().gww_encoder_workspace_bytes(self._ensure_handle(), batch, prec)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty((need,), dtype=torch.uint8, device=device)
        return self._ws

    @property
    def _prec(self) -> int:
        """The library's precision code."""
        return {"bf16": _lib.PREC_BF16, "fp32": _lib.PREC_F32}[self.precision]

    def _enter(self, x) -> _ParamCache:
        """Every entry into the encoder starts here: the validated parameter cache, and the input checked against it."""
        c = self._param_cache()
        if not x.is_cuda:
            raise _lib.GwwError("WhisperEncoder.forward needs GPU tensors: gw_whisper_amd has no CPU fallback "
                                f"(got input on {x.device})")
        t_in = 2 * self.config.max_source_positions
        if x.dim() != 3 or x.shape[1] != self.config.num_mel_bins or x.shape[-1] != t_in:
            raise ValueError(f"Whisper expects the mel input features to be of length {t_in}, but found "
                             f"{x.shape[-1]}. Make sure to pad the input mel features to {t_in}.")
        if c.named[0][1].device != x.device:
            raise _lib.GwwError("encoder parameters and input are on different devices")
        return c

    def forward_raw(self, input_features: torch.Tensor, want_hidden: bool = True, want_last: bool = False, cache=None):
        """Launch the HIP forward; returns (last_hidden_state | None, last_token | None).  ``cache``: what ``_enter``
        returned to a caller that has checked this input already."""
        c = self._enter(input_features) if cache is None else cache
        x, prec = input_features.to(torch.float32).contiguous(), self._prec
        cfg = self.config
        B = x.shape[0]
        with torch.cuda.device(x.device):
            self._sync_weights(c)
            ws = self._workspace(B, prec, x.device)
            hidden = torch.empty((B, cfg.max_source_positions, cfg.d_model), dtype=torch.float32,
                                 device=x.device) if want_hidden else None
            last = torch.empty((B, cfg.d_model), dtype=torch.float32, device=x.device) if want_last else None
            check(lib().gww_encoder_forward(self._handle, x.data_ptr(), B, prec, ws.data_ptr(), ws.numel(),
                                            hidden.data_ptr() if want_hidden else None,
                                            last.data_ptr() if want_last else None,
                                            torch.cuda.current_stream().cuda_stream), "gww_encoder_forward")
        return hidden, last

    def forward_outputs_raw(self, input_features: torch.Tensor, want_hidden_states: bool, want_attentions: bool,
                            cache=None):
        """Launch the HIP forward with HF's per-layer outputs (gww_encoder_forward_outputs); returns
        (last_hidden_state, hidden_states | None, attentions | None).  Each output is a view of one fp32 slab;
        ``hidden_states[-1]`` is ``last_hidden_state`` itself."""
        c = self._enter(input_features) if cache is None else cache
        x, prec = input_features.to(torch.float32).contiguous(), self._prec
        cfg = self.config
        B, T, d, L, H = x.shape[0], cfg.max_source_positions, cfg.d_model, cfg.encoder_layers, cfg.encoder_attention_heads
        f32 = dict(dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            self._sync_weights(c)
            ws = self._workspace(B, prec, x.device)
            hs = torch.empty((L + 1, B, T, d), **f32) if want_hidden_states else None
            last = hs[L] if want_hidden_states else torch.empty((B, T, d), **f32)
            at = torch.empty((L, B, H, T, T), **f32) if want_attentions else None
            check(lib().gww_encoder_forward_outputs(self._handle, x.data_ptr(), B, prec, ws.data_ptr(), ws.numel(),
                                                    last.data_ptr(), hs.data_ptr() if hs is not None else None,
                                                    at.data_ptr() if at is not None else None,
                                                    torch.cuda.current_stream().cuda_stream), "gww_encoder_forward_outputs")
        hidden_states = tuple(hs[:L].unbind(0)) + (last,) if hs is not None else None
        attentions = tuple(at.unbind(0)) if at is not None else None
        return last, hidden_states, attentions

    def set_split(self, on: bool = True):
        """Process large batches as two half batches on two streams (see gww_encoder_set_split)."""
        check(lib().gww_encoder_set_split(self._ensure_handle(), int(on)), "gww_encoder_set_split")
        self._ws = None

    def set_stem_shortcut(self, on: bool = True):
        """Constant-tail shortcut of the bf16 inference stem (see gww_encoder_set_stem_shortcut); on by default."""
        check(lib().gww_encoder_set_stem_shortcut(self._ensure_handle(), int(on)), "gww_encoder_set_stem_shortcut")

    def set_x_native(self, on: bool = True):
        """Residual stream in accumulator order between the fused blocks (see gww_encoder_set_x_native); on by default."""
        check(lib().gww_encoder_set_x_native(self._ensure_handle(), int(on)), "gww_encoder_set_x_native")

    def stem_shortcut_flags(self, batch: int) -> tuple:
        """What the last inference forward of ``batch`` segments decided on the device, per half batch: 1 = shortcut
        taken, 0 = full stem, -1 = does not apply (synchronises)."""
        if self._ws is None:
            raise _lib.GwwError("stem_shortcut_flags: no forward has run yet")
        flags = (C.c_int * 2)()
        with torch.cuda.device(self._ws.device):
            torch.cuda.synchronize()
            check(lib().gww_encoder_stem_shortcut_flags(self._ensure_handle(), int(batch), self._prec, self._ws.data_ptr(), flags),
                  "gww_encoder_stem_shortcut_flags")
        return int(flags[0]), int(flags[1])

    # ---- per-kernel event trace (bench.py roofline)
    def trace_enable(self, on: bool = True):
        check(lib().gww_encoder_trace_enable(self._ensure_handle(), int(on)), "gww_encoder_trace_enable")

    def trace_read(self) -> dict:
        """{kernel class: (total ms, launches)} since the last read (synchronises)."""
        n = lib().gww_encoder_trace_classes()
        ms = (C.c_float * n)()
        cnt = (C.c_int * n)()
        check(lib().gww_encoder_trace_read(self._ensure_handle(), ms, cnt), "gww_encoder_trace_read")
        return {lib().gww_encoder_trace_class_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def forward(self, input_features, attention_mask=None, output_hidden_states=None, output_attentions=None,
                return_dict=None, **kwargs):
        """HF ``WhisperEncoder.forward``: ``None`` flags fall back to the config.  ``output_hidden_states`` /
        ``output_attentions`` are inference only (no gradient flows through them): with autograd on and trainable
        adapters (or an input that requires grad) they raise."""
        c = self.config
        want_h = c.output_hidden_states if output_hidden_states is None else bool(output_hidden_states)
        want_a = c.output_attentions if output_attentions is None else bool(output_attentions)
        as_dict = c.return_dict if return_dict is None else bool(return_dict)
        cache = self._enter(input_features)
        if want_a and c.max_source_positions % 4:
            raise _lib.GwwError(f"WhisperEncoder: output_attentions needs max_source_positions % 4 == 0 (the attention maps "
                                f"are stored 16 bytes at a time), got {c.max_source_positions}")
        if self._wants_grad(input_features, cache):
            if want_h or want_a:
                raise _lib.GwwError("WhisperEncoder: output_hidden_states / output_attentions are inference only (no "
                                    "gradient flows through them): run under torch.no_grad() or freeze the adapters")
            # DoRA training step: HIP forward that keeps activations + HIP backward (training.py)
            from .training import encoder_train_forward
            out = BaseModelOutput(last_hidden_state=encoder_train_forward(self, input_features, cache=cache))
        elif want_h or want_a:
            last, hs, at = self.forward_outputs_raw(input_features, want_h, want_a, cache=cache)
            out = BaseModelOutput(last_hidden_state=last, hidden_states=hs, attentions=at)
        else:
            hidden, _ = self.forward_raw(input_features, want_hidden=True, want_last=False, cache=cache)
            out = BaseModelOutput(last_hidden_state=hidden)
        return out if as_dict else out.to_tuple()

    def _wants_grad(self, input_features, c=None) -> bool:
        if not torch.is_grad_enabled():
            return False
        # Only the frozen-base + DoRA backward exists (and the input gradient).  A base parameter that was un-frozen on
        # purpose -- the reference's `full_finetune` method, Signal_vs_Noise/src/train.py:244-250 -- would silently get no
        # gradient: refuse.  (Nothing trainable at all is the inference case.)
        c = self._param_cache() if c is None else c
        input_grad = torch.is_tensor(input_features) and input_features.requires_grad
        base_trainable = [n for n, p in c.base if p.requires_grad]
        if not base_trainable and not any(p.requires_grad for p in c.adapters):
            return input_grad
        if self.full_finetune:
            if c.adapters:
                raise _lib.GwwError("WhisperEncoder: full fine-tuning is enabled and DoRA / LoRA adapters are attached: "
                                    "the two do not combine")
            return True   # (no adapters, so a base parameter trains)
        if base_trainable:
            raise _lib.GwwError(
                "WhisperEncoder: autograd is on and base parameters require grad (e.g. " + base_trainable[0] + "): only "
                "the frozen-base + DoRA training step (and the input gradient) is implemented -- freeze the encoder "
                "(get_peft_model does) or run under torch.no_grad()")
        return self._has_trainable_adapters(c) or input_grad

    def _has_trainable_adapters(self, c=None) -> bool:
        """Whether an adapter on one of the linear layers of _LAYER trains (its A matrix requires grad)."""
        return any(p.requires_grad for p in (self._param_cache() if c is None else c).lora_A)

    def last_token(self, input_features) -> torch.Tensor:
        """``self(mel).last_hidden_state[:, -1, :]`` without materialising the other
        1499 rows of the final LayerNorm (reference ``src/model.py:25-26``).  Differentiable: with trainable
        adapters (or an input that requires grad) this is the pooled training step of ``training.py``."""
        cache = self._enter(input_features)
        if self._wants_grad(input_features, cache):
            from .training import encoder_train_forward
            return encoder_train_forward(self, input_features, pooled=True, cache=cache)
        return self.forward_raw(input_features, want_hidden=False, want_last=True, cache=cache)[1]
