"""The reference's MLGWSC-1 training program (``MLGWSC-1/train.py``) on the MI355X path: the pieces
``harness/run_mlgwsc_train.py`` is built from, under the reference's names.

    info_nce                 <->  ContrastivePretrainer._info_nce (:410-424), an autograd Function over the HIP kernels
                                  of ``csrc/contrastive.hip`` (``gww_info_nce_forward_f32`` / ``_backward_f32``)
    BinaryGWDataset          <->  BinaryGWDataset (:221-297): injections first (label [1, 0]), then noise ([0, 1])
    PretrainDataset          <->  PretrainDataset (:300-351): two views noise_k + SNR * waveform, or two noise rows
    ConcatGWData                  the reference's ConcatDataset of one BinaryGWDataset per file (:744-773), device resident
    DeviceBatches                 DataLoader(shuffle=...) over either dataset: batches are PLANNED on the host (the same
                                  generator calls, in the same order, as the reference's ``__getitem__``) and BUILT on the
                                  device in one launch (``gww_assemble_batch_f32``); the arrays never leave HBM
    ContrastivePretrainer    <->  ContrastivePretrainer (:377-463)
    SupervisedTrainer        <->  SupervisedTrainer (:478-640), checkpoint layout, resume, early stop, ``losses.txt``
    apply_lora / save_model_components / build_network  <->  :666-737

The model is ``inference.GWWhisperClassifier`` with ``qscan.QTransformAdapter.train_variant``; every GPU-side step of it
is HIP (Q-scan, the adapter CNN and its tail in both directions, the DoRA / LoRA encoder step, InfoNCE).
"""

from __future__ import annotations

import fnmatch
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .inference import GWWhisperClassifier, RegBCELoss

__all__ = ["info_nce", "BinaryGWDataset", "PretrainDataset", "ConcatGWData", "DeviceBatches", "ContrastivePretrainer",
           "SupervisedTrainer", "RegBCELoss", "apply_lora", "build_network", "save_model_components"]


# =============================================================================================== InfoNCE
class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, temperature):
        from . import ops
        loss, saved = ops.info_nce_forward(z1.to(torch.float32), z2.to(torch.float32), temperature)
        ctx.saved, ctx.temperature, ctx.dtypes = saved, float(temperature), (z1.dtype, z2.dtype)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import ops
        dz1, dz2 = ops.info_nce_backward(ctx.saved, ctx.temperature, g.to(torch.float32))
        ctx.saved = None
        return dz1.to(ctx.dtypes[0]), dz2.to(ctx.dtypes[1]), None


def info_nce(z1: torch.Tensor, z2: torch.Tensor, temperature: float) -> torch.Tensor:
    """``ContrastivePretrainer._info_nce`` (MLGWSC-1/train.py:410-424): z1, z2 [B, P] (P <= 1024) -> scalar loss
    ``mean_i[-log(pos_i / den1_i) - log(pos_i / den2_i)]`` over ``F.normalize``-d rows, similarities ``/ temperature``.
    Three HIP launches forward, one backward, fp32, fixed-order reductions (identical bits on identical calls).  The log-sum-exp
    subtracts the row maximum: where the reference's fp32 ``exp(sim)`` is finite the value is the same; for temperatures
    below about 1/88.7, where ``exp(1 / temperature)`` overflows fp32 and the reference returns inf or NaN, this stays
    finite."""
    if not (z1.is_cuda and z2.is_cuda):
        raise _lib.GwwError("info_nce needs GPU tensors: gw_whisper_amd has no CPU path")
    return _InfoNCE.apply(z1, z2, float(temperature))


# =============================================================================================== datasets
WAVE_LABEL = (1.0, 0.0)
NOISE_LABEL = (0.0, 1.0)


class BinaryGWDataset:
    """Reference ``BinaryGWDataset`` (MLGWSC-1/train.py:221-297): the first ``len(waveforms)`` indices are injections
    ``noises[i] + snr * waveforms[i]`` (label [1, 0], snr ~ U(snr_range)), the rest noise alone (label [0, 1]);
    ``len`` is ``len(noises)``.  ``__getitem__`` is the reference's; ``plan`` is what ``DeviceBatches`` uses."""

    def __init__(self, noises=None, waveforms=None, store_device: str = "cpu", train_device: str = "cuda",
                 snr_range: Tuple[float, float] = (5.0, 15.0)):
        self.noises = noises
        self.waveforms = waveforms
        self.store_device = store_device
        self.train_device = train_device
        self.snr_range = snr_range
        self.wave_label = torch.tensor(WAVE_LABEL, dtype=torch.float32)
        self.noise_label = torch.tensor(NOISE_LABEL, dtype=torch.float32)
        if self.noises is not None:
            self._to_tensors()
        self.rng = np.random.default_rng()

    def __len__(self) -> int:
        return len(self.noises)

    def __getitem__(self, i: int):
        if i < len(self.waveforms):
            snr_val = self.rng.uniform(*self.snr_range)
            return self.noises[i] + snr_val * self.waveforms[i], self.wave_label
        return self.noises[i], self.noise_label

    def plan(self, indices: Sequence[int], rng: Optional[np.random.Generator] = None):
        """(noise row [n], wave row or -1 [n], snr fp32 [n]) of items ``indices``: for each item the draw
        ``__getitem__`` makes (one ``uniform(*snr_range)`` per injection), in item order."""
        rng = self.rng if rng is None else rng
        n = len(indices)
        idx_n, idx_w, snr = np.empty(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.float32)
        n_wave = len(self.waveforms)
        for k, i in enumerate(indices):
            i = int(i)
            idx_n[k] = i
            if i < n_wave:
                snr[k] = rng.uniform(*self.snr_range)
                idx_w[k] = i
        return idx_n, idx_w, snr

    def _to_tensors(self) -> None:
        if isinstance(self.noises, np.ndarray):
            self.noises = torch.from_numpy(self.noises)
        if isinstance(self.waveforms, np.ndarray):
            self.waveforms = torch.from_numpy(self.waveforms)
        self.noises = self.noises.to(dtype=torch.float32, device=self.store_device)
        self.waveforms = self.waveforms.to(dtype=torch.float32, device=self.store_device)

    def load(self, group, group_name: str = None) -> None:
        """``load(h5py_file, group_name)`` as the reference; also ``load(mapping_of_arrays)`` for one group."""
        g = group[group_name] if group_name is not None else group
        self.noises = np.asarray(g["noises"][()])
        self.waveforms = np.asarray(g["waveforms"][()])
        self._to_tensors()


class PretrainDataset:
    """Reference ``PretrainDataset`` (MLGWSC-1/train.py:300-351): item ``idx`` is, with probability ``noise_only_prob``,
    two random noise rows, otherwise ``noise_a + snr * waveforms[idx]`` and ``noise_b + snr * waveforms[idx]`` with one
    snr ~ U(snr_range); ``len`` is ``len(waveforms)``."""

    def __init__(self, noises: torch.Tensor, waveforms: torch.Tensor, snr_range: Tuple[float, float] = (5.0, 15.0),
                 noise_only_prob: float = 0.25, device: str = "cuda"):
        assert 0.0 <= noise_only_prob <= 1.0, "`noise_only_prob` must be in [0,1]"
        if noises.ndim == 2:
            noises = noises.unsqueeze(1)
        if waveforms.ndim == 2:
            waveforms = waveforms.unsqueeze(1)
        assert noises.shape[1:] == waveforms.shape[1:], (
            f"shape mismatch: noises {noises.shape[1:]} vs waveforms {waveforms.shape[1:]}")
        self.noises = noises.to(device=device, dtype=torch.float32)
        self.waveforms = waveforms.to(device=device, dtype=torch.float32)
        self.snr_low, self.snr_high = snr_range
        self.noise_only_prob = noise_only_prob
        self.device = device
        self.rng = np.random.default_rng()

    def __len__(self) -> int:
        return self.waveforms.size(0)

    def plan(self, indices: Sequence[int], rng: Optional[np.random.Generator] = None):
        """(noise row of view 1 [n], noise row of view 2 [n], wave row or -1 [n], snr fp32 [n]) of items ``indices``,
        drawn as ``__getitem__`` draws: ``random()``, then two ``integers(0, len(noises))`` for a noise-only pair, else
        ``uniform(lo, hi)`` and the two ``integers``."""
        rng = self.rng if rng is None else rng
        n = len(indices)
        n1, n2, iw, snr = np.empty(n, np.int64), np.empty(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.float32)
        nn_ = len(self.noises)
        for k, idx in enumerate(indices):
            if rng.random() < self.noise_only_prob:
                n1[k] = int(rng.integers(0, nn_))
                n2[k] = int(rng.integers(0, nn_))
            else:
                iw[k] = int(idx)
                snr[k] = rng.uniform(self.snr_low, self.snr_high)
                n1[k] = int(rng.integers(0, nn_))
                n2[k] = int(rng.integers(0, nn_))
        return n1, n2, iw, snr

    def batch(self, indices: Sequence[int], rng: Optional[np.random.Generator] = None):
        """(X1, X2) [n, D, T] of items ``indices``: both views in ONE device launch."""
        from . import ops
        n1, n2, iw, snr = self.plan(indices, rng)
        x = ops.assemble_batch(self.noises, self.waveforms, np.concatenate((n1, n2)), np.concatenate((iw, iw)),
                               np.concatenate((snr, snr)))
        n = len(indices)
        return x[:n], x[n:]


class ConcatGWData:
    """``ConcatDataset`` of one ``BinaryGWDataset`` per file (MLGWSC-1/train.py:744-773) with all rows in ONE pair of device
    arrays: global item g is item g - offset_k of file k, keeping each file's injections-first labelling."""

    def __init__(self, datasets: Sequence[BinaryGWDataset], device):
        self.datasets = list(datasets)
        self.noises = torch.cat([d.noises.to(torch.float32) for d in self.datasets]).to(device).contiguous()
        self.waveforms = torch.cat([d.waveforms.to(torch.float32) for d in self.datasets]).to(device).contiguous()
        self.cum = np.cumsum([0] + [len(d) for d in self.datasets])
        self.noise_off = self.cum[:-1]
        self.wave_off = np.cumsum([0] + [len(d.waveforms) for d in self.datasets])[:-1]
        self.device = device

    def __len__(self) -> int:
        return int(self.cum[-1])

    def plan(self, indices: Sequence[int], rng: np.random.Generator):
        n = len(indices)
        idx_n, idx_w, snr = np.empty(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.float32)
        for k, g in enumerate(indices):
            f = int(np.searchsorted(self.cum, int(g), side="right")) - 1
            a, b, s = self.datasets[f].plan([int(g) - int(self.cum[f])], rng)
            idx_n[k] = a[0] + self.noise_off[f]
            idx_w[k] = b[0] + self.wave_off[f] if b[0] >= 0 else -1
            snr[k] = s[0]
        return idx_n, idx_w, snr

    def batch(self, indices: Sequence[int], rng: np.random.Generator):
        """(X [n, D, T], one-hot labels [n, 2]) on the device."""
        from . import ops
        idx_n, idx_w, snr = self.plan(indices, rng)
        x = ops.assemble_batch(self.noises, self.waveforms, idx_n, idx_w, snr)
        lab = np.where((idx_w >= 0)[:, None], np.asarray(WAVE_LABEL, np.float32), np.asarray(NOISE_LABEL, np.float32))
        return x, torch.from_numpy(lab.astype(np.float32)).to(self.device)


class DeviceBatches:
    """``DataLoader(dataset, batch_size, shuffle)`` over ``ConcatGWData`` / ``PretrainDataset``: every pass draws its order
    (``shuffle``) and then, batch by batch, the items' random draws from ONE generator, and builds each batch on the device.
    ``reseed``: the generator restarts from ``seed`` at every pass (validation: the same SNRs every epoch)."""

    def __init__(self, dataset, batch_size: int, shuffle: bool, seed: int, reseed: bool = False):
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), shuffle
        self.seed, self.reseed = seed, reseed
        self.rng = np.random.default_rng(seed)

    def __len__(self) -> int:
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        rng = np.random.default_rng(self.seed) if self.reseed else self.rng
        n = len(self.dataset)
        order = rng.permutation(n) if self.shuffle else np.arange(n)
        for i in range(0, n, self.batch_size):
            yield self.dataset.batch(order[i:i + self.batch_size], rng)


# =============================================================================================== pretraining
class ContrastivePretrainer:
    """Reference ``ContrastivePretrainer`` (MLGWSC-1/train.py:377-463): projection ``Linear(d D, proj_dim) -> ReLU ->
    Linear(proj_dim, proj_dim)``, AdamW over adapter + encoder + projection parameters (the frozen base parameters have no
    gradient and take no step), InfoNCE on two views.

    ``_embed`` runs the adapter once per view -- the Q-scan picks its plane over the whole batch of one call, so the two
    views may not share a call -- and then ONE pooled encoder step (``last_token``) over the stacked ``[2 B D]`` feature
    maps: segments are independent in the encoder, so stacking is exact."""

    def __init__(self, q_adapter: nn.Module, whisper_encoder: nn.Module, n_detectors: int, device: str = "cuda",
                 proj_dim: int = 256, lr: float = 1e-4, temperature: float = 0.1):
        self.device = device
        self.q_adapter = q_adapter.to(device)
        self.encoder = whisper_encoder.to(device)
        self.n_detectors = n_detectors
        d_model = whisper_encoder.config.d_model * n_detectors
        self.proj = nn.Sequential(nn.Linear(d_model, proj_dim), nn.ReLU(), nn.Linear(proj_dim, proj_dim)).to(device)
        self.opt = torch.optim.AdamW(list(self.q_adapter.parameters()) + list(self.encoder.parameters())
                                     + list(self.proj.parameters()), lr=lr)
        self.temp = temperature

    def _info_nce(self, z1: torch.Tensor, z2: torch.Tensor) -> torch.Tensor:
        return info_nce(z1, z2, self.temp)

    def _embed(self, *views: torch.Tensor) -> List[torch.Tensor]:
        feats = [self.q_adapter(x) for x in views]                    # [B, D, F, T] each, one Q-scan call per view
        B, D = feats[0].shape[:2]
        flat = torch.cat([f.reshape(B * D, *f.shape[2:]) for f in feats])
        tok = self.encoder.last_token(flat)                           # [V B D, d]: one pooled training step
        return [t.reshape(B, D * t.shape[-1]) for t in tok.split(B * D)]   # == cat over detectors, per view

    def loss(self, X1: torch.Tensor, X2: torch.Tensor) -> torch.Tensor:
        e1, e2 = self._embed(X1, X2)
        return self._info_nce(self.proj(e1), self.proj(e2))

    def step(self, X1: torch.Tensor, X2: torch.Tensor) -> torch.Tensor:
        loss = self.loss(X1, X2)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.detach()

    def train(self, loader, steps: int = 25_000, log_every: int = 100) -> None:
        """``steps`` updates, cycling through ``loader`` (an iterable of ``(X1, X2)``) as the reference does."""
        self.q_adapter.train()
        self.encoder.train()
        it = iter(loader)
        for step in range(steps):
            try:
                X1, X2 = next(it)
            except StopIteration:
                it = iter(loader)
                X1, X2 = next(it)
            loss = self.step(X1.to(self.device), X2.to(self.device))
            if (step + 1) % log_every == 0 or step + 1 == steps:
                logging.info("Contrastive pre-train step %d/%d: loss %.4f", step + 1, steps, float(loss))


# =============================================================================================== fine-tuning
class SupervisedTrainer:
    """Reference ``SupervisedTrainer`` (MLGWSC-1/train.py:478-640): Adam over adapter + ``'lora'`` parameters + classifier,
    ``clip_grad_norm_(model.parameters())``, ``losses.txt``, ``last.pt`` / ``state_dict_e_XXXX.pt`` /
    ``best_state_dict.pt``, the components of the best model, resume ``latest`` | ``best``, early stopping.
    One difference: ``last.pt`` records the best validation loss AFTER the epoch's comparison (the reference stores the
    value before it, so a resumed run can overwrite a better ``best_state_dict.pt``)."""

    def __init__(self, model: nn.Module, device: str, lr: float = 5e-5, clip_norm: float = 100.0,
                 loss_fn: Optional[nn.Module] = None,
                 trainable_param_filter: Optional[Callable[[str, nn.Parameter], bool]] = None):
        self.model = model.to(device)
        self.device = device
        self.clip_norm = clip_norm
        self.loss_fn = loss_fn or RegBCELoss(dim=2)
        params: List[nn.Parameter] = list(self.model.adapter.parameters())
        params += [p for n, p in self.model.encoder.named_parameters() if "lora" in n and p.requires_grad]
        params += list(self.model.classifier.parameters())
        self.optimizer = torch.optim.Adam(params, lr=lr)

    @staticmethod
    def _run_epoch(model, loader, device, loss_fn, optimizer=None, clip_norm: float = 0.0, desc: str = "",
                   log: bool = False) -> float:
        running, batches = 0.0, 0
        is_train = optimizer is not None
        model.train(is_train)
        for X, y in loader:
            X, y = X.to(device), y.to(device)
            with torch.set_grad_enabled(is_train):
                loss = loss_fn(model(X), y)
            if is_train:
                optimizer.zero_grad()
                loss.backward()
                if clip_norm > 0:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=clip_norm)
                optimizer.step()
            running += loss.detach().float().cpu().item()
            batches += 1
        if log:
            logging.info("%s: loss %.6f over %d batches", desc, running / max(1, batches), batches)
        return running / max(1, batches)

    def fit(self, train_loader, valid_loader, outdir: str, epochs: int = 100, resume: Optional[str] = None,
            force: bool = False, early_stop_patience: int = 10) -> None:
        os.makedirs(outdir, exist_ok=True)
        losses_path = os.path.join(outdir, "losses.txt")
        if os.path.isfile(losses_path) and not force:
            raise RuntimeError(f"Output file exists: {losses_path}")
        start_epoch, best_val = 1, float("inf")
        if resume:
            start_epoch, best_val = self._resume(outdir, resume)
        patience = 0
        with open(losses_path, "a", buffering=1) as f:
            for epoch in range(start_epoch, epochs + 1):
                train_loss = self._run_epoch(self.model, train_loader, self.device, self.loss_fn, optimizer=self.optimizer,
                                             clip_norm=self.clip_norm, desc=f"Train {epoch}", log=True)
                val_loss = self._run_epoch(self.model, valid_loader, self.device, self.loss_fn, optimizer=None,
                                           clip_norm=0.0, desc=f"Valid {epoch}", log=True)
                f.write(f"{epoch:04d}\t{train_loss:.6f}\t{val_loss:.6f}\n")
                improved = val_loss < best_val
                if improved:
                    best_val = val_loss
                torch.save({"epoch": epoch, "best_val_loss": best_val, "model_state": self.model.state_dict(),
                            "optimizer_state": self.optimizer.state_dict()}, os.path.join(outdir, "last.pt"))
                torch.save(self.model.state_dict(), os.path.join(outdir, f"state_dict_e_{epoch:04d}.pt"))
                if improved:
                    torch.save(self.model.state_dict(), os.path.join(outdir, "best_state_dict.pt"))
                    patience = 0
                    logging.info(f"New best @ epoch {epoch:04d} — val_loss={val_loss:.6e}")
                    save_model_components(outdir, adapter=self.model.adapter, peft_model=self.model.encoder,
                                          dense_layers=self.model.classifier, adapter_path="best_adapter.pt",
                                          lora_weights_path="best_lora_weights", dense_layers_path="best_dense_layers.pth")
                else:
                    patience += 1
                    if patience >= early_stop_patience:
                        logging.info(f"Early stopping (patience {early_stop_patience}) at epoch {epoch:04d}.")
                        break
        logging.info(f"Training complete. Best validation loss: {best_val:.6f}")

    def _resume(self, outdir: str, which: str) -> Tuple[int, float]:
        """``best``: the model from ``best_state_dict.pt``, epoch 1, no optimizer state; ``latest``: model + optimizer from
        ``last.pt``, the epoch after it.  A missing file starts fresh (with a warning), as in the reference."""
        if which == "best":
            path = os.path.join(outdir, "best_state_dict.pt")
            if not os.path.isfile(path):
                logging.warning("No best_state_dict.pt found; starting fresh.")
                return 1, float("inf")
            self.model.load_state_dict(torch.load(path, map_location=self.device))
            logging.info("Resumed model from best_state_dict.pt (optimizer not restored).")
            return 1, float("inf")
        last_path = os.path.join(outdir, "last.pt")
        if not os.path.isfile(last_path):
            logging.warning("No last.pt found; starting fresh.")
            return 1, float("inf")
        payload = torch.load(last_path, map_location=self.device)
        self.model.load_state_dict(payload["model_state"])
        if payload.get("optimizer_state"):
            self.optimizer.load_state_dict(payload["optimizer_state"])
        logging.info("Resumed model+optimizer from last.pt.")
        return payload.get("epoch", 1) + 1, payload.get("best_val_loss", float("inf"))


# =============================================================================================== builders
LORA_PATTERNS = ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj",
                 "layers.*.self_attn.out_proj"]


def apply_lora(encoder: nn.Module, r: int = 8, alpha: int = 32, use_dora: bool = True,
               patterns: Optional[List[str]] = None) -> nn.Module:
    """Reference ``apply_lora`` (MLGWSC-1/train.py:666-702): LoRA / DoRA on the attention projections matched by
    ``patterns`` (q, k, v and out_proj by default), base parameters frozen, ``'lora'`` parameters trainable."""
    from .peft import LoraConfig, get_peft_model
    module_names = [name for name, _ in encoder.named_modules()]
    matched = [m for p in (patterns or LORA_PATTERNS) for m in fnmatch.filter(module_names, p)]
    logging.info(f"LoRA targeting modules: {matched}")
    peft_encoder = get_peft_model(encoder, LoraConfig(use_dora=use_dora, r=r, lora_alpha=alpha, target_modules=matched))
    for name, param in peft_encoder.named_parameters():
        param.requires_grad = "lora" in name
    return peft_encoder


def build_network(encoder: nn.Module, adapter: nn.Module, n_detectors: int, num_classes: int, device) -> GWWhisperClassifier:
    model = GWWhisperClassifier(encoder, n_detectors=n_detectors, num_classes=num_classes, adapter=adapter).to(device)
    total = sum(p.numel() for p in model.parameters())
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    logging.info(f"Total params: {total:,} | Trainable: {trainable:,} ({100 * trainable / total:.2f}%)")
    return model


def save_model_components(results_path: str, adapter: nn.Module, peft_model: nn.Module, dense_layers: nn.Module,
                          adapter_path: str, lora_weights_path: str, dense_layers_path: str) -> None:
    """Reference ``save_model_components`` (MLGWSC-1/train.py:723-737): what ``run_inference.py --adapter-weights
    --lora-weights --dense-weights`` reads."""
    os.makedirs(results_path, exist_ok=True)
    torch.save(adapter.state_dict(), os.path.join(results_path, adapter_path))
    peft_model.save_pretrained(os.path.join(results_path, lora_weights_path))
    torch.save(dense_layers.state_dict(), os.path.join(results_path, dense_layers_path))
    logging.info("Saved components: adapter, LoRA weights, dense layers.")
