"""The reference's glitch-classification programs (``Glitch_classification/src/train.py``, ``train_full_finetune.py``,
``evaluate.py``) on the MI355X path: the pieces ``harness/run_glitch_train.py`` and ``harness/run_glitch_evaluate.py``
are built from.

    modify_label / fit_classes / encode_labels  <->  train.py:144-151 (label transformation + sklearn LabelEncoder order)
    head_cross_entropy        the classifier head + ``CrossEntropyLoss`` as ONE autograd Function over the HIP kernels of
                              ``csrc/classify.hip`` (2 launches forward, 2 backward); reads the parameters of the same
                              ``nn.Sequential`` ``models.glitch_classifier`` builds, so ``.pth`` heads load unchanged
    EvalState                 confusion matrix, loss sum and count in device buffers (``gww_eval_accumulate``), read once
    classification_report / macro_f1 / confusion_scores   sklearn's report (``zero_division=0``) from the C x C matrix
    build_model / evaluate_model / load_split             what both programs share
"""

from __future__ import annotations

import fnmatch
import os
from typing import List, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["modify_label", "fit_classes", "encode_labels", "head_cross_entropy", "EvalState", "classification_report",
           "macro_f1", "confusion_scores", "build_model", "evaluate_model", "load_split", "synthetic_split",
           "DEFAULT_LORA_TARGETS"]

# the adapted modules of the reference (train.py:162; o_proj matches nothing in HF Whisper)
DEFAULT_LORA_TARGETS = ("layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj",
                        "layers.*.self_attn.o_proj")


# =============================================================================================== labels
def modify_label(label: str) -> str:
    """train.py:147: ``"GW" if label == "GW" else " ".join(label.split("_")).title()``."""
    return "GW" if label == "GW" else " ".join(label.split("_")).title()


def fit_classes(raw_labels: Sequence[str]) -> List[str]:
    """The classes ``sklearn.preprocessing.LabelEncoder().fit`` finds on the modified labels: sorted unique strings
    (code-point order: ``"1080 Lines" < "Blip" < ... < "GW" < "Koi Fish"``)."""
    return sorted(set(modify_label(str(l)) for l in raw_labels))


def encode_labels(raw_labels: Sequence[str], classes: Sequence[str]) -> np.ndarray:
    """``LabelEncoder.transform`` of the modified labels: int64 class indices; an unseen label is a ``ValueError``."""
    index = {c: i for i, c in enumerate(classes)}
    out = np.empty(len(raw_labels), np.int64)
    for i, l in enumerate(raw_labels):
        m = modify_label(str(l))
        if m not in index:
            raise ValueError(f"y contains previously unseen labels: {m!r}")
        out[i] = index[m]
    return out


# =============================================================================================== the HIP head step
_NEEDS = "head_cross_entropy needs the nn.Sequential of models.glitch_classifier (Linear ReLU Dropout x 3, Linear)"


def _head_parameters(classifier):
    """The eight ``nn.Linear`` tensors and the dropout probability of ``glitch_classifier.classifier`` (slots 0 3 6 9)."""
    from .models import linear_params
    params = linear_params(classifier, (0, 3, 6, 9), _NEEDS)
    if not isinstance(classifier[2], torch.nn.Dropout):
        raise _lib.GwwError(_NEEDS)
    return params, float(classifier[2].p)


class _HeadCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, labels, p, train, seed, offset, *params):
        from . import ops
        loss, logits, _row_loss, _pred, saved = ops.head_forward(pooled.to(torch.float32), [t.detach() for t in params],
                                                                 labels, p, train, seed, offset)
        ctx.saved, ctx.in_dtype = saved, pooled.dtype
        ctx.mark_non_differentiable(logits)
        return loss.reshape(()), logits

    @staticmethod
    def backward(ctx, g_loss, _g_logits):
        from . import ops
        dx, grads = ops.head_backward(ctx.saved, g_loss.to(torch.float32))
        ctx.saved = None
        return (dx.to(ctx.in_dtype), None, None, None, None, None, *grads)


def head_cross_entropy(classifier, pooled: torch.Tensor, labels: torch.Tensor, seed: int = 0, offset: int = 0):
    """``CrossEntropyLoss()(classifier(pooled), labels)`` -> (loss, logits) in four HIP launches for forward + backward
    (``csrc/classify.hip``), exact fp32, identical bits on identical calls.  ``classifier`` is the ``nn.Sequential`` of
    ``models.glitch_classifier``; its parameters receive their gradients through autograd as usual, ``pooled`` [B, d_model]
    its own.  Dropout is applied when ``classifier.training``; the mask is a counter-based function of (seed, offset,
    layer, element) -- pass the step number as ``offset`` -- and is NOT torch's mask (``ops.head_dropout_mask`` returns
    it).  The logits are returned for metrics and carry no gradient."""
    if not pooled.is_cuda or not labels.is_cuda:
        raise _lib.GwwError("head_cross_entropy needs GPU tensors: gw_whisper_amd has no CPU path")
    params, p = _head_parameters(classifier)
    return _HeadCE.apply(pooled, labels.to(torch.int64), p, bool(classifier.training), int(seed), int(offset), *params)


class EvalState:
    """Evaluation state kept on the device: ``add`` is one launch per batch and never synchronises, ``read`` copies the
    three buffers to the host once."""

    def __init__(self, n_classes: int, device):
        self.n_classes = n_classes
        self.confusion = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros((1,), dtype=torch.float64, device=device)
        self.n = torch.zeros((1,), dtype=torch.int64, device=device)

    def add(self, logits, labels, row_loss):
        from . import ops
        ops.eval_accumulate(logits, labels, row_loss, self.confusion, self.loss_sum, self.n)

    def read(self):
        """(confusion [C, C] int64 numpy, sum of the row losses, number of rows)."""
        return self.confusion.cpu().numpy(), float(self.loss_sum.item()), int(self.n.item())


# =============================================================================================== metrics
def confusion_scores(cm):
    """(precision, recall, f1, support, present) per class from the confusion matrix (rows = true class) with
    ``zero_division=0``; ``present`` marks the classes that occur in the truth or the predictions -- the label set
    sklearn's ``unique_labels(y_true, y_pred)`` gives."""
    cm = np.asarray(cm, dtype=np.int64)
    tp = np.diag(cm).astype(np.float64)
    pred = cm.sum(axis=0).astype(np.float64)
    true = cm.sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred > 0, tp / pred, 0.0)
        rec = np.where(true > 0, tp / true, 0.0)
        den = prec + rec
        f1 = np.where(den > 0, 2.0 * prec * rec / den, 0.0)
    return prec, rec, f1, cm.sum(axis=1), (pred + true) > 0


def macro_f1(cm) -> float:
    """``sklearn.metrics.f1_score(y_true, y_pred, average="macro")`` from the confusion matrix."""
    _, _, f1, _, present = confusion_scores(cm)
    return float(np.mean(f1[present])) if present.any() else 0.0


def classification_report(cm, class_names: Sequence[str], digits: int = 2) -> str:
    """``sklearn.metrics.classification_report(y_true, y_pred, target_names=class_names, zero_division=0)`` from the
    confusion matrix, character for character.  Like sklearn it lists the classes that occur in the truth or the
    predictions; where sklearn raises because a named class occurs in neither, that class is left out here."""
    cm = np.asarray(cm, dtype=np.int64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] != len(class_names) or cm.shape[0] > 64:
        raise ValueError(f"classification_report: confusion matrix {cm.shape} for {len(class_names)} class names (C <= 64)")
    prec, rec, f1, sup, present = confusion_scores(cm)
    idx = np.flatnonzero(present)
    names = [str(class_names[i]) for i in idx]
    width = max([len(n) for n in names] + [len("weighted avg"), digits])
    report = ("{:>{width}s} " + " {:>9}" * 4).format("", "precision", "recall", "f1-score", "support", width=width) + "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for i, n in zip(idx, names):
        report += row_fmt.format(n, prec[i], rec[i], f1[i], int(sup[i]), width=width, digits=digits)
    report += "\n"
    total = int(sup[idx].sum())
    acc = float(np.diag(cm).sum()) / total if total else 0.0
    report += ("{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n").format(
        "accuracy", "", "", acc, total, width=width, digits=digits)
    w = sup[idx].astype(np.float64)
    for heading, avg in (("macro avg", lambda v: float(np.mean(v[idx])) if len(idx) else 0.0),
                         ("weighted avg", lambda v: float(np.sum(v[idx] * w) / w.sum()) if w.sum() > 0 else 0.0)):
        report += row_fmt.format(heading, avg(prec), avg(rec), avg(f1), total, width=width, digits=digits)
    return report


# =============================================================================================== data
def load_concatenated_dataset(data_path: str):
    """train.py:26-35: ``chunk*`` sub-directories concatenated in sorted order, else the directory itself."""
    from datasets import concatenate_datasets, load_from_disk
    chunks = sorted(os.path.join(data_path, d) for d in os.listdir(data_path)
                    if os.path.isdir(os.path.join(data_path, d)) and "chunk" in d)
    if chunks:
        return concatenate_datasets([load_from_disk(c) for c in chunks])
    return load_from_disk(data_path)


def load_split(data_path: str, concatenated: bool = True):
    """(data [n, L] float32, raw label strings, SNR [n] float32) of a dataset with the reference's columns ``data``,
    ``labels``, ``SNR`` (dataset.py:41-43)."""
    if concatenated:
        ds = load_concatenated_dataset(data_path)
    else:
        from datasets import load_from_disk
        ds = load_from_disk(data_path)      # evaluate.py:81 reads the directory itself
    return (np.asarray(ds["data"], np.float32), [str(l) for l in ds["labels"]], np.asarray(ds["SNR"], np.float32))


def synthetic_split(n: int, n_classes: int, seed: int, test: bool = False):
    """``--synthetic N``: N seeded training segments, or (``test``) the N // 4 (at least n_classes) test segments of
    the same classes from another seed; raw label strings as a dataset would carry them."""
    from . import synth
    if test:
        n, seed = max(n // 4, n_classes), seed + 1000003
    wave, cls, snr = synth.glitch_segments(n, n_classes, seed=seed)
    names = synth.glitch_class_names(n_classes)
    return wave, [names[c] for c in cls], snr


# =============================================================================================== model
def build_model(encoder_name: str, n_classes: int, method: str, lora_rank: int = 8, lora_alpha: int = 32,
                precision: str = "bf16", lora_targets: Sequence[str] = DEFAULT_LORA_TARGETS, encoder_weights: str = None,
                seed: int = 0, device="cuda"):
    """train.py:159-186 / train_full_finetune.py / evaluate.py:16-36: encoder -> fnmatch target search ->
    ``LoraConfig(use_dora=...)`` -> ``get_peft_model`` -> ``requires_grad = 'lora' in name`` -> ``glitch_classifier``;
    ``full_finetune``: the bare encoder through ``enable_full_finetune()``, every parameter trainable."""
    from . import synth
    from .encoder import WhisperConfig, WhisperEncoder
    from .models import glitch_classifier
    from .peft import LoraConfig, get_peft_model
    if method not in ("DoRA", "LoRA", "full_finetune"):
        raise ValueError(f"--method {method}: expected DoRA, LoRA or full_finetune")
    d, L, H, F = synth.ENCODER_SIZES[encoder_name]
    config = WhisperConfig.named(encoder_name)
    encoder = WhisperEncoder(config, precision=precision)
    if encoder_weights:
        if encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            encoder.load_state_dict(load_file(encoder_weights))
        else:
            encoder.load_state_dict(torch.load(encoder_weights, map_location="cpu"))
    else:
        sd = synth.encoder_state_dict(d, L, H, F, seed=seed, n_mels=config.num_mel_bins)
        encoder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    if method == "full_finetune":
        body = encoder.enable_full_finetune().to(device)      # refuses precision='fp32' with the encoder's own error
    else:
        names = [n for n, _ in encoder.named_modules()]
        matched = [m for pat in lora_targets for m in fnmatch.filter(names, pat)]
        body = get_peft_model(encoder, LoraConfig(use_dora=method == "DoRA", r=lora_rank, lora_alpha=lora_alpha,
                                                  target_modules=matched)).to(device)
        for name, p in body.named_parameters():
            p.requires_grad = "lora" in name
    model = glitch_classifier(body, num_classes=n_classes).to(device)
    if method == "full_finetune":
        for p in model.parameters():
            p.requires_grad = True
    return model


def evaluate_model(model, wave: np.ndarray, labels: np.ndarray, batch_size: int, head: str, n_mels: int = 80):
    """Eval-mode pass over ``wave`` in dataset order.  Returns (loss, confusion [C, C] int64) with loss the mean of the
    per-batch mean losses (train.py:76: ``total_loss / len(data_loader)``).  ``head="hip"``: the HIP head forward and the
    device accumulate, ONE host read at the end; ``head="torch"``: the reference's loop (``loss.item()`` and
    ``argmax(...).cpu()`` per batch)."""
    from . import ops
    from .models import _pooled
    device = next(model.parameters()).device
    n_classes = model.classifier[9].out_features
    model.eval()
    y_all = torch.from_numpy(np.asarray(labels, np.int64)).to(device)
    n_batches = 0
    with torch.no_grad():
        if head == "hip":
            state, batch_losses = EvalState(n_classes, device), []
            params, p = _head_parameters(model.classifier)
            for i in range(0, len(wave), batch_size):
                mel = ops.logmel(torch.from_numpy(wave[i:i + batch_size]).to(device), n_mels=n_mels)
                y = y_all[i:i + batch_size]
                loss, logits, row_loss, _pred, _ = ops.head_forward(_pooled(model.encoder, mel).to(torch.float32),
                                                                    [t.detach() for t in params], y, p, False)
                state.add(logits, y, row_loss)
                batch_losses.append(loss)
                n_batches += 1
            cm, _loss_sum, _n = state.read()
            total = float(torch.cat(batch_losses).double().sum().item()) if batch_losses else 0.0
        elif head == "torch":
            criterion = torch.nn.CrossEntropyLoss()
            cm, total = np.zeros((n_classes, n_classes), np.int64), 0.0
            for i in range(0, len(wave), batch_size):
                mel = ops.logmel(torch.from_numpy(wave[i:i + batch_size]).to(device), n_mels=n_mels)
                y = y_all[i:i + batch_size]
                logits = model(mel).float()
                total += criterion(logits, y).item()
                preds = torch.argmax(logits, dim=1).cpu().numpy()
                np.add.at(cm, (np.asarray(labels[i:i + batch_size], np.int64), preds), 1)
                n_batches += 1
        else:
            raise ValueError(f"--head {head}: expected hip or torch")
    return total / max(n_batches, 1), cm
