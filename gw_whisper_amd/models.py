"""Counterparts of the reference's model wrappers (the callers of the hot path).

Same names, constructor arguments, ``nn.Sequential`` layouts (so the shipped ``.pth`` heads
load unchanged -- SURVEY.md appendix A) and forward semantics as

  * ``Signal_vs_Noise/src/model.py:4-29``   two_channel_ligo_binary_classifier
  * ``Signal_vs_Noise/src/model.py:31-52``  one_channel_ligo_binary_classifier
  * ``Signal_vs_Noise/src/model.py:57-85``  TwoChannelLIGOBinaryClassifierCNN (the conv chain runs in HIP, csrc/cnn_head.hip)
  * ``Glitch_classification/src/model.py:4-39``  (multi-class head with Dropout(0.3))
  * ``Signal_vs_Noise/Efficiency_test/src/network.py:69-90``  efficiency_classifier (2-way Softmax head)

The reference's own classes also work unchanged on a ``gw_whisper_amd`` encoder (they only
call ``encoder(mel).last_hidden_state[:, -1, :]`` and read ``encoder.config.d_model``);
these copies exist because the reference tree does not travel to the GPU box, and they use
the encoder's ``last_token`` fast path when it is available (inference: only token 1499 goes
through the final LayerNorm; training: the last layer's row-wise ops and their backward run on
the pooled rows only).  The MLP heads are plain ``torch.nn`` on the GPU unless a trainer asks for their HIP
step (``binary.head_bce_with_logits`` on ``pooled(...)``, ``glitch.head_cross_entropy``, ``efficiency.reg_bce_head``); the
CNN head is HIP.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import GwwError


def _pooled(encoder, mel):
    fast = getattr(encoder, "last_token", None)
    if fast is not None:
        return fast(mel)
    return encoder(mel).last_hidden_state[:, -1, :]


def linear_params(classifier, slots, needs):
    """[weight, bias, weight, bias, ...] of the ``nn.Linear`` modules in ``slots`` of a head's ``nn.Sequential``; a
    classifier of another layout is a ``GwwError`` with the text ``needs``."""
    try:
        return [t for i in slots for t in (classifier[i].weight, classifier[i].bias)]
    except (IndexError, AttributeError, TypeError) as e:
        raise GwwError(needs) from e


class two_channel_ligo_binary_classifier(nn.Module):
    def __init__(self, encoder, num_classes=1):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Sequential(
            nn.Linear(self.encoder.config.d_model * 2, 1024), nn.ReLU(),
            nn.Linear(1024, 512), nn.ReLU(),
            nn.Linear(512, 256), nn.ReLU(),
            nn.Linear(256, num_classes))

    def pooled(self, mel_tensor_0, mel_tensor_1):
        """[B, 2 d_model]: what ``forward`` feeds the classifier (the input of ``binary.head_bce_with_logits``)"""
        n = mel_tensor_0.shape[0]
        both = _pooled(self.encoder, torch.cat((mel_tensor_0, mel_tensor_1), dim=0))
        return torch.cat((both[:n], both[n:]), dim=1)

    def forward(self, mel_tensor_0, mel_tensor_1):
        # both detectors share the encoder weights: one pass over the stacked batch (same arithmetic
        # as the reference's two sequential calls, segments are independent)
        n = mel_tensor_0.shape[0]
        both = _pooled(self.encoder, torch.cat((mel_tensor_0, mel_tensor_1), dim=0))
        return self.classifier(torch.cat((both[:n], both[n:]), dim=1))


CNN_SLOTS = (0, 2, 4, 8)   # the parameter slots of TwoChannelLIGOBinaryClassifierCNN.classifier


class _CnnHead(torch.autograd.Function):
    """``ops.cnn_head_forward`` / ``ops.cnn_head_backward`` behind autograd: dx goes on into the pooled tokens of both
    detectors, the eight parameter gradients to the classifier."""

    @staticmethod
    def forward(ctx, x, *params):
        from . import ops
        logits, ctx.head_saved = ops.cnn_head_forward(x.detach(), [p.detach() for p in params], train=True)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        from . import ops
        dx, grads = ops.cnn_head_backward(ctx.head_saved, dlogits.contiguous())
        return (dx, *grads)


class TwoChannelLIGOBinaryClassifierCNN(nn.Module):
    """``Signal_vs_Noise/src/model.py:57-85``: the pooled tokens of the two detectors stacked to [B, 2, d_model], three
    ``Conv1d(k=3, pad=1)`` + ReLU over the length d_model, the mean, a ``Linear``.  ``classifier`` has the reference's
    slots (its ``state_dict`` loads there and the reference's here).  ``head="hip"`` runs the chain in HIP, forward and
    backward (csrc/cnn_head.hip: exact fp32, bit-reproducible, independent of the batch); ``head="torch"`` runs
    ``self.classifier`` as plain ``torch.nn``."""

    def __init__(self, encoder, num_classes=1, head="hip"):
        super().__init__()
        if head not in ("hip", "torch"):
            raise GwwError(f"TwoChannelLIGOBinaryClassifierCNN: head={head!r} must be 'hip' or 'torch'")
        self.encoder = encoder
        self.head = head
        self.classifier = nn.Sequential(
            nn.Conv1d(2, 64, kernel_size=3, stride=1, padding=1), nn.ReLU(),
            nn.Conv1d(64, 128, kernel_size=3, stride=1, padding=1), nn.ReLU(),
            nn.Conv1d(128, 256, kernel_size=3, stride=1, padding=1), nn.ReLU(),
            nn.AdaptiveAvgPool1d(1), nn.Flatten(),
            nn.Linear(256, num_classes))

    def head_params(self):
        return linear_params(self.classifier, CNN_SLOTS, "the CNN head needs the reference's nn.Sequential: Conv1d at 0, 2, 4 "
                                                         "and Linear at 8")

    def decode(self, x):
        """logits [B, C] of the stacked pooled tokens x [B, 2, d_model]"""
        if self.head == "torch":
            return self.classifier(x)
        from . import ops
        params = self.head_params()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _CnnHead.apply(x, *params)
        return ops.cnn_head_forward(x, [p.detach() for p in params])

    def forward(self, mel_tensor_0, mel_tensor_1):
        n = mel_tensor_0.shape[0]
        both = _pooled(self.encoder, torch.cat((mel_tensor_0, mel_tensor_1), dim=0))
        return self.decode(torch.stack((both[:n], both[n:]), dim=1))


class one_channel_ligo_binary_classifier(nn.Module):
    def __init__(self, encoder, num_classes=1):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Sequential(
            nn.Linear(self.encoder.config.d_model, 512), nn.ReLU(),
            nn.Linear(512, 256), nn.ReLU(),
            nn.Linear(256, 128), nn.ReLU(),
            nn.Linear(128, 64), nn.ReLU(),
            nn.Linear(64, num_classes))

    def pooled(self, mel_tensor_0):
        """[B, d_model]: what ``forward`` feeds the classifier (the input of ``binary.head_bce_with_logits``)"""
        return _pooled(self.encoder, mel_tensor_0)

    def forward(self, mel_tensor_0):
        return self.classifier(_pooled(self.encoder, mel_tensor_0))


class glitch_classifier(nn.Module):
    """``Glitch_classification/src/model.py:4-39`` (there also named
    ``one_channel_ligo_binary_classifier``): d -> 512 -> 256 -> 128 -> C with Dropout(0.3)."""

    def __init__(self, encoder, num_classes):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Sequential(
            nn.Linear(self.encoder.config.d_model, 512), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(512, 256), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(256, 128), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(128, num_classes))

    def forward(self, mel_tensor_0):
        return self.classifier(_pooled(self.encoder, mel_tensor_0))


class efficiency_classifier(nn.Module):
    """``Signal_vs_Noise/Efficiency_test/src/network.py:69-90`` (there also named
    ``one_channel_ligo_binary_classifier``): d -> 512 -> 256 -> 128 -> 64 -> C with a trailing ``Softmax(dim=1)``, slots
    ``0 2 4 6 8`` as there, so the reference's ``dense_layers_*.pth`` load unchanged."""

    def __init__(self, encoder, num_classes=2):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Sequential(
            nn.Linear(self.encoder.config.d_model, 512), nn.ReLU(),
            nn.Linear(512, 256), nn.ReLU(),
            nn.Linear(256, 128), nn.ReLU(),
            nn.Linear(128, 64), nn.ReLU(),
            nn.Linear(64, num_classes), nn.Softmax(dim=1))

    def forward(self, mel_tensor_0):
        return self.classifier(_pooled(self.encoder, mel_tensor_0))
