"""The binary heads of the signal-vs-noise trainers (the reference's ``Signal_vs_Noise/src/train.py`` and
``src/sd_train.py``) as one HIP step: ``classifier(pooled)`` + ``BCEWithLogitsLoss`` forward and backward in four launches
(``csrc/binary_head.hip``), exact fp32, identical bits on identical calls, no host synchronisation.

Two layouts, read off the classifier's ``nn.Sequential``:
  * ``models.one_channel_ligo_binary_classifier``  Linear at slots 0 2 4 6 8, d -> 512 -> 256 -> 128 -> 64 -> C
  * ``models.two_channel_ligo_binary_classifier``  Linear at slots 0 2 4 6,   2 d -> 1024 -> 512 -> 256 -> C
"""

from __future__ import annotations

import torch

from . import _lib

_SLOTS = ((1, (0, 2, 4, 6, 8)), (2, (0, 2, 4, 6)))     # (ops.BIN_HEAD_*, the Linear slots)
_NEEDS = ("the binary head step needs the nn.Sequential of models.one_channel_ligo_binary_classifier (Linear at slots "
          "0 2 4 6 8 with ReLU between: d -> 512 -> 256 -> 128 -> 64 -> C) or of models.two_channel_ligo_binary_classifier "
          "(Linear at slots 0 2 4 6: d -> 1024 -> 512 -> 256 -> C)")


def head_layout(classifier):
    """(layout, parameters) of a binary classifier's ``nn.Sequential``: ``ops.BIN_HEAD_ONE`` / ``ops.BIN_HEAD_TWO`` and its
    ``nn.Linear`` tensors [w1, b1, ...] in order.  Any other module is a ``GwwError`` that names the two layouts."""
    from .models import linear_params
    from .ops import BIN_HEAD_WIDTHS
    try:
        n = len(classifier)
    except TypeError as e:
        raise _lib.GwwError(_NEEDS) from e
    for layout, slots in _SLOTS:
        if n != 2 * len(slots) - 1:
            continue
        if not all(isinstance(classifier[i], torch.nn.Linear) for i in slots):
            break
        if not all(isinstance(classifier[i], torch.nn.ReLU) for i in range(1, n, 2)):
            break
        params = linear_params(classifier, slots, _NEEDS)
        widths = tuple(w.shape[0] for w in params[0:-2:2])
        if widths != BIN_HEAD_WIDTHS[layout] or any(a.shape[1] != b.shape[0] for a, b in zip(params[2::2], params[0::2])):
            break
        return layout, params
    raise _lib.GwwError(_NEEDS)


class _HeadBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, targets, layout, *params):
        from . import ops
        loss, logits, _probs, _row_loss, saved = ops.bin_head_forward(layout, pooled.to(torch.float32),
                                                                      [t.detach() for t in params], targets)
        ctx.saved, ctx.in_dtype = saved, pooled.dtype
        ctx.mark_non_differentiable(logits)
        return loss.reshape(()), logits

    @staticmethod
    def backward(ctx, g_loss, _g_logits):
        from . import ops
        dx, grads = ops.bin_head_backward(ctx.saved, g_loss.to(torch.float32))
        ctx.saved = None
        return (dx.to(ctx.in_dtype), None, None, *grads)


def head_bce_with_logits(classifier, pooled: torch.Tensor, labels: torch.Tensor):
    """``BCEWithLogitsLoss()(classifier(pooled), labels)`` -> (loss, logits) in four HIP launches for forward + backward.
    ``classifier`` is the ``nn.Sequential`` of one of the two binary classifiers; its parameters receive their gradients
    through autograd as usual, ``pooled`` [B, d_in] its own.  ``labels``: [B, C] floats in [0, 1].  The logits are returned
    for metrics and carry no gradient."""
    if not pooled.is_cuda or not labels.is_cuda:
        raise _lib.GwwError("head_bce_with_logits needs GPU tensors: gw_whisper_amd has no CPU path")
    layout, params = head_layout(classifier)
    return _HeadBCE.apply(pooled, labels.to(torch.float32), layout, *params)


def head_logits(classifier, pooled: torch.Tensor):
    """``classifier(pooled)`` in one launch, inference only (no gradient): the bits of ``head_bce_with_logits``'s logits."""
    from . import ops
    if not pooled.is_cuda:
        raise _lib.GwwError("head_logits needs GPU tensors: gw_whisper_amd has no CPU path")
    layout, params = head_layout(classifier)
    return ops.bin_head_scores(layout, pooled.detach().to(torch.float32), [t.detach() for t in params])
