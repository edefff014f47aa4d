"""Search background from time slides: one encoder pass, the head per slide.

A two-detector search estimates its false-alarm rate from data in which no astrophysical signal can be coincident:
detector 0's data paired with detector 1's data shifted by more than any physical delay, many times over.  In
``GWWhisperClassifier`` adapter, whitening and encoder run per detector and the detectors only meet in the head, so the
score of the pair (detector-0 window ``i``, detector-1 window ``j``) is ``classifier(cat(tok0[i], tok1[j]))`` on the tokens
the zero-lag pass computes anyway.  The head's first ``Linear`` splits over the concatenation, ``W1 = [W1_0 | W1_1 | ...]``:
its partial products are computed once per window (``head_partials``), and what is left per pair is
``relu(P0[i] + P1[j])`` through 512 -> 256 -> 128 -> 64 -> C (``csrc/timeslide.hip``).

Semantics.  With ``k = slide_shift / step_size`` windows, slide ``s = 1..S`` has offset ``o_s = s k`` and detector ``g`` of
pair ``(i, s)`` reads window ``(i + g o_s) mod N``, circular within a segment of ``N`` windows; detector 0 is never moved
and a slid score carries the time stamp of its window.  A slide exists for a segment only if ``k <= o_s <= N - k`` (no wrap
back towards zero lag); its live time is the sum of ``N_seg * time_step_size`` over the segments it exists for.  Each slide
is thresholded and clustered exactly as ``inference.get_clusters`` does one trigger list; slides and segments never share
a cluster.

The background is the HEAD's response to pairs.  It equals a physically shifted rerun of the whole search only because
everything in front of the head is per detector."""

from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import GwwError

HEAD_WIDTHS = (512, 256, 128, 64)
BYTE_BUDGET = 1 << 30     # scores plus event buffers of one chunk of slides (slide_background)


class SlidePlan(NamedTuple):
    """What ``slide_plan`` returns.  ``slides`` / ``offsets``: the slide numbers (1-based) that exist for the segment and
    their window offsets; ``livetime`` fp64 [n_slides]: seconds of background slide s + 1 adds (0 where it does not exist)."""
    k: int
    n_slides: int
    slides: Tuple[int, ...]
    offsets: Tuple[int, ...]
    livetime: np.ndarray


def slide_plan(n_windows: int, step_size: float, slide_shift: float, n_slides: int, slice_seconds: float,
               time_step_size: float | None = None) -> SlidePlan:
    """The slides of one segment of ``n_windows`` windows (host only).  ``slice_seconds``: the length of a window
    (``slice_length * delta_t``).  ``time_step_size``: the seconds a window step really covers
    (``DeviceSegmentSlicer.time_step_size``; default ``step_size``), what live time is counted in."""
    if n_slides < 1:
        raise GwwError(f"slide_plan: n_slides={n_slides} must be >= 1")
    if not step_size > 0:
        raise GwwError(f"slide_plan: step_size={step_size} must be positive")
    ratio = slide_shift / step_size
    k = int(round(ratio))
    if k < 1 or abs(ratio - k) > 1e-9:
        raise GwwError(f"slide_plan: slide_shift={slide_shift} must be a whole number of steps of {step_size} s "
                       f"(slide_shift / step_size = {ratio!r})")
    if not slide_shift > slice_seconds:
        raise GwwError(f"slide_plan: slide_shift={slide_shift} s must exceed the window length {slice_seconds} s, or a pair "
                       "would hold the same second of sky twice")
    n = int(n_windows)
    step = float(step_size if time_step_size is None else time_step_size)
    slides = tuple(s for s in range(1, n_slides + 1) if k <= s * k <= n - k)
    live = np.zeros((n_slides,), np.float64)
    for s in slides:
        live[s - 1] = n * step
    return SlidePlan(k, int(n_slides), slides, tuple(s * k for s in slides), live)


def head_layers(classifier) -> Tuple[List[nn.Linear], bool]:
    """(the five ``nn.Linear`` of the search head, whether a Softmax follows): ``GWWhisperClassifier.classifier`` with or
    without its Softmax -- Linear / ReLU alternating, widths 512 / 256 / 128 / 64 / C.  Anything else is refused."""
    if not isinstance(classifier, nn.Sequential):
        raise GwwError("time_slides: the head must be the nn.Sequential of GWWhisperClassifier")
    mods = list(classifier.children())
    softmax = bool(mods) and isinstance(mods[-1], nn.Softmax)
    if softmax:
        mods = mods[:-1]
    ok = len(mods) == 9 and all(isinstance(m, nn.Linear if i % 2 == 0 else nn.ReLU) for i, m in enumerate(mods))
    lin = mods[0::2] if ok else []
    if ok:
        ok = tuple(l.out_features for l in lin[:4]) == HEAD_WIDTHS and 1 <= lin[4].out_features <= 64 \
            and all(l.bias is not None for l in lin) \
            and all(lin[i + 1].in_features == lin[i].out_features for i in range(4))
    if not ok:
        raise GwwError("time_slides: the head must be five Linear layers of widths 512 / 256 / 128 / 64 / C (C <= 64) with "
                       "ReLU between them and at most a trailing Softmax")
    return lin, softmax


def _tokens(tokens, lin0):
    if not torch.is_tensor(tokens) or tokens.dim() != 3 or tokens.dtype != torch.float32:
        raise GwwError("time_slides: tokens must be an fp32 tensor [N, D, d]")
    N, D, d = tokens.shape
    if D < 2 or D > ops.SLIDE_MAX_D:
        raise GwwError(f"time_slides: D={D} detectors; time slides need 2..{ops.SLIDE_MAX_D}")
    if lin0.in_features != D * d:
        raise GwwError(f"time_slides: the head takes {lin0.in_features} features, the tokens give D * d = {D * d}")
    if N < 1:
        raise GwwError("time_slides: no windows")
    if not tokens.is_cuda:
        raise GwwError("time_slides: tokens must live on the GPU; gw_whisper_amd has no CPU path")
    return N, D, d


def head_partials(tokens: torch.Tensor, classifier) -> torch.Tensor:
    """fp32 [D, N, 512]: ``tokens[:, g] @ W1[:, g d:(g + 1) d]^T`` per detector (D fp32 ``ops.gemm`` calls on the column
    blocks of ``classifier[0].weight``), the bias folded into detector 0."""
    lin, _ = head_layers(classifier)
    N, D, d = _tokens(tokens, lin[0])
    w = lin[0].weight.detach().to(torch.float32)
    out = torch.empty((D, N, HEAD_WIDTHS[0]), dtype=torch.float32, device=tokens.device)
    for g in range(D):
        bias = lin[0].bias.detach().to(torch.float32) if g == 0 else None
        out[g] = ops.gemm(tokens[:, g, :].contiguous(), w[:, g * d:(g + 1) * d].contiguous(), bias, 0)
    return out


def _tail_params(lin):
    return [t.detach().to(torch.float32).contiguous() for l in lin[1:] for t in (l.weight, l.bias)]


def slide_scores(tokens: torch.Tensor, classifier, offsets: Sequence[int], softmax: bool = False) -> torch.Tensor:
    """fp32 [S, N]: row s is the head's score of ``cat_g tokens[(i + g * offsets[s]) mod N, g]`` for every window i --
    ``z[0]`` of the head without its Softmax, or ``softmax(z)[0]`` with ``softmax``."""
    lin, _ = head_layers(classifier)
    if softmax and lin[4].out_features < 2:
        raise GwwError("time_slides: the softmax score needs C >= 2 classes")
    return ops.slide_scores(head_partials(tokens, classifier), _tail_params(lin), offsets,
                            ops.SLIDE_PROB0 if softmax else ops.SLIDE_LOGIT0)


def cluster_capacity(times_host: np.ndarray, cluster_threshold: float) -> int:
    """Clusters one trigger list over these stamps can hold at most: two neighbouring clusters lie more than
    ``cluster_threshold`` apart and the gaps between them are disjoint parts of the segment, so there are at most
    ``1 + span / cluster_threshold`` of them, and never more than windows."""
    n = len(times_host)
    if n == 0 or not cluster_threshold > 0:
        return max(1, n)
    return max(1, min(n, 1 + int((times_host[-1] - times_host[0]) / cluster_threshold)))


def slide_background(slicer, tokens: torch.Tensor, classifier, plan: SlidePlan, trigger_threshold: float,
                     cluster_threshold: float, byte_budget: int = BYTE_BUDGET):
    """The clustered background events of one segment: ``(time, stat, var, slide)`` as numpy arrays (fp64, fp64, fp64,
    int32; ``slide`` the 1-based slide number), slide after slide, each in time order.  ``tokens`` [N, D, d] are the
    segment's (``evaluate_slices(..., return_tokens=True)``), ``plan`` its ``slide_plan``.  The score is ``softmax(z)[0]``
    when ``classifier`` still ends in its Softmax, otherwise ``z[0]``.  The slides are processed in chunks whose scores
    (4 N bytes per slide) plus event buffers (12 bytes per possible cluster) stay under ``byte_budget`` bytes."""
    lin, softmax = head_layers(classifier)
    N = _tokens(tokens, lin[0])[0]
    if N != len(slicer):
        raise GwwError(f"slide_background: {N} tokens for a segment of {len(slicer)} windows")
    empty = (np.zeros((0,), np.float64), np.zeros((0,), np.float64), np.zeros((0,), np.float64), np.zeros((0,), np.int32))
    if not plan.offsets:
        return empty
    if softmax and lin[4].out_features < 2:
        raise GwwError("time_slides: the softmax score needs C >= 2 classes")
    partials = head_partials(tokens, classifier)
    params = _tail_params(lin)
    times_host = slicer.times_host(0, N)
    times = torch.from_numpy(times_host).to(tokens.device)
    cap = cluster_capacity(times_host, cluster_threshold)
    per_slide = 4 * N + 12 * cap + 4
    chunk = max(1, min(len(plan.offsets), ops.SLIDE_MAX_S, int(byte_budget) // per_slide))
    parts = []
    for c0 in range(0, len(plan.offsets), chunk):
        offs, ids = plan.offsets[c0:c0 + chunk], plan.slides[c0:c0 + chunk]
        scores = ops.slide_scores(partials, params, offs, ops.SLIDE_PROB0 if softmax else ops.SLIDE_LOGIT0)
        out_t, out_v, cnt = ops.cluster_slides(times, scores, trigger_threshold, cluster_threshold, cap)
        counts = cnt.cpu().numpy()
        if (counts > cap).any():
            raise GwwError(f"slide_background: a slide holds {int(counts.max())} clusters, more than the {cap} slots")
        if counts.sum() == 0:
            continue
        t, v = out_t.cpu().numpy(), out_v.cpu().numpy()
        for r, (sid, c) in enumerate(zip(ids, counts)):
            parts.append((t[r, :c], v[r, :c].astype(np.float64), np.full((c,), sid, np.int32)))
    if not parts:
        return empty
    time, stat, slide = (np.concatenate([p[j] for p in parts]) for j in range(3))
    return time, stat, np.full(time.shape, 0.2), slide
