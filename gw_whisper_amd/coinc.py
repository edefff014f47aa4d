"""Single-detector search: per-detector events, coincidences and a slid background on the device.

A single-detector model (``models.one_channel_ligo_binary_classifier``, what ``run_train.py --detectors 1`` trains) scores
every window of every detector on its own.  Each detector's scores are thresholded and clustered into events exactly as
``inference.get_clusters`` does one trigger list (``ops.cluster_slides``, one row per detector), and only then do the
detectors meet: ``ops.coinc_slides`` pairs detector 0's events with detector 1's at zero lag and under S time slides
(``csrc/coinc.hip``).

Semantics, for one segment of ``N`` windows and the detectors H1 = 0, L1 = 1.  With the events ``t_g`` fp64 ascending and
``v_g`` fp32 and a shift ``o`` in seconds, ``d(i, j) = (t_1[j] + o) - t_0[i]`` in fp64 -- one addition, then one
subtraction -- and i, j are coincident iff ``fabs(d) <= window``.  Every detector-0 event gets at most one partner: of its
coincident j the largest ``v_1[j]``, then the smallest ``fabs(d)``, then the smallest j.  A coincidence carries
``time = t_0[i]`` (detector 0 is never moved), ``stat = double(v_0[i]) + double(v_1[j])`` and ``dt = d(i, j)``.  The search
requires ``2 * window < cluster_threshold``: neighbouring events of one detector lie more than ``cluster_threshold`` apart,
so no detector-1 event can then be coincident with two detector-0 events and the matching is one to one.

Slides are NOT circular.  With ``k = slide_shift / step_size`` steps, slide ``s = 1..S`` shifts detector 1 by
``o_s = s k time_step_size`` seconds; it exists iff ``o_s < N time_step_size - slice_seconds`` and its live time is
``N time_step_size - o_s``, the overlap of the segment with its shifted copy.  (A wrap would bring the first and the last
event of a segment next to each other and break the one-to-one property.)  ``slide_shift > slice_seconds + window``, or a
slid pair could hold the same second of sky.

Every detector's events are final before any pairing, so a slide IS a shift of event times: this background is that of a
physically shifted rerun of the search by construction (``time_slides.py`` has to argue it for the head's inputs)."""

from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import GwwError

BYTE_BUDGET = 1 << 30     # partner table plus event buffers of one chunk of slides (search_segment)
EVENT_VAR = 0.2           # the time variance every event of the search carries (inference.get_clusters)


# ------------------------------------------------------------------------------------------------ host oracle
def coinc_host(t0, v0, t1, v1, shifts, window: float) -> dict:
    """The numpy restatement of the semantics above (host only, fp64): per shift a bisection on the predicate
    ``d(i, j) >= -window`` for the first candidate of every i, then the walk over the candidates under the partner rule.
    Returns what ``ops.coinc_slides`` returns, as numpy arrays: ``offsets`` int64 [S + 1], ``time``, ``stat``, ``dt`` fp64,
    ``idx0``, ``idx1`` int32."""
    t0, t1 = np.ascontiguousarray(t0, np.float64), np.ascontiguousarray(t1, np.float64)
    v0, v1 = np.ascontiguousarray(v0, np.float32), np.ascontiguousarray(v1, np.float32)
    shifts = np.atleast_1d(np.asarray(shifts, np.float64))
    window = np.float64(window)
    n0, n1 = len(t0), len(t1)
    if v0.shape != t0.shape or v1.shape != t1.shape or t0.ndim != 1 or t1.ndim != 1:
        raise GwwError("coinc_host: t0 / v0 and t1 / v1 must be vectors of equal length")
    offsets = np.zeros((len(shifts) + 1,), np.int64)
    cols = []
    rows = np.arange(n0)
    for s, o in enumerate(shifts):
        best = np.full((n0,), -1, np.int64)
        if n0 and n1:
            lo, hi = np.zeros((n0,), np.int64), np.full((n0,), n1, np.int64)
            while True:                                   # the first j with d(i, j) >= -window, for every i at once
                act = lo < hi
                if not act.any():
                    break
                mid = lo + ((hi - lo) >> 1)
                d = (t1[np.minimum(mid, n1 - 1)] + o) - t0
                ge = d >= -window
                hi = np.where(act & ge, mid, hi)
                lo = np.where(act & ~ge, mid + 1, lo)
            bv, bd = np.zeros((n0,), np.float32), np.zeros((n0,), np.float64)
            alive, j = np.ones((n0,), bool), lo.copy()
            while True:                                   # the candidates in ascending j, until d leaves the window
                alive &= j < n1
                if not alive.any():
                    break
                jj = np.minimum(j, n1 - 1)
                ad = np.fabs((t1[jj] + o) - t0)
                alive &= ad <= window
                v = v1[jj]
                take = alive & ((best < 0) | (v > bv) | ((v == bv) & (ad < bd)))
                best, bv, bd = np.where(take, jj, best), np.where(take, v, bv), np.where(take, ad, bd)
                j = j + 1
        i = rows[best >= 0]
        jb = best[i]
        cols.append((t0[i], v0[i].astype(np.float64) + v1[jb].astype(np.float64), (t1[jb] + o) - t0[i],
                     i.astype(np.int32), jb.astype(np.int32)))
        offsets[s + 1] = offsets[s] + len(i)
    names = ("time", "stat", "dt", "idx0", "idx1")
    out = {k: np.concatenate([c[n] for c in cols]) if cols else np.zeros((0,)) for n, k in enumerate(names)}
    out["offsets"] = offsets
    return out


# ------------------------------------------------------------------------------------------------ the slides of a segment
class CoincPlan(NamedTuple):
    """What ``slide_shifts`` returns.  ``slides`` / ``shifts``: the slide numbers (1-based) that exist for the segment and
    the seconds each adds to detector 1's event times; ``livetime`` fp64 [n_slides]: seconds of background slide s + 1 adds
    (0 where it does not exist)."""
    k: int
    n_slides: int
    slides: Tuple[int, ...]
    shifts: Tuple[float, ...]
    livetime: np.ndarray


def slide_shifts(n_windows: int, step_size: float, slide_shift: float, n_slides: int, slice_seconds: float,
                 time_step_size: float | None = None, window: float = 0.0) -> CoincPlan:
    """The non-circular slides of one segment of ``n_windows`` windows (host only).  ``slice_seconds``: the length of a
    window; ``time_step_size``: the seconds a window step really covers (``DeviceSegmentSlicer.time_step_size``; default
    ``step_size``), what shifts and live time are counted in; ``window``: the coincidence window the slides will be searched
    with."""
    if n_slides < 1:
        raise GwwError(f"slide_shifts: n_slides={n_slides} must be >= 1")
    if not step_size > 0:
        raise GwwError(f"slide_shifts: step_size={step_size} must be positive")
    if not window >= 0:
        raise GwwError(f"slide_shifts: window={window} must not be negative")
    ratio = slide_shift / step_size
    k = int(round(ratio))
    if k < 1 or abs(ratio - k) > 1e-9:
        raise GwwError(f"slide_shifts: slide_shift={slide_shift} must be a whole number of steps of {step_size} s "
                       f"(slide_shift / step_size = {ratio!r})")
    if not slide_shift > slice_seconds + window:
        raise GwwError(f"slide_shifts: slide_shift={slide_shift} s must exceed the window length plus the coincidence window, "
                       f"{slice_seconds} + {window} s, or a slid pair could hold the same second of sky")
    n = int(n_windows)
    step = float(step_size if time_step_size is None else time_step_size)
    span = n * step
    slides, shifts = [], []
    live = np.zeros((n_slides,), np.float64)
    for s in range(1, n_slides + 1):
        o = (s * k) * step
        if o < span - slice_seconds:
            slides.append(s)
            shifts.append(o)
            live[s - 1] = span - o
    return CoincPlan(k, int(n_slides), tuple(slides), tuple(shifts), live)


# ------------------------------------------------------------------------------------------------ scores of every detector
def _features(windows: torch.Tensor, frontend) -> torch.Tensor:
    """[b, D, L] cut windows -> features [D * b, n_mels, n_frames], detector-major: as ``real_events.scan_events`` makes
    them (``frontend=None``: resample to 16 kHz + Whisper's published log-mel)."""
    from .inference import resample
    b, D, L = windows.shape
    rows = windows.permute(1, 0, 2).reshape(D * b, L)
    if frontend is not None:
        return ops.logmel(rows.contiguous(), config=frontend)
    return ops.logmel(resample(rows, L * 16000 // 2048))


def _logits(model, mel: torch.Tensor) -> torch.Tensor:
    """fp32 [n]: the model's (first) logit of every row of features -- ``classifier(pooled(mel))``, the head in one HIP
    launch (``binary.head_logits``), the encoder on the ``last_token`` path ``pooled`` takes."""
    from .binary import head_logits
    return head_logits(model.classifier, model.pooled(mel))[:, 0]


def _models(model, D: int):
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    if len(models) not in (1, D):
        raise GwwError(f"detector_scores: {len(models)} models for {D} detector(s): one shared model or one per detector")
    for m in models:
        if not (hasattr(m, "pooled") and hasattr(m, "classifier")):
            raise GwwError("detector_scores: a single-detector model (models.one_channel_ligo_binary_classifier) has "
                           "pooled() and classifier")
    return models


def detector_scores(slicer, model, batch_size: int = 256, frontend=None) -> torch.Tensor:
    """fp32 [D, N] on the device: the logit of every window of every detector of ``slicer`` under a single-detector model.
    ``model``: one model -- the windows of all detectors go through the encoder stacked in ONE batch of D * b rows,
    detector-major, as ``GWWhisperClassifier.embed_features`` stacks them -- or a sequence of D models, one pass each.
    ``frontend``: an ``ops.FrontendConfig`` whose ``n_samples`` is the window -- the features come from
    ``ops.logmel_windows`` on the rows of ``slicer.dss``, no window is cut; ``None``: ``inference.resample`` to 16 kHz and
    ``ops.logmel``, on the cut windows."""
    D, N = int(slicer.dss.shape[0]), len(slicer)
    models = _models(model, D)
    if N < 1:
        raise GwwError("detector_scores: the segment holds no window")
    if batch_size < 1:
        raise GwwError(f"detector_scores: batch_size={batch_size} must be >= 1")
    if frontend is not None and frontend.n_samples != slicer.slice_length:
        raise GwwError(f"detector_scores: frontend.n_samples is {frontend.n_samples} but the slicer's windows hold "
                       f"{slicer.slice_length} samples: the front end's chunk must be the window")
    out = torch.empty((D, N), dtype=torch.float32, device=slicer.dss.device)
    with torch.no_grad():
        for i0 in range(0, N, batch_size):
            i1 = min(N, i0 + batch_size)
            b = i1 - i0
            if frontend is not None:
                mel = ops.logmel_windows(slicer.dss, frontend, slicer.index_step_size, w0=i0, n_windows=b, rows_major=True)
                mel = mel.reshape(D * b, *mel.shape[2:])
            else:
                mel = _features(slicer.windows(i0, i1), None)
            if len(models) == 1:
                out[:, i0:i1] = _logits(models[0], mel).to(torch.float32).reshape(D, b)
            else:
                for g, m in enumerate(models):
                    out[g, i0:i1] = _logits(m, mel[g * b:(g + 1) * b]).to(torch.float32)
    return out


# ------------------------------------------------------------------------------------------------ one segment
def detector_events(slicer, scores: torch.Tensor, trigger_threshold: float, cluster_threshold: float):
    """The clustered events of every row of ``scores`` [D, N]: (t fp64 [D, cap], v fp32 [D, cap], count int32 [D]) on the
    device (``ops.cluster_slides`` with one row per detector) and the counts on the host -- one read of 4 D bytes."""
    from .time_slides import cluster_capacity
    N = len(slicer)
    if scores.dim() != 2 or scores.shape[1] != N:
        raise GwwError(f"detector_events: scores {tuple(scores.shape)} for a segment of {N} windows")
    times_host = slicer.times_host(0, N)
    cap = cluster_capacity(times_host, cluster_threshold)
    t, v, cnt = ops.cluster_slides(torch.from_numpy(times_host).to(scores.device), scores, trigger_threshold,
                                   cluster_threshold, cap)
    counts = cnt.cpu().numpy()
    if (counts > cap).any():
        raise GwwError(f"detector_events: a detector holds {int(counts.max())} events, more than the {cap} slots")
    return t, v, cnt, counts


def search_segment(slicer, model, trigger_threshold: float, cluster_threshold: float, window: float,
                   plan: CoincPlan | None = None, batch_size: int = 256, frontend=None, byte_budget: int = BYTE_BUDGET,
                   scores: torch.Tensor | None = None):
    """The coincident search of one segment: foreground ``(time, stat, var)`` and background ``(time, stat, var, slide)``
    as numpy arrays (fp64, fp64, fp64, int32; ``var`` = 0.2, ``slide`` the 1-based slide number), the background slide after
    slide, each in time order.  ``plan``: the segment's ``slide_shifts`` (None: no background).  ``scores``: fp32 [D, N] from
    an earlier ``detector_scores`` call instead of a new pass.  Host reads: the D event counts once, then ONE copy per chunk
    of slides -- the chunks sized so that the partner table (4 bytes per detector-0 event and slide) and the event buffers
    (32 bytes per possible coincidence) stay under ``byte_budget`` bytes; zero lag travels with the first chunk.
    With one detector there are no pairs: its own events are the foreground, and slides are refused."""
    D = int(slicer.dss.shape[0])
    empty_bg = (np.zeros((0,), np.float64), np.zeros((0,), np.float64), np.zeros((0,), np.float64), np.zeros((0,), np.int32))
    if D not in (1, 2):
        raise GwwError(f"search_segment: {D} detectors; the coincident search pairs two (or lists the events of one)")
    if D == 1 and plan is not None:
        raise GwwError("search_segment: time slides pair the events of two detectors; with one detector there is nothing to "
                       "slide against, and its background cannot be estimated this way")
    if D == 2:
        if not window >= 0:
            raise GwwError(f"search_segment: window={window} must not be negative")
        if not 2 * window < cluster_threshold:
            raise GwwError(f"search_segment: 2 * window = {2 * window} s must be less than cluster_threshold = "
                           f"{cluster_threshold} s, or one event could be coincident with two events of the other detector")
    if scores is None:
        scores = detector_scores(slicer, model, batch_size, frontend)
    elif tuple(scores.shape) != (D, len(slicer)) or scores.dtype != torch.float32 or not scores.is_cuda:
        raise GwwError(f"search_segment: scores must be fp32 [{D}, {len(slicer)}] on the GPU")
    t, v, _, counts = detector_events(slicer, scores, trigger_threshold, cluster_threshold)
    if D == 1:
        n = int(counts[0])
        time = t[0, :n].cpu().numpy()
        return (time, v[0, :n].cpu().numpy().astype(np.float64), np.full(time.shape, EVENT_VAR)), empty_bg
    n0, n1 = int(counts[0]), int(counts[1])
    shifts = [0.0] + list(plan.shifts if plan is not None else ())
    ids = [0] + list(plan.slides if plan is not None else ())
    per_slide = min(n0, n1)                     # one to one: a slide holds at most this many coincidences
    chunk = max(1, min(ops.COINC_MAX_S, int(byte_budget) // max(1, 4 * n0 + 8 + 32 * per_slide)))
    fg, parts = None, []
    for c0 in range(0, len(shifts), chunk):
        sh, sid = shifts[c0:c0 + chunk], ids[c0:c0 + chunk]
        S = len(sh)
        r = ops.coinc_slides(t[0], v[0], n0, t[1], v[1], n1, torch.tensor(sh, dtype=torch.float64).to(scores.device), window,
                             cap_total=S * per_slide)
        host = torch.cat((r["offsets"].view(torch.float64), r["time"], r["stat"])).cpu().numpy()     # the chunk's one read
        offs = host[:S + 1].view(np.int64)
        cap = S * per_slide
        if offs[S] > cap:
            raise GwwError(f"search_segment: {int(offs[S])} coincidences in {S} slides, more than the {cap} a one-to-one "
                           "matching allows")
        time, stat = host[S + 1:S + 1 + cap], host[S + 1 + cap:]
        for k, s in enumerate(sid):
            a, b = int(offs[k]), int(offs[k + 1])
            if s == 0:
                fg = (time[a:b].copy(), stat[a:b].copy(), np.full((b - a,), EVENT_VAR))
            elif b > a:
                parts.append((time[a:b], stat[a:b], np.full((b - a,), s, np.int32)))
    if not parts:
        return fg, empty_bg
    time, stat, slide = (np.concatenate([p[j] for p in parts]) for j in range(3))
    return fg, (time, stat, np.full(time.shape, EVENT_VAR), slide)
