"""Scoring a search (the reference's ``MLGWSC-1/evaluate.py``) on the device: clustered events against the injections ->
the false-alarm rate and the sensitive distance of the MLGWSC-1 challenge.

``get_stats`` has the reference's signature and returns its sixteen keys.  Sorting, searching, compaction, the best
statistic per injection, the rates and the volumes run in ``csrc/score.hip``; the arithmetic is integer counting plus a few
fp64 operations in the reference's order, so every key equals numpy's bit for bit except the chirp-mass-weighted sums,
which are sums of many positive terms taken in another (fixed) order.  The events may be the
device tensors ``inference.cluster_triggers_device`` works on: nothing goes through the host on the way in, and the device
is read once at the end.

Kept on the host, on purpose: ``sensitive-distance = (3 vol / (4 pi)) ** (1 / 3)`` is one elementwise numpy expression
over the ``vol`` array that is read back anyway -- a device ``pow`` would differ from numpy's in the last bits for no gain
--, and the per-injection weights ``mchirp ** 2.5`` / ``mchirp ** 5`` and the scalars (duration, Ninj, prefactor) are O(N)
input preparation in the reference's own expressions.

Two quirks of the reference are reproduced: ``found-indices`` is the closest injection of EVERY sorted event (length E,
true positive or not), and ``missed-indices`` its complement -- an injection only false positives point at is in neither
the found injections nor ``missed-indices``.  The reference's sort of the false positives' statistics changes no output
(``fg-far`` depends on their number only) and is not repeated.

Refused with ``GwwError`` instead of the reference's silent or obscure failures: ``tc`` not ascending (the reference
sorts a copy and then indexes the unsorted array), NaNs in times or statistics, no foreground event or no true positive at
all (the reference dies with an IndexError), CPU tensors, more than 2^27 events."""

from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import GwwError

KEYS = ("fg-events", "found-indices", "missed-indices", "true-positive-event-indices", "false-positive-event-indices",
        "sorting-indices", "true-positive-diffs", "false-positive-diffs", "true-positives", "false-positives", "fg-far", "far",
        "sensitive-volume", "sensitive-distance", "sensitive-volume-error", "sensitive-fraction")


def mchirp(mass1, mass2):
    """The chirp mass (``evaluate.py:100-101``)."""
    return (mass1 * mass2) ** (3. / 5.) / (mass1 + mass2) ** (1. / 5.)


def _ascending(tc, who):
    tc = np.ascontiguousarray(np.asarray(tc, np.float64).reshape(-1))
    if tc.size == 0:
        raise GwwError(f"{who}: no injection times")
    if np.isnan(tc).any():
        raise GwwError(f"{who}: the injection times hold NaN")
    if tc.size > 1 and not bool(np.all(tc[1:] >= tc[:-1])):
        raise GwwError(f"{who}: the injection times tc are not ascending")
    return tc


def find_closest_index(array, value):
    """``find_closest_index`` of the reference (``evaluate.py:66-97``) on the device: for every value the index of the
    closest element of the ascending ``array``; of two equally close neighbours the right one.  numpy in, int64 out."""
    tc = _ascending(array, "find_closest_index")
    v = np.ascontiguousarray(np.asarray(value, np.float64))
    if v.size == 0:
        return np.zeros(v.shape, np.int64)
    if np.isnan(v).any():
        raise GwwError("find_closest_index: the values hold NaN")
    idx, _ = ops.score_closest(torch.from_numpy(tc).cuda(), torch.from_numpy(v.reshape(-1)).cuda())
    return idx.cpu().numpy().astype(np.int64).reshape(v.shape)


def find_injection_times(segments, injtimes, padding_start=0, padding_end=0):
    """``find_injection_times`` of the reference (``evaluate.py:13-63``) over segment lists instead of open files:
    ``segments`` = (start_time, n_samples, delta_t) per foreground segment.  Returns (the total duration of all segments,
    the bool mask of the injections inside a segment shortened by the paddings).  Host code: file bookkeeping."""
    injtimes = np.asarray(injtimes)
    duration = 0
    times = []
    for start, n, dt in segments:
        end = start + n * dt
        duration += end - start
        start = start + padding_start
        end = end - padding_end
        if end > start:
            times.append([start, end])
    ret = np.full((len(times), len(injtimes)), False)
    for i, (start, end) in enumerate(times):
        ret[i] = np.logical_and(start <= injtimes, injtimes <= end)
    return duration, np.any(ret, axis=0)


def _events(ev, name, device=None):
    """[3, n] fp64 on the device from numpy or a CUDA tensor."""
    if torch.is_tensor(ev):
        if not ev.is_cuda:
            raise GwwError(f"get_stats: {name} is a CPU tensor; pass numpy or a GPU tensor (gw_whisper_amd has no CPU path)")
        if ev.dtype != torch.float64:
            raise GwwError(f"get_stats: {name} must be torch.float64, got {ev.dtype}")
    else:
        ev = np.asarray(ev, np.float64)
    if ev.ndim != 2 or ev.shape[0] != 3:
        raise GwwError(f"get_stats: {name} must be [3, n] (time, stat, var), got {tuple(ev.shape)}")
    if ev.shape[1] > ops.SCORE_MAX_N:
        raise GwwError(f"get_stats: {name} holds {ev.shape[1]} events, more than 2^27")
    if torch.is_tensor(ev):
        return ev.contiguous()
    return torch.from_numpy(np.ascontiguousarray(ev)).to(device if device is not None else "cuda")


def get_stats(fgevents, bgevents, injparams, duration=None, chirp_distance=False, background_duration=None):
    """``get_stats`` of the reference (``evaluate.py:104-278``): fgevents, bgevents [3, n] (time, stat, var) as numpy or
    CUDA fp64 tensors, injparams a dict of numpy arrays with ``tc`` (ascending), ``distance`` and, for
    ``chirp_distance``, ``mass1`` / ``mass2``.  Returns the reference's sixteen keys as numpy arrays (integers int64).
    ``background_duration``: the seconds of background the events in ``bgevents`` were found in, when that is not the
    foreground's ``duration`` (time slides, ``time_slides.py``): ``far`` is counted per that time; ``fg-far`` and every
    other key keep ``duration``."""
    tc = _ascending(injparams["tc"], "get_stats")
    dist = np.asarray(injparams["distance"], np.float64)
    N = tc.size
    if dist.shape != (N,):
        raise GwwError(f"get_stats: distance must be [N = {N}] as tc is")
    if N > ops.SCORE_MAX_N:
        raise GwwError(f"get_stats: {N} injections, more than 2^27")
    fg = _events(fgevents, "fgevents", bgevents.device if torch.is_tensor(bgevents) and bgevents.is_cuda else None)
    bg = _events(bgevents, "bgevents", fg.device)
    dev = fg.device
    E, B = fg.shape[1], bg.shape[1]
    if E == 0:
        raise GwwError("get_stats: no foreground events")
    if duration is None:
        duration = tc.max() - tc.min()
    if background_duration is not None and not float(background_duration) > 0:
        raise GwwError(f"get_stats: background_duration={background_duration} must be positive")
    # the scalars and per-injection weights, in the reference's own expressions (evaluate.py:233-242, 256-261)
    max_distance = dist.max()
    vtot = (4. / 3.) * np.pi * max_distance**3.
    if chirp_distance:
        massc = mchirp(np.asarray(injparams["mass1"], np.float64), np.asarray(injparams["mass2"], np.float64))
        if massc.shape != (N,):
            raise GwwError(f"get_stats: mass1 and mass2 must be [N = {N}] as tc is")
        mchirp_max = massc.max()
        mc_norm = mchirp_max ** (5. / 2.) * len(massc)
        n_inj = np.sum((mchirp_max / massc) ** (5. / 2.))
        w1 = torch.from_numpy(np.ascontiguousarray(massc ** (5. / 2.))).to(dev)
        w2 = torch.from_numpy(np.ascontiguousarray(massc ** 5)).to(dev)
    else:
        mc_norm = n_inj = len(dist)
    prefactor = vtot / mc_norm

    order, _, nan_t = ops.score_sort(fg[0])
    m = ops.score_match(fg, order, torch.from_numpy(tc).to(dev))
    counts = m["counts"]
    n_found = counts[2:3]
    fg_far = ops.score_far(E, duration, dev, n_dev=counts[1:2])
    f_order, f_sorted, _ = ops.score_sort(m["found_stat"], n_dev=n_found)
    nan_b = None
    if B > 0:
        _, noise, nan_b = ops.score_sort(bg[1])
        far = ops.score_far(B, duration if background_duration is None else float(background_duration), dev)
        cs1 = cs2 = None
        if chirp_distance:
            cs1, cs2 = ops.score_suffix(w1, w2, m["found_inj"], f_order, n_found)
        nfound, frac, vol, vol_err = ops.score_volume(f_sorted, n_found, noise, n_inj, prefactor, cs1, cs2)

    # the one read of the device
    n_tp, n_fp, n_f, n_m, n_nan = (int(v) for v in counts.cpu().numpy())
    n_nan += int(nan_t.item()) + (int(nan_b.item()) if nan_b is not None else 0)
    if n_nan > 0:
        raise GwwError("get_stats: the event times or statistics hold NaN")
    if n_tp == 0 or n_f == 0:
        raise GwwError(f"get_stats: no true positive among the {E} foreground events: no injection was found")

    def host(t, dtype=None):
        a = t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)
    ret = {}
    ret["fg-events"] = host(m["fg_sorted"])
    ret["found-indices"] = host(m["found_idx"], np.int64)
    ret["missed-indices"] = host(m["missed"][:n_m], np.int64)
    ret["true-positive-event-indices"] = host(m["tp_idx"][:n_tp], np.int64)
    ret["false-positive-event-indices"] = host(m["fp_idx"][:n_fp], np.int64)
    ret["sorting-indices"] = host(order, np.int64)
    ret["true-positive-diffs"] = host(m["tp_diff"][:n_tp])
    ret["false-positive-diffs"] = host(m["fp_diff"][:n_fp])
    ret["true-positives"] = host(m["tp_events"][:, :n_tp])
    ret["false-positives"] = host(m["fp_events"][:, :n_fp])
    ret["fg-far"] = host(fg_far[:n_fp])
    if B > 0:
        ret["far"] = host(far)
        v = host(vol)
        ret["sensitive-volume"] = v
        ret["sensitive-distance"] = (3 * v / (4 * np.pi))**(1. / 3.)
        ret["sensitive-volume-error"] = host(vol_err)
        ret["sensitive-fraction"] = host(frac)
    else:
        for k in ("far", "sensitive-volume", "sensitive-distance", "sensitive-volume-error", "sensitive-fraction"):
            ret[k] = np.zeros((0,), np.float64)
    return ret
