"""The test stage of the efficiency study (the reference's ``Signal_vs_Noise/Efficiency_test/src/test_network.py`` and
``evaluate_test_data.py``) on the device: windows -> the network's two outputs, and a long series of ranking statistics ->
triggers -> clustered events -> false-alarm rate and sensitive distance.

    score_windows   <->  test_network.py:111-149: resample, log-mel, encoder, both columns of the head
    triggers        <->  bnslib.py:216-240 ``get_triggers``
    events          <->  evaluate_test_data.py:261-319, 389-407 (``get_cluster_boundaries``, ``custom_get_event_list_from_triggers``)
    statistics      <->  evaluate_test_data.py:28-87, 546-612 (true / false positives, ranking steps, volumes)
    evaluate        the three chained; no count goes through the host in between, the device is read once at the end
    TimeSeries / assemble_time_series   <->  the (data, delta_t, epoch) container and evaluate_test_data.py:374-387

The kernels are ``csrc/trigger_stats.hip`` plus the sort and nearest-injection search of ``csrc/score.hip``.  The
arithmetic is comparing, counting, searching and a few fp64 operations in the reference's order, so every output equals
the reference's bit for bit, except ``sens-dist``:

Kept on the host, on purpose: ``sens-dist = (3 vol / (4 pi)) ** (1 / 3)`` is one elementwise numpy expression over the
``sens-vol`` array that is read back anyway (the reference takes the power of numpy scalars, whose last bits differ from
the array power's: the one output held to a tolerance), and the scalar ``prefactor`` in the reference's own expression.

Reproduced quirk: the false-alarm count of the FIRST ranking step is ``n`` when its run of equal values has length one and
``n - b - 1`` (b = the run's last position) otherwise, as every later step's is: the reference writes ``n - 0`` for the
first false positive and only a later equal value overwrites it.

Not computed: ``base_fidxs`` (``get_closest_injection_times``, evaluate_test_data.py:586).  The reference uses its length
only, which is the number of true positives; and the true / false positives' TIMES are not carried through the sorts,
because no output reads them.

Clusters: a trigger opens a cluster iff it is the first or ``t[j] - t[j-1] >= cluster_tolerance``; the reference's loop
compares against the last trigger taken into the cluster, which is always the previous one.  The trigger times must
ascend (``triggers`` gives them so); host arrays are checked, device tensors are taken on trust.

Refused with ``GwwError``: a NaN in the series, the injection times or the event values; no injection; ``duration <= 0``;
CPU tensors; more than 2^27 samples; more triggers than the ``capacity`` the caller set; and no true positive at all --
``NoTruePositive``, which carries the triggers and events found so far (``.partial``) because the reference writes those
two files before it dies on ``tptimes, tpvals = tp.T``.  That includes a series without any trigger.  ``triggers`` and
``events`` on their own return empty arrays for it, and no false positive gives empty statistics arrays."""

from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import GwwError

SEC_PER_MONTH = 30 * 24 * 60 * 60
STAT_KEYS = ("ranking", "far", "sens-frac", "sens-dist", "sens-vol", "sens-vol-err")
MAX_N = ops.TRIG_MAX_N


class NoTruePositive(GwwError):
    """No event lies within the tolerance of an injection.  ``partial``: {"triggers": (times, values), "events": (times,
    values)} as numpy arrays, as far as the call computed them."""

    def __init__(self, msg, partial=None):
        super().__init__(msg)
        self.partial = partial or {}


# =============================================================================================== the container
_NS = 1000000000


def _to_ns(t) -> int:
    """Seconds -> integer nanoseconds (LIGOTimeGPS semantics: whole seconds plus rounded nanoseconds)."""
    if isinstance(t, GPSTime):
        return t.ns
    t = float(t)
    sec = int(np.floor(t))
    return sec * _NS + int(round((t - sec) * 1e9))


class GPSTime:
    """An epoch as integer nanoseconds; sums and differences are exact.  ``float()`` is the whole seconds plus
    ``nanoseconds * 1e-9`` -- ``ns * 1e-9`` for a difference below one second, and exact for a GPS-sized epoch such as
    1238166018.75, which the product ``ns * 1e-9`` of all its nanoseconds is not."""
    __slots__ = ("ns",)

    def __init__(self, t=0, ns=None):
        self.ns = _to_ns(t) if ns is None else int(ns)

    def __float__(self):
        return float(self.ns // _NS) + (self.ns % _NS) * 1e-9

    def __add__(self, other):
        return GPSTime(ns=self.ns + _to_ns(other))

    __radd__ = __add__

    def __sub__(self, other):
        return GPSTime(ns=self.ns - _to_ns(other))

    def __lt__(self, other):
        return self.ns < _to_ns(other)

    def __le__(self, other):
        return self.ns <= _to_ns(other)

    def __eq__(self, other):
        return self.ns == _to_ns(other)

    def __hash__(self):
        return hash(self.ns)

    def __repr__(self):
        return f"GPSTime({float(self)!r})"


class TimeSeries:
    """What the reference uses of ``pycbc.types.TimeSeries``: (data, delta_t, epoch), ``start_time`` / ``end_time`` /
    ``duration`` / ``sample_times``, ``len`` and ``ts > threshold``.  PyCBC is no dependency of this project and the
    reference holds no vector of its container, so the last bits of ``sample_times`` are this definition's:
    ``arange(n) * delta_t + float(epoch)`` with the epoch kept as integer nanoseconds."""

    def __init__(self, data, delta_t, epoch=0):
        self.data = np.asarray(data)
        self.delta_t = delta_t
        self.start_time = GPSTime(epoch)

    def __len__(self):
        return len(self.data)

    @property
    def duration(self):
        return len(self.data) * self.delta_t

    @property
    def end_time(self):
        return self.start_time + self.duration

    @property
    def sample_times(self):
        return np.arange(len(self.data)) * self.delta_t + float(self.start_time)

    def __gt__(self, threshold):
        return self.data > threshold


def assemble_plan(ts_list):
    """``assemble_time_series`` (evaluate_test_data.py:374-387) without the copy: (start, n, delta_t, [(start_idx, ts)]) of
    the zero-filled series the list (sorted by start time) is written into, in that order."""
    if not ts_list:
        raise GwwError("assemble_time_series: no time series")
    start = float(min(ts_list, key=lambda ts: ts.start_time).start_time)
    end = float(max(ts_list, key=lambda ts: ts.end_time).end_time)
    dts = {ts.delta_t for ts in ts_list}
    if len(dts) != 1:
        raise GwwError(f"assemble_time_series: the series have different delta_t {sorted(dts)}")
    dt = dts.pop()
    n = int((end - start) / dt) + 1
    ret_start = GPSTime(start)
    ret_end = float(ret_start + n * dt)
    assert int((end - ret_end) / dt) == 0, f"Got end {end} and end_time {ret_end}"
    place = []
    for ts in ts_list:
        i = int(float(ts.start_time - ret_start) / dt)
        if i < 0 or i + len(ts) > n:
            raise GwwError(f"assemble_time_series: a series of {len(ts)} samples at index {i} does not fit {n} samples")
        place.append((i, ts))
    return start, n, dt, place


def assemble_time_series_host(ts_list) -> TimeSeries:
    """The reference's ``assemble_time_series`` in numpy (the golden tool and the host tests)."""
    start, n, dt, place = assemble_plan(ts_list)
    ret = TimeSeries(np.zeros(n), delta_t=dt, epoch=start)
    for i, ts in place:
        ret.data[i:i + len(ts)] = ts.data[:]
    return ret


def assemble_time_series(ts_list, device="cuda"):
    """The same on the device: a zero-filled fp64 series and one ordered copy per file on the current stream (a later file
    overwrites an earlier one where they overlap).  Returns (series fp64 [n] on the device, delta_t, epoch)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise GwwError(f"assemble_time_series: device must be a GPU (got {device}); gw_whisper_amd has no CPU path")
    start, n, dt, place = assemble_plan(ts_list)
    if n > MAX_N:
        raise GwwError(f"assemble_time_series: {n} samples, more than 2^27")
    series = torch.zeros((n,), dtype=torch.float64, device=device)
    for i, ts in place:
        series[i:i + len(ts)].copy_(torch.from_numpy(np.ascontiguousarray(ts.data)).to(device))
    return series, dt, float(GPSTime(start))


# =============================================================================================== the device stages
def _gpu_f64(x, who, name, device=None):
    """fp64 [n] on the device from numpy or a CUDA tensor."""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise GwwError(f"{who}: {name} is a CPU tensor; pass numpy or a GPU tensor (gw_whisper_amd has no CPU path)")
        if x.dtype != torch.float64:
            raise GwwError(f"{who}: {name} must be torch.float64, got {x.dtype}")
        if x.dim() != 1:
            raise GwwError(f"{who}: {name} must be [n], got {tuple(x.shape)}")
        return x.contiguous()
    a = np.ascontiguousarray(np.asarray(x, np.float64))
    if a.ndim != 1:
        raise GwwError(f"{who}: {name} must be [n], got {a.shape}")
    return torch.from_numpy(a).to(device if device is not None else "cuda")


def _series(series, who):
    if not torch.is_tensor(series) or not series.is_cuda:
        raise GwwError(f"{who}: series must be a GPU tensor (gw_whisper_amd has no CPU path)")
    if series.dtype not in (torch.float32, torch.float64):
        raise GwwError(f"{who}: series must be torch.float32 or torch.float64, got {series.dtype}")
    if series.dim() != 1 or series.numel() < 1:
        raise GwwError(f"{who}: series must be [n] with n >= 1, got {tuple(series.shape)}")
    if series.numel() > MAX_N:
        raise GwwError(f"{who}: {series.numel()} samples, more than 2^27")
    return series


def _empty():
    return np.zeros((0,), np.float64)


def triggers(series, delta_t, epoch, threshold, capacity=None):
    """``get_triggers``: (times, values) fp64 numpy of the samples with ``series[i] > threshold``; ``time = i * delta_t +
    epoch``.  ``series``: a CUDA fp32 or fp64 tensor [n]."""
    series = _series(series, "triggers")
    t, v, counts = ops.trig_triggers(series, delta_t, float(epoch), threshold, cap=capacity)
    n_trig, n_nan = (int(c) for c in counts.cpu().numpy())
    _check_series(n_trig, n_nan, t.numel(), "triggers")
    return t[:n_trig].cpu().numpy(), v[:n_trig].cpu().numpy()


def _check_series(n_trig, n_nan, cap, who):
    if n_nan > 0:
        raise GwwError(f"{who}: the series holds {n_nan} NaN")
    if n_trig > cap:
        raise GwwError(f"{who}: {n_trig} triggers, more than the capacity {cap}")


def _ascending_host(times, who):
    if not torch.is_tensor(times):
        t = np.asarray(times, np.float64)
        if t.size > 1 and not bool(np.all(t[1:] >= t[:-1])):
            raise GwwError(f"{who}: the trigger times are not ascending")


def events(times, values, cluster_tolerance):
    """Clustered events of ascending triggers: (times, values) fp64 numpy, per cluster the first maximum of its values.
    ``times`` / ``values``: numpy (what ``--load-triggers`` reads) or CUDA fp64 tensors."""
    _ascending_host(times, "events")
    if not torch.is_tensor(times) and np.asarray(times).size == 0 and np.asarray(values).size == 0:
        return _empty(), _empty()
    t = _gpu_f64(times, "events", "times")
    v = _gpu_f64(values, "events", "values", t.device)
    if t.shape != v.shape:
        raise GwwError(f"events: times {tuple(t.shape)} and values {tuple(v.shape)} differ in length")
    if t.numel() > MAX_N:
        raise GwwError(f"events: {t.numel()} triggers, more than 2^27")
    if t.numel() == 0:
        return _empty(), _empty()
    et, ev, counts = ops.trig_events(t, v, cluster_tolerance)
    n_ev, n_nan = (int(c) for c in counts.cpu().numpy())
    if n_nan > 0:
        raise GwwError(f"events: the trigger values hold {n_nan} NaN")
    return et[:n_ev].cpu().numpy(), ev[:n_ev].cpu().numpy()


def _injections(inj_times, distance, who):
    """The host side of the injections, checked before anything touches the device: (times fp64 [N], the reference's
    ``mc_prefactor``, ``Ninj``)."""
    inj = np.ascontiguousarray(np.asarray(inj_times, np.float64).reshape(-1))
    dist = np.asarray(distance, np.float64).reshape(-1)
    if inj.size == 0:
        raise GwwError(f"{who}: no injection")
    if np.isnan(inj).any():
        raise GwwError(f"{who}: the injection times hold NaN")
    if dist.shape != inj.shape:
        raise GwwError(f"{who}: distance must be [N = {inj.size}] as the injection times are")
    if inj.size > MAX_N:
        raise GwwError(f"{who}: {inj.size} injections, more than 2^27")
    # evaluate_test_data.py:591-595, in its own expressions
    max_distance = dist.max()
    mc_vtot = (4. / 3.) * np.pi * max_distance**3.
    Ninj = len(dist)
    mc_prefactor = mc_vtot / float(Ninj)
    return inj, float(mc_prefactor), Ninj


def _sorted_on(inj, device):
    """The injection times ascending, on the device (``injtimes.sort()``, evaluate_test_data.py:62-63)."""
    return ops.score_sort(torch.from_numpy(inj).to(device))[1]


def _statistics_device(ev_t, ev_v, n_ev, inj_sorted, prefactor, Ninj, duration, event_tolerance):
    """The device part from the events (capacity-sized tensors, ``n_ev`` int32 [1] on the device or None) on.  Returns what
    ``_finish`` reads."""
    _, diff = ops.score_closest(inj_sorted, ev_t)
    tp, fp, counts = ops.trig_split(ev_v, diff, event_tolerance, n_dev=n_ev)
    _, tp_sorted, _ = ops.score_sort(tp, n_dev=counts[0:1])
    _, fp_sorted, _ = ops.score_sort(fp, n_dev=counts[1:2])
    *outs, n_steps = ops.trig_steps(fp_sorted, counts[1:2], tp_sorted, counts[0:1], duration, prefactor, Ninj)
    return outs, n_steps, counts


def _finish(outs, n_steps, counts, who, partial=None):
    n_tp, n_fp, n_nan = (int(c) for c in counts.cpu().numpy())
    if n_nan > 0:
        raise GwwError(f"{who}: the event values hold {n_nan} NaN")
    if n_tp == 0:
        raise NoTruePositive(f"{who}: no true positive among the {n_tp + n_fp} events: no injection was found", partial)
    S = int(n_steps.item())
    ranking, far, frac, vol, vol_err = (o[:S].cpu().numpy() for o in outs)
    return {"ranking": ranking, "far": far, "sens-frac": frac, "sens-dist": (3 * vol / (4 * np.pi))**(1. / 3.), "sens-vol": vol,
            "sens-vol-err": vol_err}


def _check_duration(duration, who):
    if duration is None or not float(duration) > 0:
        raise GwwError(f"{who}: duration={duration} must be positive")
    return float(duration)


def statistics(event_times, event_values, inj_times, distance, duration, event_tolerance):
    """Events against injections: the dict of ``ranking``, ``far`` (per month), ``sens-frac``, ``sens-dist``, ``sens-vol``,
    ``sens-vol-err`` (fp64 numpy, one entry per ranking step).  ``event_times`` / ``event_values``: numpy (what
    ``--load-events`` reads) or CUDA fp64 tensors; ``inj_times`` and ``distance`` numpy [N], in any order."""
    duration = _check_duration(duration, "statistics")
    inj, prefactor, Ninj = _injections(inj_times, distance, "statistics")
    t = _gpu_f64(event_times, "statistics", "event_times")
    v = _gpu_f64(event_values, "statistics", "event_values", t.device)
    if t.shape != v.shape:
        raise GwwError(f"statistics: event_times {tuple(t.shape)} and event_values {tuple(v.shape)} differ in length")
    if t.numel() > MAX_N:
        raise GwwError(f"statistics: {t.numel()} events, more than 2^27")
    if t.numel() == 0:
        raise NoTruePositive("statistics: no event, so no true positive: no injection was found")
    outs, n_steps, counts = _statistics_device(t, v, None, _sorted_on(inj, t.device), prefactor, Ninj, duration, event_tolerance)
    return _finish(outs, n_steps, counts, "statistics")


def evaluate(series, delta_t, epoch, inj_times, distance, trigger_threshold=0.1, cluster_tolerance=0.2, event_tolerance=0.3,
             duration=None, capacity=None):
    """``triggers`` -> ``events`` -> ``statistics`` on the device without a host trip in between.  ``duration`` defaults to
    ``len(series) * delta_t`` (the reference's ``ts.duration``); ``capacity``: the most triggers to make room for (default:
    the number of samples).  Returns {"triggers": (times, values), "events": (times, values), "statistics": {...}}."""
    series = _series(series, "evaluate")
    duration = _check_duration(series.numel() * delta_t if duration is None else duration, "evaluate")
    inj, prefactor, Ninj = _injections(inj_times, distance, "evaluate")
    inj_sorted = _sorted_on(inj, series.device)
    t, v, c_trig = ops.trig_triggers(series, delta_t, float(epoch), trigger_threshold, cap=capacity)
    et, ev, c_ev = ops.trig_events(t, v, cluster_tolerance, n_dev=c_trig[0:1])
    outs, n_steps, counts = _statistics_device(et, ev, c_ev[0:1], inj_sorted, prefactor, Ninj, duration, event_tolerance)
    # the one read of the device
    n_trig, n_nan = (int(c) for c in c_trig.cpu().numpy())
    _check_series(n_trig, n_nan, t.numel(), "evaluate")
    n_ev = int(c_ev[0].item())
    partial = {"triggers": (t[:n_trig].cpu().numpy(), v[:n_trig].cpu().numpy()),
               "events": (et[:n_ev].cpu().numpy(), ev[:n_ev].cpu().numpy())}
    return {**partial, "statistics": _finish(outs, n_steps, counts, "evaluate", partial)}


# =============================================================================================== the network over windows
def score_windows(model, windows, batch_size=0):
    """``test_network.py:111-149`` for one file: windows [n, 2048] (a CUDA fp32 tensor at 2048 Hz, uploaded once) ->
    ``inference.resample`` to 16 kHz -> log-mel -> the encoder's last token -> both columns of the detection head, [n, 2]
    CUDA fp32: the softmax ``(p0, p1)``, or ``(z0 - z1, z1 - z0)`` after ``efficiency.remove_softmax``.  ``batch_size`` 0:
    the whole file at once, as in the reference; a window's outputs do not depend on it."""
    from torch import nn

    from . import efficiency, inference
    from .models import _pooled
    if not torch.is_tensor(windows) or not windows.is_cuda:
        raise GwwError("score_windows: windows must be a GPU tensor (gw_whisper_amd has no CPU path)")
    if windows.dim() != 2 or windows.shape[0] < 1:
        raise GwwError(f"score_windows: windows must be [n, samples] with n >= 1, got {tuple(windows.shape)}")
    last = list(model.classifier.children())[-1]
    if isinstance(last, nn.Softmax):
        remove = False
    elif isinstance(last, efficiency.LogitDifference):
        remove = True
    else:
        raise GwwError("score_windows: the classifier must end in Softmax or in remove_softmax's layer")
    params = [p.detach() for p in efficiency._det_parameters(model.classifier)]
    n_mels = int(getattr(getattr(model.encoder, "config", None), "num_mel_bins", 80))
    n = windows.shape[0]
    step = n if int(batch_size) <= 0 else int(batch_size)
    n_out = windows.shape[1] * 16000 // 2048
    out = torch.empty((n, 2), dtype=torch.float32, device=windows.device)
    with torch.no_grad():
        for i in range(0, n, step):
            wave = inference.resample(windows[i:i + step].to(torch.float32), n_out)
            mel = ops.logmel(wave, n_mels=n_mels)
            ops.det_head_scores2(_pooled(model.encoder, mel).to(torch.float32), params, out[i:i + step], remove_softmax=remove)
    return out
