"""Glitch scan: a trained glitch model over continuous strain -- what the data contains, when, and how confidently.

The reference classifies pre-cut, labelled 1 s segments (``Glitch_classification/src/evaluate.py``); its training data were
cut around catalogued glitches after conditioning (``Glitch_classification/utils/generate_glitch_dataset.py:43-62``).  Here
the same model slides over a series:

    highpass_taps / condition   the conditioning of the training data on the device: optional decimation, ``whiten`` (4 s
                                segments, 4 s filter), PyCBC's ``highpass_fir`` (30 Hz, order 512) through ``gww_fir_f64``
    GlitchScanner.scan          windows and stamps from ``inference.DeviceSegmentSlicer``; per batch features -> pooled
                                encoder pass -> ``ops.head_scan`` (class and probability of every window, written into
                                series-long device arrays); per detector ONE ``ops.glitch_events`` call and ONE host read
    build_events_host           the event semantics as the sequential program, in numpy: what the device must equal bit
                                for bit (as ``inference.get_clusters`` is for the search)

Events: the windows of one class whose probability exceeds ``prob_threshold`` are its triggers; a trigger more than ``gap``
seconds after the class's previous one opens a new event.  Classes cluster independently, so events of different classes may
overlap in time.  An event reports its class, first / last / peak stamp, peak probability (the FIRST maximum) and its number
of windows; events are ordered by their first window.

**Parity unpinned** for ``condition``: PyCBC is not installed wherever this package can be built or run.  The whitening follows
``oracle/whiten.py`` (``whiten.py``); the taps of the high-pass are scipy's ``firwin`` to 3.5e-18, but the exact sample
alignment of PyCBC's ``fir_zero_filter`` (taken here as the centred, delay-compensated filter with zero edges, ``order``
samples dropped on each side) cannot be checked against it.
"""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["highpass_taps", "condition", "build_events_host", "GlitchScanner", "EVENT_KEYS"]

EVENT_KEYS = ("cls", "first", "n", "t_start", "t_end", "t_peak", "p_peak")     # ops.glitch_events / build_events_host
_EVENT_TYPES = (np.int32, np.int32, np.int32, np.float64, np.float64, np.float64, np.float32)
MAX_CLASSES = 64


# =============================================================================================== conditioning
def highpass_taps(frequency: float, order: int, delta_t: float, beta: float = 5.0) -> np.ndarray:
    """The taps PyCBC's ``highpass_fir(frequency, order, beta)`` designs for a series of ``delta_t``:
    ``scipy.signal.firwin(2 * order + 1, frequency / (int(1 / delta_t) / 2), window=("kaiser", beta), pass_zero=False)``
    restated in numpy (fp64 [2 * order + 1], symmetric, unit gain at the Nyquist frequency)."""
    k = frequency / float(int(1.0 / delta_t) / 2)
    if not 0.0 < k < 1.0:
        raise ValueError(f"highpass_taps: {frequency} Hz is not inside (0, Nyquist) at delta_t = {delta_t}")
    numtaps = 2 * int(order) + 1
    m = np.arange(numtaps) - order
    h = (np.sinc(m) - k * np.sinc(k * m)) * np.kaiser(numtaps, beta)
    h /= np.sum(h * np.cos(np.pi * m))
    return h


def condition(strain, delta_t: float, decimate: int = 1, segment_duration: float = 4.0, max_filter_duration: float = 4.0,
              highpass: float = 30.0, order: int = 512, beta: float = 5.0, device="cuda"):
    """The conditioning of the reference's glitch training data (``generate_glitch_dataset.py:43-60``) for ``[n]`` or
    ``[D, n]`` strain sampled every ``delta_t`` seconds: ``strain[..., ::decimate]`` (the reference's plain ``[::2]``, no
    anti-alias filter), ``whiten(segment_duration, max_filter_duration)``, then the ``highpass`` Hz FIR of ``order`` with
    ``order`` samples dropped on each side -- fp64 samples, taps and sums, one rounding to fp32 (``gww_fir_f64``).
    Returns (fp32 strain on the GPU, sampled every ``delta_t * decimate``; the seconds removed at the start).
    PARITY UNPINNED (module docstring): PyCBC is absent, the sample alignment of its ``fir_zero_filter`` is assumed."""
    from ._lib import check, lib
    from .whiten import whiten
    x = strain if torch.is_tensor(strain) else torch.from_numpy(np.asarray(strain))
    one_d = x.dim() == 1
    if one_d:
        x = x[None]
    if x.dim() != 2:
        raise ValueError("condition: strain must be [n] or [detectors, n]")
    x = x.to(device)
    if not x.is_cuda:
        raise _lib.GwwError("condition needs a GPU: gw_whisper_amd has no CPU path")
    decimate = int(decimate)
    if decimate < 1:
        raise ValueError(f"condition: decimate={decimate} must be >= 1")
    if decimate > 1:
        x = x[:, ::decimate]
        delta_t = delta_t * decimate
    if x.shape[1] % 2:
        x = x[:, :-1]                                    # whiten takes an even number of samples
    white = whiten(x.contiguous(), delta_t=delta_t, segment_duration=segment_duration,
                   max_filter_duration=max_filter_duration, device=x.device)
    removed = int(max_filter_duration * (1.0 / delta_t)) // 2
    D, n = white.shape
    n_out = n - 2 * order
    if n_out < 1:
        raise ValueError(f"condition: {n} whitened samples are not enough for a high-pass of order {order}")
    # y[i] = sum_m h[m] x[i - m], m = -order .. order, for i = order .. n - order - 1: no sample outside the series is touched,
    # so zero edges and circular ones agree on what is kept.  As a correlation: out[j] = sum_u g[u] x[j + u], g[u] = h[order - u]
    taps = highpass_taps(highpass, order, delta_t, beta)[::-1].copy()
    taps4 = (taps.size + 3) // 4 * 4
    g = torch.zeros((taps4,), dtype=torch.float64, device=x.device)
    g[:taps.size] = torch.from_numpy(taps).to(x.device)
    pad = (n_out + taps4 + 3) // 4 * 4
    out_stride = (n_out + 3) // 4 * 4
    out = torch.empty((D, out_stride), dtype=torch.float32, device=x.device)
    for d in range(D):
        xp = torch.zeros((pad,), dtype=torch.float64, device=x.device)
        xp[:n] = white[d].double()
        with torch.cuda.device(x.device):
            check(lib().gww_fir_f64(xp.data_ptr(), pad, g.data_ptr(), taps4, 1, out[d].data_ptr(), out_stride, n_out,
                                    torch.cuda.current_stream().cuda_stream), "gww_fir_f64")
    y = out[:, :n_out]
    return (y[0] if one_d else y), (removed + order) * delta_t


# =============================================================================================== events, host restatement
def ignore_mask(ignore) -> int:
    """The 64-bit mask of ``gww_glitch_events`` from a mask or an iterable of class indices."""
    if isinstance(ignore, (int, np.integer)):
        mask = int(ignore)
    else:
        mask = 0
        for c in ignore:
            if not 0 <= int(c) < MAX_CLASSES:
                raise ValueError(f"ignore: class {c} is not in 0..{MAX_CLASSES - 1}")
            mask |= 1 << int(c)
    if not 0 <= mask < 2 ** 64:
        raise ValueError("ignore: a 64-bit mask")
    return mask


def build_events_host(times, cls, prob, prob_threshold: float = 0.5, gap: float = 0.35, ignore=0) -> dict:
    """The events of ``times`` fp64 [n], ``cls`` int [n], ``prob`` fp32 [n] by the sequential program ``gww_glitch_events``
    must equal bit for bit (the threshold is compared in fp32, the stamps in fp64, both strictly).  Returns a dict of
    numpy arrays under ``EVENT_KEYS``, one entry per event, ordered by ``first``."""
    times = np.asarray(times, np.float64)
    cls = np.asarray(cls, np.int64)
    prob = np.asarray(prob, np.float32)
    if not (times.ndim == 1 and times.shape == cls.shape == prob.shape):
        raise ValueError("build_events_host: times, cls and prob must be [n]")
    mask, thr, gap = ignore_mask(ignore), np.float32(prob_threshold), np.float64(gap)
    open_, done = {}, []
    for i in range(times.size):
        c, p, t = int(cls[i]), prob[i], times[i]
        if c < 0 or c >= MAX_CLASSES or (mask >> c) & 1 or not (p > thr):      # NaN is no trigger
            continue
        e = open_.get(c)
        if e is not None and (t - e["t_end"]) > gap:                           # fp64, strict
            done.append(open_.pop(c))
            e = None
        if e is None:
            e = open_[c] = dict(cls=c, first=i, n=0, t_start=t, t_end=t, t_peak=t, p_peak=p)
        e["t_end"] = t
        e["n"] += 1
        if p > e["p_peak"]:                                                    # strict: the first maximum
            e["t_peak"], e["p_peak"] = t, p
    done.extend(open_.values())
    done.sort(key=lambda e: e["first"])
    return {k: np.array([e[k] for e in done], dtype=dt) for k, dt in zip(EVENT_KEYS, _EVENT_TYPES)}


# =============================================================================================== the scan
class GlitchScanner:
    """``model``: what ``glitch.build_model`` returns (an encoder and the ``nn.Sequential`` head of
    ``models.glitch_classifier``), ``classes``: its class names in label order.  ``frontend=None`` is the reference's
    training path -- every 1 s window resampled to 16 kHz, then ``ops.logmel``; a native-rate front end (an
    ``ops.FrontendConfig``, or a ``WhisperFeatureExtractor`` holding one) computes the features of all windows of a batch
    straight from the series (``NativeMelAdapter.from_series``: each STFT frame once), its ``n_samples`` is the window."""

    def __init__(self, model, classes: Sequence[str], frontend=None):
        from .glitch import _head_parameters
        from .inference import NativeMelAdapter
        self.model = model.eval()
        self.classes = [str(c) for c in classes]
        params, _p = _head_parameters(model.classifier)
        self.params = [t.detach() for t in params]
        C = int(self.params[-2].shape[0])
        if len(self.classes) != C or C > MAX_CLASSES:
            raise _lib.GwwError(f"GlitchScanner: {len(self.classes)} class names for a head of {C} classes (at most "
                                f"{MAX_CLASSES})")
        self.adapter = None
        if frontend is not None:
            config = frontend.frontend_config if hasattr(frontend, "frontend_config") else frontend
            if config is None:
                raise _lib.GwwError("GlitchScanner: this extractor is Whisper's published configuration, which is the default "
                                    "path (frontend=None): resample to 16 kHz, then ops.logmel")
            self.adapter = NativeMelAdapter(config, n_detectors=1)

    def class_indices(self, names_or_indices) -> list:
        """Class indices from names (as in ``classes``) or indices."""
        out = []
        for c in names_or_indices:
            if isinstance(c, str):
                if c not in self.classes:
                    raise ValueError(f"GlitchScanner: no class {c!r} among {self.classes}")
                c = self.classes.index(c)
            out.append(int(c))
        return out

    def window_length(self, delta_t: float) -> int:
        """Samples of one window: the front end's chunk, or one second (the reference's crop) on the default path."""
        rate = int(round(1.0 / delta_t))
        if self.adapter is None:
            return rate
        if self.adapter.config.sampling_rate != rate:
            raise _lib.GwwError(f"GlitchScanner: the front end is for {self.adapter.config.sampling_rate} Hz, the strain has "
                                f"{rate} Hz")
        return self.adapter.config.n_samples

    def _classify(self, slicer, batch_size: int, window: int):
        """(cls int32 [n], prob fp32 [n]) of every window of the slicer's one-detector series, on the device."""
        from . import ops
        from .inference import resample
        from .models import _pooled
        n, dev = len(slicer), slicer.dss.device
        if n == 0:
            return (torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.float32, device=dev))
        n_mels = self.model.encoder.config.num_mel_bins
        cls = prob = None
        with torch.no_grad():
            for i0 in range(0, n, batch_size):
                i1 = min(n, i0 + batch_size)
                if self.adapter is not None:
                    feats = self.adapter.from_series(slicer.dss, slicer.index_step_size, i0, i1 - i0, window=window)[:, 0]
                else:
                    feats = ops.logmel(resample(slicer.windows(i0, i1)[:, 0].contiguous()), n_mels=n_mels)
                tok = _pooled(self.model.encoder, feats).to(torch.float32)
                cls, prob, _ = ops.head_scan(tok, self.params, cls, prob, row_offset=i0, n_rows=n)
        return cls, prob

    def scan(self, strain, start_time: float = 0.0, delta_t: float = 1.0 / 2048, step_size: float = 0.1,
             peak_offset: float = 0.8, batch_size: int = 256, prob_threshold: float = 0.5, gap: float = 0.35,
             ignore=(), conditioned: bool = True, return_windows: bool = False, device="cuda") -> dict:
        """Classify every window of ``strain`` (``[n]`` or ``[D, n]``; a glitch model is single-detector, so every row is
        scanned as its own series) and build the events of every class.  Window i covers samples ``[i step, i step +
        window)`` and is stamped ``start + i step + peak_offset`` by the slicer's running sum; 0.8 s is where the
        reference's crop puts the glitch.  ``conditioned=False`` runs ``condition`` first and moves the start by what it
        removes.  ``ignore``: class names or indices that never trigger.  Returns numpy arrays, one entry per event,
        detector after detector and by first window within one: ``detector`` ``class`` ``n_windows`` (int32),
        ``time_start`` ``time_end`` ``time_peak`` (fp64), ``prob`` (fp32, the peak); with ``return_windows`` also
        ``window_class`` int32 / ``window_prob`` fp32 / ``window_time`` fp64, each ``[D, windows]``."""
        from . import ops
        from .inference import DeviceSegmentSlicer
        if torch.is_tensor(strain):
            if not strain.is_cuda:
                raise _lib.GwwError("GlitchScanner.scan needs a GPU tensor (or a numpy array, uploaded once): gw_whisper_amd "
                                    "has no CPU path")
            x = strain
        else:
            x = torch.from_numpy(np.ascontiguousarray(strain)).to(device)
            if not x.is_cuda:
                raise _lib.GwwError(f"GlitchScanner.scan: device={device!r} is not a GPU; gw_whisper_amd has no CPU path")
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError("GlitchScanner.scan: strain must be [n] or [detectors, n]")
        mask = ignore_mask(self.class_indices(ignore))
        per_det, windows = [], []
        for d in range(x.shape[0]):
            series, start, dt = x[d:d + 1], float(start_time), float(delta_t)
            if not conditioned:
                series, removed = condition(series, dt, device=x.device)
                start += removed
            window = self.window_length(dt)
            slicer = DeviceSegmentSlicer(series, start_time=start, delta_t=dt, step_size=step_size, peak_offset=peak_offset,
                                         slice_length=window, device=x.device, white=True)
            n = len(slicer)
            cls, prob = self._classify(slicer, int(batch_size), window)
            times = slicer.times(0, n)
            ev = ops.glitch_events(times, cls, prob, prob_threshold, gap, mask)
            # ONE read per detector: the count, the event arrays and (if asked for) the windows as one byte string
            parts = [ev["count"]] + [ev[k] for k in EVENT_KEYS] + ([cls, prob] if return_windows else [])
            blob = torch.cat([p.view(torch.uint8) for p in parts]).cpu().numpy()
            off, host = 0, []
            for p in parts:
                nb = p.numel() * p.element_size()
                host.append(blob[off:off + nb].view(_NUMPY_OF[p.dtype]))
                off += nb
            k = int(host[0][0])
            assert k <= n, "an event holds at least one window"
            e = {key: a[:k].copy() for key, a in zip(EVENT_KEYS, host[1:1 + len(EVENT_KEYS)])}
            e["detector"] = np.full((k,), d, np.int32)
            per_det.append(e)
            if return_windows:
                windows.append((host[-2].copy(), host[-1].copy(), slicer.times_host(0, n).copy()))

        def cat(key, dt):
            return np.concatenate([e[key] for e in per_det]).astype(dt, copy=False)
        out = {"detector": cat("detector", np.int32), "class": cat("cls", np.int32), "time_start": cat("t_start", np.float64),
               "time_end": cat("t_end", np.float64), "time_peak": cat("t_peak", np.float64), "prob": cat("p_peak", np.float32),
               "n_windows": cat("n", np.int32)}
        if return_windows:
            out["window_class"] = np.stack([w[0] for w in windows])
            out["window_prob"] = np.stack([w[1] for w in windows])
            out["window_time"] = np.stack([w[2] for w in windows])
        return out


_NUMPY_OF = {torch.int32: np.int32, torch.float32: np.float32, torch.float64: np.float64}
