"""The catalogue-event scan: counterpart of the reference's ``Signal_vs_Noise/Real_events`` (``preprocess_real_events.py``
+ ``evaluation_real_events.py``) on the device.

The reference cuts every event's H1 and L1 strain (2048 Hz) into windows of 2048 samples every 204, resamples each to
16 kHz with ``scipy.signal.resample``, writes one ``datasets`` directory per window and detector, and then scores the
windows at batch 1.  Here the strain of all events is uploaded once, the windows are strided views of it
(``inference.DeviceSegmentSlicer.windows``), and resampling (``inference.resample``), the log-mel front end
(``ops.logmel``), the encoder and the head run in batches over all events; one copy comes back.

Quirk of the reference, documented and not copied: ``evaluation_real_events.py:85-86`` globs ``.../segment_0`` only, so as
written it scores window 0 of every event although its comment expects ``(31,)`` per event.  ``scan_events`` scores every
window; column 0 (``harness/run_real_events.py --first-window-only``) is what the program as written produces.
"""

from __future__ import annotations

import os

import numpy as np
import torch

from ._lib import GwwError

WINDOW_SIZE = 2048   # preprocess_real_events.py:12
STEP_SIZE = 204


def window_starts(n_samples: int, window_size: int = WINDOW_SIZE, step_size: int = STEP_SIZE) -> range:
    """First samples of the windows ``extract_segments`` cuts (``preprocess_real_events.py:12-17``)."""
    return range(0, n_samples - window_size + 1, step_size)


def event_label(key: str) -> str:
    """``GW150914-v3`` -> ``GW150914`` (``evaluation_real_events.py:83``: the name up to its first ``-``)."""
    return os.path.basename(key).split("-")[0]


def _have_h5py() -> bool:
    try:
        import h5py  # noqa: F401
        return True
    except ImportError:
        return False


def resolve(path: str) -> str:
    """The file to open for ``path``: itself, or -- without h5py -- its ``.npz`` twin."""
    if path.endswith(".npz") or _have_h5py():
        return path
    if os.path.isfile(path + ".npz"):
        return path + ".npz"
    raise IOError(f"{path}: h5py is not importable and there is no {path}.npz beside it")


def output_path(path: str) -> str:
    return path if path.endswith(".npz") or _have_h5py() else path + ".npz"


def event_keys(path: str) -> list:
    """The event groups of a strain file, in file order."""
    path = resolve(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            keys = []
            for k in z.files:
                ev, _, name = k.rpartition("/")
                if name in ("h1_strain", "l1_strain") and ev and ev not in keys:
                    keys.append(ev)
            return keys
    import h5py
    with h5py.File(path, "r") as fp:
        return list(fp.keys())


def read_events(path: str, names=None):
    """(keys, strain [E, 2, N] float32) of ``<event>/h1_strain`` (detector 0) and ``<event>/l1_strain`` (detector 1).
    ``names``: the events wanted, in that order (default: every event, in file order).  Events of unequal length are
    refused: the reference's ``np.array(...)`` and its even split of the windows assume one length too."""
    have = event_keys(path)
    keys = list(names) if names else have
    missing = [k for k in keys if k not in have]
    if missing:
        raise GwwError(f"{path}: no event {missing[0]!r} (the file has {', '.join(have) or 'no events'})")
    if not keys:
        raise GwwError(f"{path}: no <event>/h1_strain + <event>/l1_strain pairs")
    path = resolve(path)
    rows = []
    if path.endswith(".npz"):
        with np.load(path) as z:
            for k in keys:
                rows.append((np.asarray(z[f"{k}/h1_strain"]), np.asarray(z[f"{k}/l1_strain"])))
    else:
        import h5py
        with h5py.File(path, "r") as fp:
            for k in keys:
                rows.append((fp[k]["h1_strain"][()], fp[k]["l1_strain"][()]))
    return keys, stack_events(keys, rows)


def stack_events(keys, rows) -> np.ndarray:
    """[(h1, l1)] per event -> [E, 2, N] float32; unequal lengths are refused with the offending event named."""
    n = len(rows[0][0])
    for k, (h1, l1) in zip(keys, rows):
        if h1.ndim != 1 or l1.ndim != 1 or len(h1) != n or len(l1) != n:
            raise GwwError(f"event {k}: h1_strain {h1.shape} / l1_strain {l1.shape} where the first event has ({n},): the "
                           f"scan needs every event and both detectors at one length")
    return np.stack([np.stack((h1, l1)) for h1, l1 in rows]).astype(np.float32)


def scan_events(model, strain, batch_size: int = 256, window_size: int = WINDOW_SIZE, step_size: int = STEP_SIZE,
                n_mels: int = 80, device="cuda", frontend=None) -> np.ndarray:
    """``sigmoid(model(mel_h1, mel_l1))`` of every window of every event: strain [E, 2, N] at 2048 Hz (H1 = detector 0,
    L1 = detector 1), one upload; result [E, n_windows] float32, one copy back.  ``model``: a two-detector model on the
    device (``two_channel_ligo_binary_classifier`` or ``TwoChannelLIGOBinaryClassifierCNN``, num_classes = 1).
    ``frontend``: an ``ops.FrontendConfig`` whose ``n_samples`` is ``window_size`` -- the features of a model trained at the
    strain's own rate, through ``ops.logmel_windows`` on the [E * 2, N] rows (no resampling, no window is cut, an STFT
    frame shared by several windows of a batch is computed once); ``None``: resample to 16 kHz + Whisper's published
    log-mel, as the reference does."""
    from . import ops
    from .inference import resample
    if isinstance(strain, (list, tuple)):
        lens = {tuple(np.shape(s)) for s in strain}
        if len(lens) != 1:
            raise GwwError(f"scan_events: events of unequal shape {sorted(lens)}: the scan needs one length")
    t = strain if torch.is_tensor(strain) else torch.as_tensor(np.asarray(strain))
    if t.dim() != 3 or t.shape[1] != 2:
        raise GwwError(f"scan_events: strain {tuple(t.shape)} is not [events, 2, samples]")
    E, _, N = t.shape
    starts = window_starts(N, window_size, step_size)
    W = len(starts)
    if W == 0:
        raise GwwError(f"scan_events: {N} samples hold no window of {window_size}")
    dss = t.to(device=device, dtype=torch.float32).contiguous()      # the one host-to-device copy
    if frontend is not None:
        return _scan_native(model, dss, W, batch_size, window_size, step_size, frontend)
    # window (e, j), detector k as a view: no bytes move
    win = dss.as_strided((E, W, 2, window_size), (dss.stride(0), step_size, dss.stride(1), 1))
    out = torch.empty((E * W,), dtype=torch.float32, device=dss.device)
    n_out = window_size * 16000 // 2048                              # preprocess_real_events.py:22
    with torch.no_grad():
        for i0 in range(0, E * W, batch_size):
            idx = torch.arange(i0, min(i0 + batch_size, E * W), device=dss.device)
            w = win[idx // W, idx % W]                               # [b, 2, window]
            b = w.shape[0]
            wave = resample(w.permute(1, 0, 2).reshape(2 * b, window_size), n_out)
            mel = ops.logmel(wave, n_mels=n_mels)
            logits = model(mel[:b], mel[b:])
            out[i0:i0 + b] = torch.sigmoid(logits.float().reshape(b))
    return out.reshape(E, W).cpu().numpy()


def _scan_native(model, dss, W: int, batch_size: int, window_size: int, step_size: int, frontend) -> np.ndarray:
    """``scan_events`` on a native-rate front end: batches of ``batch_size`` windows as before, now window-major -- windows
    j0 .. j1 - 1 of as many events as fill the batch -- so that one ``ops.logmel_windows`` call serves a batch; rows-major
    output [E' * 2, n, ...] viewed as [E', 2, n, ...] gives ``mel_h1`` and ``mel_l1`` as slices (views, where a batch holds the
    windows of one event -- the catalogue's case of long events)."""
    from . import ops
    if frontend.n_samples != window_size:
        raise GwwError(f"scan_events: frontend.n_samples is {frontend.n_samples} but window_size is {window_size}: the front "
                       f"end's chunk must be the window")
    E, _, N = dss.shape
    rows = dss.reshape(E * 2, N)
    out = torch.empty((E, W), dtype=torch.float32, device=dss.device)
    nm, F = frontend.n_mels, frontend.n_frames
    with torch.no_grad():
        if W >= batch_size:                                           # one event at a time, its windows in batches
            groups = [(e, e + 1, j0, min(j0 + batch_size, W)) for e in range(E) for j0 in range(0, W, batch_size)]
        else:                                                         # whole events, as many as fit a batch
            per = max(1, batch_size // W)
            groups = [(e0, min(e0 + per, E), 0, W) for e0 in range(0, E, per)]
        for e0, e1, j0, j1 in groups:
            b, n = e1 - e0, j1 - j0
            mel = ops.logmel_windows(rows[2 * e0:2 * e1], frontend, step_size, w0=j0, n_windows=n, rows_major=True)
            mel = mel.reshape(b, 2, n, nm, F)
            logits = model(mel[:, 0].reshape(b * n, nm, F), mel[:, 1].reshape(b * n, nm, F))
            out[e0:e1, j0:j1] = torch.sigmoid(logits.float().reshape(b, n))
    return out.cpu().numpy()
