"""Band-limited strain, the ideal-fp32 yardstick and the per-element error model of the log-mel tests (a plain module, numpy
only, deterministic per seed).

The reference feeds the front end strain that was FFT-resampled from 2048 Hz (or 4096 Hz) to 16 kHz: above the old Nyquist
frequency such a segment holds only window leakage, 8 to 12 decades below the band.  About half of the live elements of
its log-mel then sit on the ``max - 8`` clamp floor, and the ones just above it are small remainders of large
cancellations.  White noise (all the other log-mel tests use it) never gets there.  The tests built on this module hold
every element the clamp leaves alone to an error bound of its OWN, ``e_model``:

    u = 2^-24,  d_f = u * ||windowed frame f||_2,  A_k = |X_k| of the oracle
    e_model[m, f] = sum_k fb[k, m] (2 A_k d_f + d_f^2) / max(mel[m, f], 1e-10) / (4 ln 10)  +  2 u max(|out|, 1)

(one fp32 rounding of every windowed sample perturbs each X_k by about d_f; the rest is that perturbation carried through
|X|^2, the filterbank, log10 and the affine map, plus the roundings of the output itself).

Oracle: ``oracle.logmel.log_mel`` in fp64 on the library's own window table, ``float32(0.5 - 0.5 cos(2 pi n / 400))``, so
that it is exact arithmetic on the function the kernels compute (``torch.hann_window(400)`` is another table, see
test_logmel_like_host.py).  Yardstick: ``ideal_fp32`` restates the documented dataflow of ``csrc/logmel.hip`` in numpy
float32 with nothing the kernel does not have to do: fp32 window product, even / odd fold, exactly rounded twiddles, one
n-ordered multiply-add chain per sum (every product and every sum rounded once: plain elementwise numpy, so the figures do
not depend on a BLAS), fp32 power and mel.  ``GAMMA`` is the worst ``|ideal_fp32 - oracle| / e_model`` over the unclamped
live elements of a family; the GPU tests allow the kernel ``LIMIT`` = 4 x that (the MFMA chain takes two terms per step
and fuses; the yardstick does neither).  test_logmel_like_host.py re-derives the constants on every run.
"""

import numpy as np

from oracle import logmel as olm

FS = 16000
N = 16000                    # 1 s
N_MELS = (80, 128)
LIMIT = 4.0                  # kernel error <= LIMIT x GAMMA x e_model
U = 2.0 ** -24
NEAR = 0.01                  # log10 distance from a clamp floor inside which an element counts as neither side's
FRAMES_1S = 105              # frames of a 1 s item the tests look at: 102 live ones and three dead ones

FAMILIES = ("white", "resampled2048", "resampled4096", "burst", "line60", "line500", "ladder", "mixed", "ragged")
LADDER_K = (0, -10, -17, 20)
RAGGED_N = (12345, 40000, 480000)
_SEED = {f: 100 + i for i, f in enumerate(FAMILIES)}

# max over the unclamped live elements of |ideal_fp32 - oracle| / e_model, per (family, n_mels); derived by
# test_logmel_like_host.py::test_ideal_fp32_reproduces_gamma (which holds them to 10 %)
GAMMA = {
    ("white", 80): 2.366e+00,
    ("white", 128): 3.349e+00,
    ("resampled2048", 80): 4.442e+00,
    ("resampled2048", 128): 8.466e+00,
    ("resampled4096", 80): 3.583e+00,
    ("resampled4096", 128): 4.118e+00,
    ("burst", 80): 3.920e+00,
    ("burst", 128): 4.871e+00,
    ("line60", 80): 6.611e+00,
    ("line60", 128): 9.004e+00,
    ("line500", 80): 7.248e+00,
    ("line500", 128): 8.450e+00,
    ("ladder", 80): 4.566e+00,
    ("ladder", 128): 5.628e+00,
    ("mixed", 80): 7.476e+00,
    ("mixed", 128): 8.127e+00,
    ("ragged", 80): 6.404e+00,
    ("ragged", 128): 1.297e+01,
}


# ---------------------------------------------------------------------------------------------------- segments

def fft_resample(x, num):
    """FFT zero-padding resample of real ``x`` [..., n] to ``num`` >= n samples (what ``scipy.signal.resample`` computes:
    the spectrum is kept, an even n's Nyquist bin is shared between the two new bins it becomes)."""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    assert num >= n
    X = np.fft.rfft(x, axis=-1)
    Y = np.zeros(x.shape[:-1] + (num // 2 + 1,), np.complex128)
    Y[..., :n // 2 + 1] = X
    if n % 2 == 0 and num > n:
        Y[..., n // 2] *= 0.5
    return np.fft.irfft(Y, num, axis=-1) * (num / n)


def resampled(n_items, rate, seed, n_out=N):
    """float64 [n_items, n_out]: unit-variance white noise at ``rate`` Hz, resampled to 16 kHz and cut to n_out."""
    n_in = -(-n_out * rate // FS)
    x = np.random.default_rng(seed).standard_normal((n_items, n_in))
    return fft_resample(x, n_in * FS // rate)[:, :n_out]


def batches(family):
    """The family's batches, a list of float32 [n, L] (one batch, or one per length for ``ragged``)."""
    seed = _SEED[family]
    t = np.arange(N) / FS
    burst = 300.0 * np.sin(2 * np.pi * (80.0 + 400.0 * t) * t) * np.exp(-0.5 * ((t - 0.5) / 0.02) ** 2)
    line60 = 1000.0 * np.sin(2 * np.pi * 60.0 * t)
    if family == "white":
        x = [np.random.default_rng(seed).standard_normal((2, N))]
    elif family == "resampled2048":
        x = [resampled(2, 2048, seed)]
    elif family == "resampled4096":
        x = [resampled(2, 4096, seed)]
    elif family == "burst":
        x = [resampled(2, 2048, seed) + burst]
    elif family == "line60":
        x = [resampled(2, 2048, seed) + line60]
    elif family == "line500":
        x = [np.random.default_rng(seed).standard_normal((2, N)) + 1e3 * np.sin(2 * np.pi * 500.3 * t)]
    elif family == "ladder":
        base = resampled(1, 2048, seed).astype(np.float32)[0]
        x = [np.stack([base * np.float32(2.0 ** k) for k in LADDER_K])]       # exact scalings of one fp32 item
    elif family == "mixed":
        r = resampled(4, 2048, seed)
        x = [np.stack([r[0] + burst, r[1] * 1e-3, np.zeros(N), r[3] + line60])]
    elif family == "ragged":
        x = [resampled(1, 2048, seed + i, n) for i, n in enumerate(RAGGED_N)]
    else:
        raise KeyError(family)
    return [np.ascontiguousarray(b, dtype=np.float32) for b in x]


# ---------------------------------------------------------------------------------------------------- tables

def lib_window():
    """The window table the library holds (csrc/logmel.hip, csrc/logmel_host.cpp): the exact periodic Hann rounded to fp32."""
    return olm.hann_periodic().astype(np.float32)


def _twiddles():
    k = np.arange(olm.N_FFT)
    return (np.cos(2 * np.pi * k / olm.N_FFT).astype(np.float32), np.sin(2 * np.pi * k / olm.N_FFT).astype(np.float32))


def _frames(wave, dtype):
    """[n, L] -> (windowless frames [n, live, 400] of the zero-padded, reflect-padded buffer, live)."""
    wave = np.asarray(wave, np.float32)
    live = olm.live_frames(wave.shape[1])
    xp = np.pad(olm.pad_or_trim(wave), ((0, 0), (olm.N_FFT // 2, olm.N_FFT // 2)), mode="reflect").astype(dtype)
    idx = np.arange(live)[:, None] * olm.HOP + np.arange(olm.N_FFT)[None, :]
    return xp[:, idx], live


def _finish_fp32(lg, live, divide):
    """fp32 raw log-mel of the live frames [n, n_mels, live] -> [n, n_mels, 3000] as both twins finish it."""
    f32 = np.float32
    assert lg.dtype == np.float32
    mx = lg.reshape(lg.shape[0], -1).max(axis=1)
    if live < olm.N_FRAMES:
        mx = np.maximum(mx, f32(-10.0))
    floor = (mx - f32(8.0))[:, None, None]
    aff = (lambda v: (v + f32(4.0)) / f32(4.0)) if divide else (lambda v: (v + f32(4.0)) * f32(0.25))
    out = np.empty(lg.shape[:2] + (olm.N_FRAMES,), np.float32)
    out[:, :, :live] = aff(np.maximum(lg, floor))
    out[:, :, live:] = aff(np.maximum(f32(-10.0), floor))
    return out


def _log10_once(mel32):
    return np.log10(np.maximum(mel32, np.float32(1e-10)).astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- yardsticks

def ideal_fp32(wave, n_mels):
    """float32 [n, n_mels, 3000]: the device dataflow in numpy float32 (see the module docstring)."""
    fr, live = _frames(wave, np.float32)
    n = fr.shape[0]
    a = fr * lib_window()[None, None, :]
    h = olm.N_FFT // 2
    ev = np.zeros((n, live, h + 1), np.float32)
    od = np.zeros((n, live, h + 1), np.float32)
    ev[..., 0], ev[..., h] = a[..., 0], a[..., h]
    b = a[..., :h:-1]                                       # a[400 - n], n = 1 .. 199
    ev[..., 1:h] = a[..., 1:h] + b
    od[..., 1:h] = a[..., 1:h] - b
    ct, st = _twiddles()
    k = np.arange(olm.N_FREQ)
    re = np.zeros((n, live, olm.N_FREQ), np.float32)
    im = np.zeros((n, live, olm.N_FREQ), np.float32)
    for j in range(h + 1):
        idx = (k * j) % olm.N_FFT
        re += ev[..., j, None] * ct[idx]
        im += od[..., j, None] * st[idx]
    pw = re * re + im * im
    fb = olm.mel_filter_bank(n_mels=n_mels).astype(np.float32)
    mel = np.zeros((n, live, n_mels), np.float32)
    for j in range(olm.N_FREQ):
        mel += pw[..., j, None] * fb[j]
    assert mel.dtype == np.float32
    return _finish_fp32(_log10_once(mel).transpose(0, 2, 1), live, divide=False)


def ideal_host(wave, n_mels):
    """float32 [n, n_mels, 3000]: the host twin's dataflow (csrc/logmel_host.cpp): the fp32 window table, the window
    product and the DFT in fp64, the powers rounded to fp32, an fp64 mel sum rounded to fp32 once per mel."""
    fr, live = _frames(wave, np.float64)
    spec = np.fft.rfft(fr * lib_window().astype(np.float64)[None, None, :], axis=-1)
    pw = (spec.real ** 2 + spec.imag ** 2).astype(np.float32).astype(np.float64)
    fb = olm.mel_filter_bank(n_mels=n_mels).astype(np.float32).astype(np.float64)
    mel = (pw @ fb).astype(np.float32)
    return _finish_fp32(_log10_once(mel).transpose(0, 2, 1), live, divide=True)


# ---------------------------------------------------------------------------------------------------- oracle, model

def e_model(out, parts, n_mels, frames):
    """The per-element bound of the module docstring on frames [0, frames): float64 [n, n_mels, frames]."""
    fb = olm.mel_filter_bank(n_mels=n_mels)
    d = U * parts["frame_norm"][:, None, :frames]                                  # [n, 1, F]
    a = parts["mag"][:, :, :frames]                                                # [n, 201, F]
    num = np.einsum("km,nkf->nmf", fb, 2.0 * a * d + d * d)
    mel = 10.0 ** parts["raw"][:, :, :frames].astype(np.float64)                   # already >= 1e-10
    return num / mel / (4.0 * np.log(10.0)) + 2.0 * U * np.maximum(np.abs(out[:, :, :frames]), 1.0)


class Case:
    """One batch with its fp64 oracle, cut to the frames the tests look at.  Nothing here is writable."""

    def __init__(self, wave, n_mels):
        self.wave, self.n_mels = wave, n_mels
        self.live = olm.live_frames(wave.shape[1])
        self.frames = min(olm.N_FRAMES, self.live + 3)
        out, parts = olm.log_mel(wave, dtype=np.float64, n_mels=n_mels, window=lib_window().astype(np.float64),
                                 return_parts=True)
        F = self.frames
        self.out = out[:, :, :F].copy()                        # float64 [n, n_mels, F]
        self.raw = parts["raw"][:, :, :F].copy()
        self.floor = parts["max"] - 8.0                        # [n], in log10 units
        self.e_model = e_model(out, parts, n_mels, F)
        self.pad = out[:, 0, olm.N_FRAMES - 1].copy()          # the value of a dead frame (frame 2999 of a full item)
        live_mask = np.arange(F)[None, None, :] < self.live
        fl = self.floor[:, None, None]
        self.unclamped = live_mask & (self.raw > fl)
        self.clamped = live_mask & (self.raw <= fl - NEAR)     # far enough below for any fp32 twin to clamp it too
        self.at_1e10 = live_mask & (self.raw == -10.0) & (fl < -10.0)
        am = self.raw.reshape(self.raw.shape[0], -1).argmax(axis=1)
        self.e_max = self.e_model.reshape(self.e_model.shape[0], -1)[np.arange(len(am)), am]   # bound of the maximum
        for v in vars(self).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    def ratio(self, got):
        """|got - oracle| / e_model on frames [0, frames): float64 [n, n_mels, frames]."""
        return np.abs(np.asarray(got, np.float64)[:, :, :self.frames] - self.out) / self.e_model


_CASES = {}


def cases(family, n_mels):
    """The family's batches as ``Case`` objects, computed once."""
    if (family, n_mels) not in _CASES:
        _CASES[(family, n_mels)] = [Case(w, n_mels) for w in batches(family)]
    return _CASES[(family, n_mels)]


def gamma(family, n_mels, fn=None):
    """max over the unclamped live elements of |fn(wave) - oracle| / e_model (``fn`` defaults to ``ideal_fp32``)."""
    fn = fn or ideal_fp32
    return max(float(c.ratio(fn(c.wave, n_mels))[c.unclamped].max()) for c in cases(family, n_mels))


def shares(family, n_mels):
    """(unclamped, clamped) share of the live-frame elements over the family's batches, by the oracle."""
    cs = cases(family, n_mels)
    total = sum(c.wave.shape[0] * n_mels * c.live for c in cs)
    return sum(int(c.unclamped.sum()) for c in cs) / total, sum(int(c.clamped.sum()) for c in cs) / total


def out_ulp(v):
    """The spacing of fp32 at max(|v|, 1): the unit the affine map's two roundings are counted in (the log10 is rounded at
    a magnitude of up to 16 and divided by four, the sum with 4.0 likewise: each at most half of this unit at |out| < 2)."""
    return np.spacing(np.maximum(np.abs(v), 1.0).astype(np.float32)).astype(np.float64)
