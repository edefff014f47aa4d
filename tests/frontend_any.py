"""The log-mel front end of ANY configuration restated in numpy (a plain module, numpy only, deterministic per seed): the
fp64 oracle, the ideal-fp32 yardstick of ``csrc/logmel_any.hip``'s documented dataflow and the per-element error model of
``tests/logmel_like.py`` with ``n_fft`` in place of 400.

    u = 2^-24,  d_f = u * ||windowed frame f||_2,  A_k = |X_k| of the oracle
    e_model[m, f] = sum_k fb[k, m] (2 A_k d_f + d_f^2) / max(mel[m, f], 1e-10) / (4 ln 10)  +  2 u max(|out|, 1)

The oracle is exact (fp64) arithmetic on the tables the library holds: the window ``float32(0.5 - 0.5 cos(2 pi n / n_fft))``
and the fp32-rounded slaney filterbank (``oracle.logmel.mel_filter_bank``, HF's ``mel_filter_bank`` for any band and rate).
``ideal_fp32`` is the kernel's dataflow with nothing the kernel does not have to do: fp32 window product, even / odd fold,
exactly rounded twiddles, one n-ordered multiply-add chain per sum (every product and sum rounded once), fp32 power and
mel.  ``GAMMA[i]`` is the worst ``|ideal_fp32 - oracle| / e_model`` over the unclamped live elements of configuration
``i``; the GPU test allows the kernel ``LIMIT`` x that (the kernel fuses its multiply-adds, the yardstick does not).
``tests/test_frontend_config_host.py`` re-derives the table on every run and holds it to 10 %.

The configurations and their seeded inputs are those of ``tools/make_golden_frontend.py`` (``tests/golden/
frontend_configs.npz`` holds HF's outputs for them).
"""

import numpy as np

from oracle import logmel as olm

LIMIT = 4.0                  # kernel error <= LIMIT x GAMMA x e_model (the project's factor, tests/logmel_like.py)
U = 2.0 ** -24
NEAR = 0.01                  # log10 distance from the clamp floor inside which an element counts as neither side's
N_SEG = 2

# (mels, rate, hop, chunk, n_fft, input samples, fmax): tools/make_golden_frontend.py
CONFIGS = (
    (80, 2048, 16, 2, 128, 2048, 8000),
    (80, 2048, 16, 2, 128, 2048, 1024),
    (80, 16000, 160, 2, 400, 16000, 8000),
    (80, 16000, 160, 1, 400, 16000, 8000),
    (128, 4000, 25, 1, 250, 3000, 2000),
    (80, 4096, 256, 4, 1024, 5000, 2048),
    (80, 2048, 8, 1, 64, 2048, 1024),
)
DEFAULT = (80, 16000, 160, 30, 400, 16000, 8000)     # Whisper's published configuration on 1 s of input

# max over the unclamped live elements of |ideal_fp32 - oracle| / e_model per configuration, and for DEFAULT; derived by
# test_frontend_config_host.py::test_ideal_fp32_reproduces_gamma
GAMMA = {
    0: 9.098e-01,
    1: 1.689e+00,
    2: 2.402e+00,
    3: 1.371e+00,
    4: 2.949e+00,
    5: 7.332e-01,
    6: 1.829e+00,
    "default": 1.805e+00,
}


class Cfg:
    """One configuration: the fields of ``gww_frontend_cfg`` and what follows from them."""

    def __init__(self, mels, rate, hop, chunk, n_fft, n_in, fmax, fmin=0.0):
        self.n_mels, self.rate, self.hop, self.chunk, self.n_fft, self.n_in = mels, rate, hop, chunk, n_fft, n_in
        self.fmin, self.fmax = float(fmin), float(fmax)
        self.n_samples = chunk * rate
        self.n_frames = self.n_samples // hop
        self.n_freq = n_fft // 2 + 1

    def live(self, n=None):
        """Leading frames that can see a non-zero sample of an input of n samples (all of them once the reflection at the
        far end of the chunk can reach the input)."""
        n = min(self.n_in if n is None else n, self.n_samples)
        if n >= self.n_samples - self.n_fft:
            return self.n_frames
        return min(self.n_frames, max(1, -(-(n + self.n_fft // 2) // self.hop)))

    def window(self):
        n = np.arange(self.n_fft, dtype=np.float64)
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / self.n_fft)).astype(np.float32)

    def filters(self):
        """float32 [n_freq, n_mels]: what both twins multiply with."""
        return olm.mel_filter_bank(self.n_freq, self.n_mels, self.fmin, self.fmax, self.rate).astype(np.float32)

    def extractor_kwargs(self):
        return dict(feature_size=self.n_mels, sampling_rate=self.rate, hop_length=self.hop, chunk_length=self.chunk,
                    n_fft=self.n_fft, min_frequency=self.fmin, max_frequency=self.fmax)


def cfg(i):
    return Cfg(*(DEFAULT if i == "default" else CONFIGS[i]))


def waves(i):
    """float32 [N_SEG, samples]: the seeded white-noise input of configuration i (tools/make_golden_frontend.py)."""
    c = cfg(i)
    seed = 1999 if i == "default" else 1000 + i
    return np.random.default_rng(seed).standard_normal((N_SEG, c.n_in)).astype(np.float32)


def _frames(c, wave, dtype):
    """[n, L] -> windowless frames [n, live, n_fft] of the zero-padded, reflect-padded buffer."""
    wave = np.asarray(wave, np.float32)
    live = c.live(wave.shape[1])
    buf = np.zeros((wave.shape[0], c.n_samples), np.float32)
    n = min(wave.shape[1], c.n_samples)
    buf[:, :n] = wave[:, :n]
    xp = np.pad(buf, ((0, 0), (c.n_fft // 2, c.n_fft // 2)), mode="reflect").astype(dtype)
    idx = np.arange(live)[:, None] * c.hop + np.arange(c.n_fft)[None, :]
    return xp[:, idx], live


def _log10_once(mel):
    return np.log10(np.maximum(mel, mel.dtype.type(1e-10)).astype(np.float64))


def oracle(c, wave):
    """fp64 on the library's tables: (out [n, n_mels, n_frames] float64, parts) with parts ``raw`` (log10 of the clamped
    mel energies, dead frames -10), ``max`` [n], ``frame_norm`` [n, live], ``mag`` [n, n_freq, live], ``live``."""
    fr, live = _frames(c, wave, np.float64)
    a = fr * c.window().astype(np.float64)[None, None, :]
    spec = np.fft.rfft(a, axis=-1)                                    # [n, live, n_freq]
    power = spec.real ** 2 + spec.imag ** 2
    mel = power @ c.filters().astype(np.float64)                      # [n, live, n_mels]
    raw = np.full((fr.shape[0], c.n_mels, c.n_frames), -10.0)
    raw[:, :, :live] = _log10_once(mel).transpose(0, 2, 1)
    mx = raw.reshape(raw.shape[0], -1).max(axis=1)
    out = (np.maximum(raw, (mx - 8.0)[:, None, None]) + 4.0) / 4.0
    parts = {"raw": raw, "max": mx, "frame_norm": np.sqrt((a ** 2).sum(axis=-1)), "live": live,
             "mag": np.sqrt(power).transpose(0, 2, 1)}
    return out, parts


def ideal_fp32(c, wave):
    """float32 [n, n_mels, n_frames]: the device dataflow of csrc/logmel_any.hip in numpy float32."""
    f32 = np.float32
    fr, live = _frames(c, wave, np.float32)
    n, N, h = fr.shape[0], c.n_fft, c.n_fft // 2
    a = fr * c.window()[None, None, :]
    ev = np.zeros((n, live, h + 1), f32)
    od = np.zeros((n, live, h + 1), f32)
    ev[..., 0], ev[..., h] = a[..., 0], a[..., h]
    b = a[..., :h:-1]                                       # a[n_fft - j], j = 1 .. h - 1
    ev[..., 1:h] = a[..., 1:h] + b
    od[..., 1:h] = a[..., 1:h] - b
    k = np.arange(N)
    ct, st = np.cos(2 * np.pi * k / N).astype(f32), np.sin(2 * np.pi * k / N).astype(f32)
    kk = np.arange(c.n_freq)
    re = np.zeros((n, live, c.n_freq), f32)
    im = np.zeros((n, live, c.n_freq), f32)
    for j in range(h + 1):
        idx = (kk * j) % N
        re += ev[..., j, None] * ct[idx]
        im += od[..., j, None] * st[idx]
    pw = re * re + im * im
    fb = c.filters()
    mel = np.zeros((n, live, c.n_mels), f32)
    for j in range(c.n_freq):
        mel += pw[..., j, None] * fb[j]
    assert mel.dtype == f32
    lg = _log10_once(mel).astype(f32).transpose(0, 2, 1)    # [n, n_mels, live]
    mx = lg.reshape(n, -1).max(axis=1)
    if live < c.n_frames:
        mx = np.maximum(mx, f32(-10.0))
    floor = (mx - f32(8.0))[:, None, None]
    out = np.empty((n, c.n_mels, c.n_frames), f32)
    out[:, :, :live] = (np.maximum(lg, floor) + f32(4.0)) * f32(0.25)
    out[:, :, live:] = (np.maximum(f32(-10.0), floor) + f32(4.0)) * f32(0.25)
    return out


def e_model(c, out, parts):
    """The per-element bound of the module docstring on the live frames: float64 [n, n_mels, live]."""
    live = parts["live"]
    fb = c.filters().astype(np.float64)
    d = U * parts["frame_norm"][:, None, :]                                        # [n, 1, live]
    num = np.einsum("km,nkf->nmf", fb, 2.0 * parts["mag"] * d + d * d)
    mel = 10.0 ** parts["raw"][:, :, :live]                                        # already >= 1e-10
    return num / mel / (4.0 * np.log(10.0)) + 2.0 * U * np.maximum(np.abs(out[:, :, :live]), 1.0)


class Case:
    """One configuration's seeded batch with its fp64 oracle.  Nothing here is writable."""

    def __init__(self, i):
        self.key, self.cfg = i, cfg(i)
        self.wave = waves(i)
        self.out, parts = oracle(self.cfg, self.wave)
        self.live = parts["live"]
        self.raw = parts["raw"][:, :, :self.live].copy()
        self.floor = parts["max"] - 8.0                            # [n], log10 units
        self.e_model = e_model(self.cfg, self.out, parts)
        self.pad = (np.maximum(-10.0, self.floor) + 4.0) / 4.0     # the value of a dead frame, [n]
        fl = self.floor[:, None, None]
        self.unclamped = self.raw > fl + NEAR
        self.clamped = self.raw <= fl - NEAR                       # far enough below for any fp32 twin to clamp it too
        self.near = ~self.unclamped & ~self.clamped
        am = self.raw.reshape(self.raw.shape[0], -1).argmax(axis=1)
        self.e_max = self.e_model.reshape(self.e_model.shape[0], -1)[np.arange(len(am)), am]   # bound of the maximum
        for v in vars(self).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    def ratio(self, got):
        """|got - oracle| / e_model on the live frames: float64 [n, n_mels, live]."""
        return np.abs(np.asarray(got, np.float64)[:, :, :self.live] - self.out[:, :, :self.live]) / self.e_model


_CASES = {}


def case(i):
    if i not in _CASES:
        _CASES[i] = Case(i)
    return _CASES[i]


def gamma(i):
    c = case(i)
    return float(c.ratio(ideal_fp32(c.cfg, c.wave))[c.unclamped].max())
