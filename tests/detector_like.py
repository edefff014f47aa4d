"""Detector-like strain for the whitening tests (a plain module, numpy only, deterministic per seed).

Real interferometer strain is steep: its amplitude spectral density (ASD) rises by about 1e6 between the 100 - 300 Hz bucket
and a few Hz, the in-band signal is about 1e-5 of the sample peak and narrow lines stand hundreds of times above the floor.
The spectrum here is analytic, so that nothing rests on a data file:

    ff  = max(f, 1 Hz)
    asd = 1e-23 (1 + (40 / ff)^4 + (12 / ff)^wall + ff / 400)            (wall = 0 drops that term)
    asd += 1e-23 (300 exp(-((f - 60) / 0.05)^2) + 1000 exp(-((f - 500.3) / 0.02)^2))    with lines

ASD range (max / min over the bins): 2.0e6 for wall 0 and wall 4, 4.4e6 for wall 6; in-band (> 20 Hz) rms 7e-6 .. 3e-5 of the
sample peak.
"""

import numpy as np

FS = 2048
IN_BAND_HZ = 20.0
SEED = 11                                  # of every input the whitening tests draw
# (wall, lines) of the cases the whitening tests use
CASES = [(0, False), (4, True), (6, True)]
SIZES = [2048 * 32, 2048 * 33 + 512]      # 127 (odd) and 132 (even) half-overlapping 0.5 s Welch segments


def asd(n, wall=4, lines=True):
    """The amplitude spectral density on rfftfreq(n, 1 / FS)."""
    f = np.fft.rfftfreq(n, 1.0 / FS)
    ff = np.maximum(f, 1.0)
    a = 1 + (40 / ff) ** 4 + ff / 400
    if wall:
        a = a + (12 / ff) ** wall
    a = 1e-23 * a
    if lines:
        a = a + 1e-23 * (300 * np.exp(-((f - 60) / 0.05) ** 2) + 1000 * np.exp(-((f - 500.3) / 0.02) ** 2))
    return a


def in_band(x):
    """x without everything at or below IN_BAND_HZ (an ideal high-pass)."""
    n = x.shape[-1]
    X = np.fft.rfft(x)
    X[..., np.fft.rfftfreq(n, 1.0 / FS) <= IN_BAND_HZ] = 0
    return np.fft.irfft(X, n)


def sine_gaussian(n, centre, peak, f0=150.0, sigma=0.010):
    t = (np.arange(n) - centre) / FS
    return peak * np.exp(-0.5 * (t / sigma) ** 2) * np.cos(2 * np.pi * f0 * t)


def glitch_centre(n):
    """A third of the way in: a 10 ms burst there lies inside at most 3 of the >= 127 Welch segments."""
    return n // 3


def strain(n, seed, wall=4, lines=True, glitch=False):
    """float64 [n], about 1e-17 at its peak.  glitch: a sine-Gaussian (150 Hz, sigma 10 ms) of 200 x the in-band rms."""
    rng = np.random.default_rng(seed)
    x = np.fft.irfft(np.fft.rfft(rng.standard_normal(n)) * asd(n, wall, lines), n) * np.sqrt(FS / 2)
    if glitch:
        x = x + sine_gaussian(n, glitch_centre(n), 200.0 * in_band(x).std())
    return x


def pair(n, seed, wall=4, lines=True, glitch=False):
    """[2, n]: two detectors, the second 3e-4 of the first in amplitude (another power-of-two scale)."""
    return np.stack([strain(n, seed, wall, lines, glitch), 3e-4 * strain(n, seed + 1000, wall, lines, glitch)])


def asd_range(n, wall, lines):
    a = asd(n, wall, lines)
    return float(a.max() / a.min())
