"""Glitch-like segments, the ideal-fp32 yardstick and the error envelopes of the Q-scan tests (a plain module, numpy only,
deterministic per seed).

The Q-scan's tile energies are median-normalised: the noise floor sits near 1 whatever else the segment holds, and a loud
transient stands 1e2 .. 1e7 above it.  The tests built on this module hold every tile and every pixel to an error relative
to its OWN size (floored at 0.1), not to the segment's largest value.

Yardstick: ``ideal_fp32`` / ``ideal_interp_fp32`` restate the documented dataflow of ``csrc/qscan.hip`` in numpy float32 with
nothing the kernels do not have to do: exactly rounded twiddles, one k-ordered multiply-add chain per sum (every product and
sum rounded once: plain elementwise numpy, so the figures do not depend on a BLAS), an exact median, a true divide.  What
that restatement is off the fp64 oracle by, on a family of inputs, is what fp32 costs there; the GPU tests allow the kernels
``LIMIT`` = 4 x that (accumulation order, fused multiply-adds, the hardware sine / cosine of the twiddle table).  The
constants below were derived on a CPU by ``test_qscan_like_host.py``, which re-derives them on every run.
"""

import numpy as np

from gw_whisper_amd.qscan import QScanTables, rdft_matrix
from oracle import qscan as oq

FS = 2048
N = 2048                     # 1 s at 2048 Hz: the only configuration the tables admit
QRANGE = (4, 128)
FLOOR = 0.1                  # of both envelopes
LIMIT = 4.0                  # kernel error <= LIMIT x the yardstick constant
SEED = 0                     # of every batch the tests draw
B_TILE = 5                   # one full group of four items and a ragged one

FAMILIES = ("noise", "chirp", "glitch1e2", "glitch1e3", "glitch_hf", "glitch_edge", "line", "offset", "gated")

# |e - e_ref| / max(e_ref, 0.1) of ideal_fp32 against the fp64 oracle on segments(family, B_TILE, SEED), over row_subset():
# (rms over tiles, worst tile).  Derived by test_qscan_like_host.py::test_yardstick_constants (which holds them to 10 %).
TILE_YARDSTICK = {
    "noise": (2.155e-06, 1.502e-05),
    "chirp": (3.961e-06, 8.705e-05),
    "glitch1e2": (1.556e-05, 4.729e-04),
    "glitch1e3": (1.352e-04, 3.182e-03),
    "glitch_hf": (9.405e-06, 1.050e-04),
    "glitch_edge": (2.095e-05, 4.344e-04),
    "line": (9.026e-06, 2.596e-04),
    "offset": (7.143e-06, 1.553e-04),
    "gated": (1.602e-06, 1.857e-05),
}

# Interpolation alone: the oracle's energies of interp_batch() rounded to fp32, every plane in turn; worst pixel's
# |ideal_interp_fp32 - fp64| / E_pix over the five planes.  "rows" stands for (that plane's own row count, 256).
INTERP_SHAPES = ((128, 128), (512, 512), (80, 300), "rows", (33, 2048))
INTERP_YARDSTICK = {
    (128, 128): 6.019e-06,
    (512, 512): 3.165e-03,
    (80, 300): 1.813e-04,
    "rows": 1.364e-07,
    (33, 2048): 1.764e-05,
}


# ---------------------------------------------------------------------------------------------------- segments

def sine_gaussian(f0, sigma, centre, peak):
    t = np.arange(N) / FS - centre
    return peak * np.exp(-0.5 * (t / sigma) ** 2) * np.cos(2 * np.pi * f0 * t)


def chirp(amplitude):
    """The chirp of test_gpu_qscan.py::_signals."""
    t = np.arange(N) / FS
    return amplitude * np.sin(2 * np.pi * (60 + 300 * t) * t) * np.exp(-((t - 0.55) / 0.08) ** 2)


def segments(family, n, seed=SEED):
    """float32 [n, 2048]: seeded unit-variance Gaussian noise (the same draw for every family) plus the family's feature.
    Both the kernels and the oracle are given these fp32 values: the input's own rounding is not part of any error."""
    x = np.random.default_rng(seed).standard_normal((n, N))
    t = np.arange(N) / FS
    if family == "noise":
        pass
    elif family == "chirp":
        for i in range(n):
            x[i] += chirp(3.0 + 2.0 * (i % 5))            # amplitudes 3 .. 11
    elif family == "glitch1e2":
        x += sine_gaussian(150.0, 0.010, 0.55, 1e2)
    elif family == "glitch1e3":
        x += sine_gaussian(150.0, 0.010, 0.55, 1e3)
    elif family == "glitch_hf":
        x += sine_gaussian(700.0, 0.002, 0.55, 1e2)
    elif family == "glitch_edge":
        x += sine_gaussian(150.0, 0.010, 0.01, 1e2)       # cut off at t = 0: the circular transform wraps its response
    elif family == "line":
        x += 100.0 * np.sin(2 * np.pi * 60.0 * t)
    elif family == "offset":
        x += 50.0                                          # DC lies outside every window: only DFT leakage can show it
    elif family == "gated":
        x[:, int(0.3 * FS):int(0.6 * FS)] = 0.0
    else:
        raise KeyError(family)
    return x.astype(np.float32)


def interp_batch():
    """The two items whose oracle energies the interpolation-alone tests resample: a loud glitch and plain noise."""
    return np.concatenate([segments("glitch1e2", 1), segments("noise", 2)[1:]])


# ---------------------------------------------------------------------------------------------------- geometry

_TABLES = []


def tables():
    if not _TABLES:
        _TABLES.append(QScanTables(1.0, FS, QRANGE))
    return _TABLES[0]


def row_subset():
    """Every fourth row of each plane plus its first and last: contains every ntiles class (asserted)."""
    t = tables()
    rows = sorted({r for r0, nr in t.plane_rows for r in list(range(r0, r0 + nr, 4)) + [r0, r0 + nr - 1]})
    assert set(t.rows[rows, 1]) == set(t.rows[:, 1]) == {128, 256, 512, 1024, 2048}
    return rows


def oracle(x, shape=(128, 128)):
    """fp64 oracle on the fp32 segments: (map [B, F, T], plane, energies [n_rows] of [B, ntiles] in table order, the plane
    maxima).  Nothing returned is writable."""
    out, best, per_plane = oq.qscan(x.astype(np.float64), spectrogram_shape=shape, qrange=QRANGE, return_energies=True)
    maxima = np.array([max(float(e.max()) for e in plane) for plane in per_plane])
    flat = [e for plane in per_plane for e in plane]
    for a in [out] + flat:
        a.setflags(write=False)
    return out, best, flat, maxima


def mixed_batch():
    """[9, 2048]: item i is item i of family i's batch of nine (every family once, nine different noise draws)."""
    return np.stack([segments(f, len(FAMILIES))[i] for i, f in enumerate(FAMILIES)])


def zero_row_batches():
    """([noise, zeros, glitch1e2], [noise, glitch1e2]): the same two items with and without an all-zero one between."""
    a, b = segments("noise", 1)[0], segments("glitch1e2", 3)[2]
    return np.stack([a, np.zeros(N, np.float32), b]), np.stack([a, b])


_CASES = {}


def family_case(family):
    """(x fp32 [B_TILE, 2048], chosen plane, energies per table row, plane maxima) of one family, computed once."""
    if family not in _CASES:
        x = segments(family, B_TILE)
        x.setflags(write=False)
        _, best, flat, maxima = oracle(x)
        _CASES[family] = (x, best, flat, maxima)
    return _CASES[family]


def plane_energies(flat, plane):
    r0, nr = tables().plane_rows[plane]
    return flat[r0:r0 + nr]


# ---------------------------------------------------------------------------------------------------- yardsticks

def _twiddles(n):
    """cos, sin of 2 pi m / n rounded to fp32 from fp64, exact zeros where the angle is a multiple of pi / 2."""
    m = np.arange(n)
    c, s = np.cos(2 * np.pi * m / n), np.sin(2 * np.pi * m / n)
    c[[n // 4, 3 * n // 4]] = 0.0
    s[[0, n // 2]] = 0.0
    return c.astype(np.float32), s.astype(np.float32)


def fseries_fp32(x):
    """x fp32 [B, 2048] -> fp32 [B, 2052]: the DFT GEMM as one k-ordered chain per output."""
    m = rdft_matrix(N)                                   # [2052, 2048] fp32
    acc = np.zeros((x.shape[0], m.shape[0]), np.float32)
    for k in range(N):
        acc += x[:, k, None] * m[None, :, k]
    return acc


def ideal_fp32(x, rows):
    """{row: fp32 [B, ntiles]}: the normalised tile energies of the given table rows by the documented dataflow in fp32."""
    t = tables()
    x = np.asarray(x)
    assert x.dtype == np.float32
    f = fseries_fp32(x)
    out = {}
    for r in rows:
        _, n, ws, idx0, _, woff = (int(v) for v in t.rows[r])
        w = t.window[woff:woff + ws]
        cx = w[None, :] * f[:, 2 * idx0:2 * (idx0 + ws):2]
        cy = w[None, :] * f[:, 2 * idx0 + 1:2 * (idx0 + ws) + 1:2]
        twc, tws = _twiddles(n)
        tt = np.arange(n)
        ar = np.zeros((x.shape[0], n), np.float32)
        ai = np.zeros((x.shape[0], n), np.float32)
        for k in range(ws):
            j = (k * tt) & (n - 1)
            wx, wy = twc[j][None, :], tws[j][None, :]
            a, b = cx[:, k, None], cy[:, k, None]
            ar += a * wx - b * wy
            ai += a * wy + b * wx
        e = (ar * ar + ai * ai) * np.float32(1.0 / (float(n) * float(n)))
        s = np.sort(e, axis=-1)
        med = np.float32(0.5) * (s[:, n // 2 - 1] + s[:, n // 2])
        out[r] = e / med[:, None]
        assert out[r].dtype == np.float32
    return out


_A = np.float32(-0.75)


def _cubic4_f32(t):
    """k_qscan_interp's cubic4 in float32, the same expressions."""
    one, two = np.float32(1.0), np.float32(2.0)

    def c1(x):
        return ((_A + np.float32(2.0)) * x - (_A + np.float32(3.0))) * x * x + one

    def c2(x):
        return ((_A * x - np.float32(5.0) * _A) * x + np.float32(8.0) * _A) * x - np.float32(4.0) * _A
    return [c2(t + one), c1(t), c1(one - t), c2(two - t)]


def _src_f32(n_out, n_in):
    """(first tap's index, 4 weights): the source index is (o + 0.5) * (n / T) - 0.5 in fp32, as the kernel writes it."""
    o = np.arange(n_out, dtype=np.float32)
    src = (o + np.float32(0.5)) * (np.float32(n_in) / np.float32(n_out)) - np.float32(0.5)
    fl = np.floor(src)
    assert src.dtype == np.float32
    return fl.astype(np.int64), _cubic4_f32(src - fl)


def ideal_interp_fp32(rows, F, T):
    """One plane's energies (fp32 [B, ntiles(row)] per row) -> fp32 [B, F, T]: the two-pass bicubic in numpy float32."""
    nr = len(rows)
    timed = []
    for e in rows:
        e = np.asarray(e)
        assert e.dtype == np.float32
        n = e.shape[-1]
        if n == T:
            timed.append(e.copy())
            continue
        ti, wt = _src_f32(T, n)
        v = np.zeros(e.shape[:-1] + (T,), np.float32)
        for c in range(4):
            v = wt[c] * e[..., np.clip(ti - 1 + c, 0, n - 1)] + v
        timed.append(v)
    timed = np.stack(timed, axis=-2)                     # [B, nr, T]
    if nr == F:
        return timed
    fi, wf = _src_f32(F, nr)
    acc = np.zeros(timed.shape[:-2] + (F, T), np.float32)
    for a in range(4):
        acc = wf[a][:, None] * timed[..., np.clip(fi - 1 + a, 0, nr - 1), :] + acc
    assert acc.dtype == np.float32
    return acc


# ---------------------------------------------------------------------------------------------------- envelopes, errors

def e_tile(e_ref):
    return np.maximum(e_ref, FLOOR)


def e_pix(plane_rows_ref, shape):
    """sum over a pixel's 16 taps of |w_f| |w_t| max(e_ref, 0.1)."""
    return oq.interpolate_plane([e_tile(e) for e in plane_rows_ref], shape, abs_weights=True)


def rel_errors(got, ref, env):
    """(rms, worst) of |got - ref| / env over everything given: arrays, or lists of arrays (one per row or item)."""
    if isinstance(got, np.ndarray):
        got, ref, env = [got], [ref], [env]
    q = [np.abs(np.asarray(g, np.float64) - r) / v for g, r, v in zip(got, ref, env)]
    total = sum(a.size for a in q)
    rms = float(np.sqrt(sum(float((a ** 2).sum()) for a in q) / total))
    worst = max(float(a.max(axis=-1).max()) for a in q)          # per (row, item) first, then the worst of those
    return rms, worst


def quiet_fraction(e_ref):
    """Per item: the share of a row's tiles with 0.1 <= e_ref <= 10."""
    return ((e_ref >= 0.1) & (e_ref <= 10.0)).mean(axis=-1)


def interp_shape(shape, plane):
    return (int(tables().plane_rows[plane][1]), 256) if shape == "rows" else shape
