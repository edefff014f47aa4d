"""Whitening of the search pipeline's strain on the GPU.

Counterpart of ``whiten`` in the reference (``MLGWSC-1/inference.py:56-137``: PyCBC 2.4.0 ``TimeSeries.psd`` [Welch,
median] -> ``interpolate`` -> ``inverse_spectrum_truncation`` -> frequency-domain division -> drop the corrupted
edges), same signature and defaults, for ``[samples]`` or ``[detectors, samples]`` strain.

**Parity unpinned**: PyCBC is not installed in any environment this build can run in and the reference holds no
vector for this step; the arithmetic follows ``oracle/whiten.py`` (the restatement of the PyCBC routines with their
``delta_t`` / ``delta_f`` conventions) and is checked against it only.

Device work:

* The strain stays fp64 up to the filter's output.  Detector strain is steep: its in-band content lies at about 1e-5 of
  the sample peak, under a low-frequency wall 1e6 higher in amplitude that the filter removes by cancellation.  fp32
  samples (2^-24 of the peak each) lose 0.5 - 1.5 % of the whitened signal before any arithmetic
  (``tests/test_detector_like_host.py``), so samples, spectra, taps and sums are fp64 and only results are fp32.
* Welch spectra: the hann-windowed half-overlapping segments through the fp64 ``torch.fft.rfft`` (rocFFT, ``n_seg`` x 1024),
  rounded to fp32 per bin -- a relative 6e-8 there, whatever the bin's level -- then ``gww_welch_power_f32`` and the
  per-frequency median by radix select (``gww_column_median_f32``).  Whitening is invariant under a rescaling of the
  input, so every row is first brought to unit scale by an exact power of two (raw 1e-21 strain squares to 1e-42, below
  fp32; in-band power at unit scale is about 1e-10 of the peak's, far inside fp32).
* Filter design (a 513-point PSD in, a short FIR out): PyCBC's own sequence -- interpolate to the segment's frequency
  resolution, ``q = ifft(1 / sqrt(psd))``, hann-tapered truncation to ``max_filter_duration``, ``|fft(q)|`` -- in fp64
  with the N-point transforms of ``torch.fft`` (rocFFT); the result is read off as the impulse response
  ``h = irfft(|fft(q)|)``, which is ``max_filter_len`` taps long up to the tail the modulus adds.  The tail is kept until
  what is left out is below 1e-6 of the response in l1 AND would add less than 1e-4 of the whitened standard deviation
  for strain of the estimated PSD (``design_filter``: under a steep low-frequency wall the second test decides -- lined
  detector-like strain needs 1025 taps where 513 leak 0.07 - 0.13 per sample).  With a low-frequency cutoff the
  rectified stop-band ripple makes it too long for the FIR form (> 4097 taps): the response is then applied with the
  N-point transform, as the reference does.  Every row is designed and filtered on its own, so its result does not depend
  on the rows it is batched with.
* Filter application: ``gww_fir_f64`` -- the fp64 strain streams once through LDS against the fp64 taps, fp64 sums, fp32
  out (time domain, O(1) extra memory; circular padding reproduces the reference's circular convolution exactly) and
  the ``max_filter_len // 2`` corrupted samples on each side are never computed.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


def median_bias(n: int) -> float:
    """pycbc.psd.estimate.median_bias (host scalar)."""
    if n >= 1000:
        return math.log(2)
    ans = 1.0
    for i in range(1, int((n - 1) / 2 + 1)):
        ans += 1.0 / (2 * i + 1) - 1.0 / (2 * i)
    return ans


def welch_median_psd(x: torch.Tensor, delta_t: float, segment_duration: float):
    """``TimeSeries(x, delta_t).psd(segment_duration)`` for every row of x [D, N] (fp64, unit scale): (psd fp64 [D, L / 2 + 1],
    delta_f)."""
    D, n = x.shape
    seg_len = int(round(segment_duration / delta_t))
    stride = int(seg_len / 2)
    n_seg = int(n // stride)
    if (n_seg - 1) * stride + seg_len > n:
        n_seg -= 1
    data_len = (n_seg - 1) * stride + seg_len
    if n_seg < 1 or data_len > n:
        raise ValueError("whiten: not enough data for one PSD segment")
    diff = n - data_len
    start = diff // 2 + (diff % 2)
    n_bins = seg_len // 2 + 1
    hann = torch.from_numpy(np.hanning(seg_len)).to(x.device)
    delta_f = 1.0 / delta_t / seg_len
    wsum = float((np.hanning(seg_len) ** 2).sum())
    out = torch.empty((D, n_bins), dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream().cuda_stream
    for d in range(D):
        frames = x[d, start:start + data_len].as_strided((n_seg, seg_len), (stride, 1)) * hann
        # fp64 transform; each (re, im) then rounds to fp32 on its own, so a quiet bin is as exact as a loud one
        spec = torch.view_as_real(torch.fft.rfft(frames, dim=1)).float().reshape(n_seg, 2 * n_bins)
        power = torch.empty((n_seg, n_bins), dtype=torch.float32, device=x.device)
        med = torch.empty((n_bins,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib().gww_welch_power_f32(spec.data_ptr(), spec.shape[1], n_seg, n_bins, float(delta_t * delta_t),
                                            power.data_ptr(), stream), "gww_welch_power_f32")
            check(lib().gww_column_median_f32(power.data_ptr(), n_seg, n_bins, med.data_ptr(), stream),
                  "gww_column_median_f32")
        out[d] = med.double() / median_bias(n_seg) * (2 * delta_f * seg_len / wsum)
    return out, delta_f


K_MAX = 4095          # longest half-length of the time-domain form (gww_fir_f64 takes up to 8192 taps)


def design_filter(psd_w: torch.Tensor, delta_f_w: float, n: int, delta_t: float, max_filter_len: int,
                  low_frequency_cutoff=None, trunc_method="hann", tail: float = 1e-6, leak: float = 1e-4):
    """PyCBC's ``interpolate`` + ``inverse_spectrum_truncation`` for every row of psd_w (fp64 [D, bins]) at the resolution of an
    n-sample segment; returns the correlation taps g fp64 [D, taps4] (zero padded to a multiple of 4) and K with
    ``white[i] = sum_u g[u] x[(i - K + u) mod n]`` -- or ``(None, wf)`` with the frequency response ``|fft(q)|`` when the
    response does not fit ``K_MAX`` taps: the taps left out must hold less than ``tail`` of its l1 norm, and what they would
    have added to the output, for strain of this PSD, less than ``leak`` of the whitened standard deviation in rms."""
    D, bins = psd_w.shape
    dev = psd_w.device
    delta_f = 1.0 / (n * delta_t)
    new_n = int(np.rint((bins - 1) * delta_f_w / delta_f + 1))
    if new_n != n // 2 + 1:
        raise ValueError("whiten: the segment length does not match the PSD resolution (even sample count required)")
    f = torch.arange(new_n, dtype=torch.float64, device=dev) * delta_f
    pos = torch.clamp(f / delta_f_w, max=bins - 1)
    j = torch.clamp(pos.floor().long(), max=bins - 2)
    xp = j.double() * delta_f_w
    psd = psd_w[:, j] + (f - xp) * ((psd_w[:, j + 1] - psd_w[:, j]) / delta_f_w)          # numpy.interp
    N = (new_n - 1) * 2
    kmin = int(low_frequency_cutoff / delta_f) if low_frequency_cutoff else 1
    inv_asd = torch.zeros((D, new_n), dtype=torch.complex128, device=dev)
    inv_asd[:, kmin:N // 2] = (1.0 / psd[:, kmin:N // 2]).sqrt().to(torch.complex128)
    q = torch.fft.irfft(inv_asd, n=N, dim=1) * (N * delta_f)
    t0, t1 = max_filter_len // 2, N - max_filter_len // 2
    if t1 < t0:
        raise ValueError("Invalid value in inverse_spectrum_truncation")
    if trunc_method == "hann":
        win = torch.from_numpy(np.hanning(max_filter_len)).to(dev)
        q[:, :t0] *= win[-t0:]
        q[:, t1:] *= win[:max_filter_len // 2]
    if t0 < t1:
        q[:, t0:t1] = 0
    wf = (torch.fft.rfft(q, dim=1) * delta_t).abs()                 # (1 / psd_out) ** 0.5 = |fft(q)|
    h = torch.fft.irfft(wf.to(torch.complex128), n=N, dim=1)        # real, even: white = h (*) x circularly
    # keep the central taps until the rest is negligible (max_filter_len // 2 each side + what the modulus spreads: with a
    # low-frequency cutoff the rectified stop-band ripple decays slowly).  Negligible in two senses.  In l1, against any
    # input.  And in what it does to THIS strain: the full response is ~ 0 where the PSD is a wall 1e12 above the bucket, the
    # truncated one is not quite, and the wall leaks through the difference dH -- an error of variance sum_k dH_k^2 psd_k
    # delta_f next to the whitened variance 1 / (2 delta_t).  Steep detector strain fails that long before it fails the l1
    # test.  No K <= K_MAX passes both: return the frequency response instead and let the caller apply it with the
    # N-point transform.
    K = max(t0, 64)
    if K > K_MAX:             # a filter that is too long before any doubling (4 s at 2048 Hz: 2 K + 1 = 8193 taps)
        return None, wf
    total = h.abs().sum(dim=1)
    while True:
        rest = total - h[:, :K + 1].abs().sum(dim=1) - h[:, N - K:].abs().sum(dim=1)
        left_out = h.clone()
        left_out[:, :K + 1] = 0
        left_out[:, N - K:] = 0
        dH = torch.fft.rfft(left_out, dim=1).real
        leaked = ((dH * dH * psd).sum(dim=1) * delta_f * (2 * delta_t)).sqrt()
        if float((rest / total).max()) < tail and float(leaked.max()) < leak:
            break
        if 2 * K > K_MAX or 2 * K >= N // 2 - 1:
            return None, wf
        K *= 2
    taps = torch.cat((h[:, N - K:], h[:, :K + 1]), dim=1)            # h[-K .. K]
    g = taps.flip(1)                                                 # g[u] = h[K - u]
    taps4 = (g.shape[1] + 3) // 4 * 4
    gp = torch.zeros((D, taps4), dtype=torch.float64, device=dev)
    gp[:, :g.shape[1]] = g
    return gp, K


def whiten(strain, delta_t: float = 1.0 / 2048.0, segment_duration: float = 0.5, max_filter_duration: float = 0.25,
           trunc_method="hann", remove_corrupted: bool = True, low_frequency_cutoff=None, psd=None,
           return_psd: bool = False, device="cuda"):
    """Reference ``whiten`` (``MLGWSC-1/inference.py:56-137``): 1-D or [detectors, samples] strain -> whitened strain
    (fp32, on the GPU), ``max_filter_duration / 2`` seconds shorter on each side unless ``remove_corrupted=False``."""
    if psd is not None:
        raise NotImplementedError("whiten: only psd=None (estimate from the data, as MLGWSC-1/inference.py:225 calls it)")
    x = strain if torch.is_tensor(strain) else torch.from_numpy(np.asarray(strain))
    one_d = x.dim() == 1
    if one_d:
        x = x[None]
    if x.dim() != 2:
        raise ValueError("Strain must be 1D or 2D.")
    x = x.to(device)
    if not x.is_cuda:
        raise _lib.GwwError("whiten needs a GPU: gw_whisper_amd has no CPU path")
    D, n = x.shape
    if n % 2:
        raise ValueError("whiten: an even number of samples is required")
    # unit scale by an exact power of two, per row (whitening is scale invariant; fp32 cannot hold the square of 1e-21).
    # The samples stay fp64: in-band content at 1e-5 of the peak does not survive an fp32 cast.
    peaks = x.abs().amax(dim=1).double().tolist()
    scales = [2.0 ** (-math.floor(math.log2(p))) if p > 0 and math.isfinite(p) else 1.0 for p in peaks]
    scale = torch.tensor(scales, dtype=torch.float64, device=x.device)[:, None]
    xs = (x.double() * scale).contiguous()
    psd_w, df_w = welch_median_psd(xs, delta_t, segment_duration)
    max_filter_len = int(max_filter_duration * (1.0 / delta_t))
    cut = max_filter_len // 2 if remove_corrupted else 0
    n_out = n - 2 * cut
    out_stride = (n_out + 3) // 4 * 4
    out = torch.empty((D, out_stride), dtype=torch.float32, device=x.device)
    # row by row: the form and the length of a row's filter follow from its own PSD, never from the rows it is batched with
    for d in range(D):
        g, K = design_filter(psd_w[d:d + 1], df_w, n, delta_t, max_filter_len, low_frequency_cutoff, trunc_method)
        if g is None:
            # long response (low-frequency cutoff): the reference's own form, irfft(rfft(x) |fft(q)|), in fp64 (rocFFT)
            out[d, :n_out] = torch.fft.irfft(torch.fft.rfft(xs[d]) * K[0], n=n)[cut:n - cut]
            continue
        # circular padding: output i (= sample cut + i) needs x[(cut + i - K + u) mod n], u = 0 .. 2 K
        idx = (torch.arange(n_out + g.shape[1], device=x.device) + (cut - K)) % n
        pad = (n_out + g.shape[1] + 3) // 4 * 4
        xp = torch.zeros((pad,), dtype=torch.float64, device=x.device)
        xp[:idx.numel()] = xs[d, idx]
        with torch.cuda.device(x.device):
            check(lib().gww_fir_f64(xp.data_ptr(), pad, g.data_ptr(), g.shape[1], 1, out[d].data_ptr(), out_stride, n_out,
                                    torch.cuda.current_stream().cuda_stream), "gww_fir_f64")
    white = out[:, :n_out]
    if one_d:
        white = white[0]
    if return_psd:
        # the estimate in the input's units (the scaling above squared out again)
        p = psd_w / (scale * scale)
        return white, (p[0] if one_d else p)
    return white
