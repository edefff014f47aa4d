"""Q-transform front end #2: ``QScan`` / ``QTransformAdapter`` as the reference's MLGWSC-1 pipeline uses them
(``MLGWSC-1/train.py:45,78-154``, ``inference.py:28,300-351``), backed by the HIP kernels of ``csrc/qscan.hip``.

**Parity unpinned.**  ``ml4gw.transforms.QScan`` is a third-party dependency the reference neither vendors nor pins
and that is not installed anywhere this build runs; the tiling below restates the published constant-Q transform
(Chatterji 2004; GWpy ``qtransform``; ml4gw ``transforms/qtransform.py`` conventions as known when this was
written) and is checked only against the independent CPU restatement ``oracle/qscan.py``.

``QScan(duration, sample_rate, spectrogram_shape, qrange)(x [B, N])`` -> ``[B, F, T]``: forward-normalised real DFT
(one fp32 MFMA GEMM against a cached DFT matrix), windowed tile energies + median normalisation per (Q plane,
frequency row), the plane with the largest energy over the whole batch, bicubic resampling.  ``QTransformAdapter``
is the reference's module with the same parameter names: Q-scan (no grad) -> small CNN (plain ``torch.nn``, 0.3 GFLOP
per sample, 1 % of the encoder) -> adaptive pool to (80, 3000) + global and per-detector affine + the stack over
detectors as ONE HIP kernel (``gww_qadapter_tail_f32``); it trains through the frozen encoder via the encoder's input
gradient.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib

_CLASSES = (128, 256, 512, 1024, 2048)


def _plane_qs(qrange, mismatch):
    deltam = 2 * (mismatch / 3.0) ** 0.5
    cumum = math.log(qrange[1] / qrange[0]) / 2 ** 0.5
    nplanes = int(max(math.ceil(cumum / deltam), 1))
    dq = cumum / nplanes
    return [qrange[0] * math.exp(2 ** 0.5 * dq * (i + 0.5)) for i in range(nplanes)]


def _plane_freqs(q, duration, sample_rate, mismatch, frange):
    qprime = q / 11 ** 0.5
    minf = max(frange[0], 50 * q / (2 * math.pi * duration))
    maxf = min(frange[1], sample_rate / 2 / (1 + 1 / qprime))
    fcum = math.log(maxf / minf) * (2 + q ** 2) ** 0.5 / 2.0
    deltam = 2 * (mismatch / 3.0) ** 0.5
    nfreq = int(max(1, math.ceil(fcum / deltam)))
    fstep = fcum / nfreq
    base = np.exp(2 / ((2 + q ** 2) ** 0.5) * (np.arange(0, nfreq) + 0.5) * fstep)
    return np.unique((minf * base // (1 / duration)) * (1 / duration))


class QScanTables:
    """Static geometry of a Q-scan, in the layout ``gww_qscan_energy_f32`` / ``gww_qscan_interp_f32`` take."""

    def __init__(self, duration: float, sample_rate: float, qrange: Sequence[float], mismatch: float = 0.2,
                 frange: Tuple[float, float] = (0.0, math.inf)):
        rows, windows, plane_rows = [], [], []
        e_off = w_off = 0
        n_bins = int(round(duration * sample_rate)) // 2 + 1
        for p, q in enumerate(_plane_qs(qrange, mismatch)):
            freqs = _plane_freqs(q, duration, sample_rate, mismatch, frange)
            plane_rows.append((len(rows), len(freqs)))
            qprime = q / 11 ** 0.5
            for f in freqs:
                ws = 2 * int(f / qprime * duration) + 1
                ntiles = int(2 ** math.ceil(math.log2(duration * 2 * math.pi * f / q / (2 * (mismatch / 3.0) ** 0.5))))
                half = int((ws - 1) / 2.0)
                k = np.arange(-half, half + 1)
                x = (k / duration) * qprime / f
                norm = ntiles / (duration * sample_rate) * (315 * qprime / (128 * f)) ** 0.5
                idx = np.round(k + 1 + f * duration).astype(np.int64)
                if ntiles not in _CLASSES or ws > 704 or idx[0] < 0 or idx[-1] >= n_bins:
                    raise _lib.GwwError(f"Q-scan tile outside the kernel's limits: q={q:.2f} f={f:.1f} ntiles={ntiles} ws={ws}")
                rows.append((p, ntiles, ws, int(idx[0]), e_off, w_off))
                windows.append(((1 - x ** 2) ** 2 * norm).astype(np.float32))
                e_off += ntiles
                w_off += ws
        self.rows = np.asarray(rows, np.int32)
        self.window = np.concatenate(windows)
        self.plane_rows = np.asarray(plane_rows, np.int32)
        self.e_total = e_off
        self.n_bins = n_bins
        order = np.argsort(self.rows[:, 1], kind="stable").astype(np.int32)
        self.order = order
        nt = self.rows[order, 1]
        self.class_ranges = np.asarray([[int(np.searchsorted(nt, c, "left")), int(np.searchsorted(nt, c, "right"))]
                                        for c in _CLASSES], np.int32)


def rdft_matrix(n: int) -> np.ndarray:
    """[>= 2 (n/2+1), n] fp32: rows (2 j, 2 j + 1) = real / imaginary part of ``rfft(x, norm='forward')[j]``, positive
    frequencies doubled (``X[..., 1:] *= 2`` of ml4gw's SingleQTransform)."""
    j = np.arange(n // 2 + 1)[:, None].astype(np.float64)
    k = np.arange(n)[None, :].astype(np.float64)
    ang = 2 * np.pi * j * k / n
    s = np.where(j == 0, 1.0, 2.0) / n
    rows = 2 * (n // 2 + 1)
    m = np.zeros(((rows + 3) // 4 * 4, n), np.float64)       # the GEMM wants N % 4 == 0: zero rows at the end
    m[0:rows:2] = np.cos(ang) * s
    m[1:rows:2] = -np.sin(ang) * s
    return m.astype(np.float32)


class QScan(nn.Module):
    """``ml4gw.transforms.QScan`` call surface: ``QScan(duration, sample_rate, spectrogram_shape, qrange)(x)``."""

    def __init__(self, duration: float, sample_rate: float, spectrogram_shape: Sequence[int] = (128, 128),
                 qrange: Sequence[float] = (1, 1000), frange: Sequence[float] = (0.0, math.inf), mismatch: float = 0.2):
        super().__init__()
        self.duration, self.sample_rate = duration, sample_rate
        self.spectrogram_shape = tuple(int(v) for v in spectrogram_shape)
        self.tables = QScanTables(duration, sample_rate, qrange, mismatch, tuple(frange))
        self._dev = {}
        self.last_plane = None

    def _device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            t = self.tables
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev[key] = dict(rows=up(t.rows), order=up(t.order), window=up(t.window), plane_rows=up(t.plane_rows),
                                  dft=up(rdft_matrix(int(round(self.duration * self.sample_rate)))))
        return self._dev[key]

    @torch.no_grad()
    def forward(self, X: torch.Tensor) -> torch.Tensor:
        from . import ops
        if not X.is_cuda:
            raise _lib.GwwError("QScan needs a GPU tensor: gw_whisper_amd has no CPU path")
        lead = X.shape[:-1]
        x = X.reshape(-1, X.shape[-1]).to(torch.float32).contiguous()
        n = int(round(self.duration * self.sample_rate))
        if x.shape[-1] != n:
            raise ValueError(f"QScan was built for {n} samples, got {x.shape[-1]}")
        t, d = self.tables, self._device_tables(x.device)
        B = x.shape[0]
        F, T = self.spectrogram_shape
        fser = ops.gemm(x, d["dft"], None, 0)                       # [B, 2 n_bins]
        energy = torch.empty((B, t.e_total), dtype=torch.float32, device=x.device)
        n_planes = len(t.plane_rows)
        pmax = torch.empty((n_planes,), dtype=torch.int32, device=x.device)
        chosen = torch.empty((1,), dtype=torch.int32, device=x.device)
        out = torch.empty((B, F, T), dtype=torch.float32, device=x.device)
        cr = (C.c_int * 10)(*[int(v) for v in t.class_ranges.reshape(-1)])
        stream = torch.cuda.current_stream().cuda_stream
        with torch.cuda.device(x.device):
            check(lib().gww_qscan_energy_f32(fser.data_ptr(), fser.shape[1], B, d["rows"].data_ptr(), d["order"].data_ptr(),
                                             cr, d["window"].data_ptr(), energy.data_ptr(), t.e_total, pmax.data_ptr(),
                                             n_planes, stream), "gww_qscan_energy_f32")
            check(lib().gww_qscan_interp_f32(energy.data_ptr(), t.e_total, d["rows"].data_ptr(), d["plane_rows"].data_ptr(),
                                             n_planes, pmax.data_ptr(), B, F, T, out.data_ptr(), chosen.data_ptr(), stream),
                  "gww_qscan_interp_f32")
        self.last_plane = chosen          # device int: which Q plane won (no host sync here)
        return out.reshape(*lead, F, T)


class _AdapterTail(torch.autograd.Function):
    """pool -> global affine -> FiLM of one detector as ONE HIP kernel that writes into the stacked feature tensor
    (``gww_qadapter_tail_f32``).  Backward (the adapter trains through the frozen encoder, MLGWSC-1/train.py:494-504):
    ONE HIP pass as well (``gww_qadapter_tail_backward_f32``) -- training-side only, the inference path never runs it."""

    @staticmethod
    def forward(ctx, y, scale, bias, gamma, beta, out, det):
        B, Hin, Win = y.shape
        F, T = out.shape[-2:]
        yc = y.detach().to(torch.float32).contiguous()
        view = out[:, det]
        with torch.cuda.device(y.device):
            check(lib().gww_qadapter_tail_f32(yc.data_ptr(), B, Hin, Win, scale.data_ptr(), bias.data_ptr(),
                                              gamma[det:det + 1].data_ptr(), beta[det:det + 1].data_ptr(),
                                              view.data_ptr(), out.stride(0), F, T,
                                              torch.cuda.current_stream().cuda_stream), "gww_qadapter_tail_f32")
        ctx.save_for_backward(yc, scale, bias, gamma)
        ctx.det, ctx.shape = det, (F, T)
        ctx.mark_dirty(out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        from . import ops
        y, scale, bias, gamma = ctx.saved_tensors
        det = ctx.det
        F, T = ctx.shape
        # one HIP pass over g_out[:, det]: the adaptive-pool backward as a fixed-order gather and the four scalar
        # gradients from fixed-order partials (gww_qadapter_tail_backward_f32; no float atomics, reproducible bits)
        d_y, d_scale, d_bias, d_gam, d_bet = ops.qadapter_tail_backward(g_out[:, det], y, scale, bias, gamma[det:det + 1],
                                                                        F, T)
        d_gamma = torch.zeros_like(gamma)
        d_gamma[det:det + 1] = d_gam
        d_beta = torch.zeros_like(gamma)
        d_beta[det:det + 1] = d_bet
        g_rest = g_out.clone()
        g_rest[:, det] = 0                                                    # this call overwrote detector `det` of `out`
        return d_y, d_scale, d_bias, d_gamma, d_beta, g_rest, None


class _CnnFunction(torch.autograd.Function):
    """``freq_adapter(qspec[:, None])[:, 0]`` with BOTH directions as HIP kernels (``gww_qadapter_cnn_forward_f32`` /
    ``gww_qadapter_cnn_backward_f32``): the training step of the adapter (MLGWSC-1/train.py:494-504) makes no library
    convolution call either.  The Q-scan map needs no gradient (the reference computes it under ``no_grad``, :139-141); the
    forward saves only its input, the backward recomputes the activations."""

    @staticmethod
    def forward(ctx, adapter, qspec, w1, b1, w2, b2, w3, b3, w4, b4):
        y = adapter.cnn_forward(qspec)
        ctx.adapter = adapter
        ctx.save_for_backward(qspec.detach().to(torch.float32).contiguous(), w2.detach(), w3.detach())
        return y

    @staticmethod
    def backward(ctx, dy):
        qspec, w2, w3 = ctx.saved_tensors
        ad = ctx.adapter
        packed, ch = ad._packed_cnn()
        B, H, W = qspec.shape
        dev = qspec.device
        c1, c2, c3 = ch
        g = [torch.empty(s, dtype=torch.float32, device=dev) for s in
             ((c1, 1, 3, 3), (c1,), (c2, c1, 3, 3), (c2,), (c3, c2, 3, 3), (c3,), (1, c3, 1, 1), (1,))]
        need = lib().gww_qadapter_cnn_backward_workspace_bytes(B, H, W, c1, c2, c3)
        ws = getattr(ad, "_cnn_bwd_ws", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = ad._cnn_bwd_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dyc = dy.to(torch.float32).contiguous()
        w2c, w3c = w2.to(torch.float32).contiguous(), w3.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            check(lib().gww_qadapter_cnn_backward_f32(qspec.data_ptr(), dyc.data_ptr(), B, H, W, packed.data_ptr(),
                                                      w2c.data_ptr(), w3c.data_ptr(), c1, c2, c3, ws.data_ptr(), ws.numel(),
                                                      *[t.data_ptr() for t in g], torch.cuda.current_stream().cuda_stream),
                  "gww_qadapter_cnn_backward_f32")
        return (None, None, *g)


class QTransformAdapter(nn.Module):
    """The reference's Q-transform adapter, both variants, same constructor arguments, parameter names and forward:

    * ``MLGWSC-1/train.py:78-154``  -- ``spectrogram_shape=[128, 128]``, CNN channels 1 -> 32 -> 64 -> 128 -> 1
      (the defaults here, ``QTransformAdapter.train_variant``);
    * ``MLGWSC-1/inference.py:303-351`` -- ``spectrogram_shape=[512, 512]``, channels 1 -> 16 -> 32 -> 64 -> 1
      (``QTransformAdapter.inference_variant``; ``build_model`` :425-426 loads its ``state_dict``).

    ``channels`` is the one argument the reference does not have (it hard-codes the widths per file);
    ``from_state_dict`` picks the variant from a checkpoint's tensor shapes."""

    TRAIN_CHANNELS = (32, 64, 128)
    INFERENCE_CHANNELS = (16, 32, 64)

    def __init__(self, kernel_length: float = 1.0, sample_rate: int = 2048, q_range: List[int] = [4, 128],
                 spectrogram_shape: List[int] = [128, 128], target_shape: Tuple[int, int] = (80, 3000),
                 n_detectors: int = 2, channels: Sequence[int] = TRAIN_CHANNELS):
        super().__init__()
        self.n_detectors = n_detectors
        self.target_shape = tuple(int(v) for v in target_shape)
        self.q_transform = QScan(duration=kernel_length, sample_rate=sample_rate, spectrogram_shape=spectrogram_shape,
                                 qrange=q_range)
        c1, c2, c3 = (int(c) for c in channels)
        self.freq_adapter = nn.Sequential(
            nn.Conv2d(1, c1, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(c1, c2, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(c2, c3, 3, padding=1), nn.ReLU(),
            nn.Conv2d(c3, 1, 1))
        self.final_pool = nn.AdaptiveAvgPool2d(self.target_shape)
        self.scale = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))
        self.film_gamma = nn.Parameter(torch.ones(self.n_detectors))
        self.film_beta = nn.Parameter(torch.zeros(self.n_detectors))

    @classmethod
    def train_variant(cls, **kw) -> "QTransformAdapter":
        return cls(spectrogram_shape=[128, 128], channels=cls.TRAIN_CHANNELS, **kw)

    @classmethod
    def inference_variant(cls, **kw) -> "QTransformAdapter":
        return cls(spectrogram_shape=[512, 512], channels=cls.INFERENCE_CHANNELS, **kw)

    @classmethod
    def from_state_dict(cls, sd: dict, spectrogram_shape=None, **kw) -> "QTransformAdapter":
        """Build the variant a checkpoint was saved from (channel widths read off ``freq_adapter.{0,3,6}.weight``;
        the Q-scan resolution is not stored in a ``state_dict``: it defaults to the one the reference pairs with the
        widths -- 128 x 128 for 32/64/128, 512 x 512 for 16/32/64) and load it."""
        ch = tuple(int(sd[f"freq_adapter.{i}.weight"].shape[0]) for i in (0, 3, 6))
        if spectrogram_shape is None:
            spectrogram_shape = [512, 512] if ch == cls.INFERENCE_CHANNELS else [128, 128]
        kw.setdefault("n_detectors", int(sd["film_gamma"].shape[0]))
        m = cls(spectrogram_shape=spectrogram_shape, channels=ch, **kw)
        m.load_state_dict(sd)
        return m

    # ---- the CNN as HIP kernels (csrc/qadapter_cnn.hip), forward AND (round 4) backward: training the adapter
    # (MLGWSC-1/train.py:494-504 trains it through the frozen encoder) goes through _CnnFunction; the torch.nn modules hold
    # the parameters (state_dict names of the reference) and only run for channel widths / map sizes the kernels do not have.
    def _cnn_params(self):
        fa = self.freq_adapter
        return [fa[0].weight, fa[0].bias, fa[3].weight, fa[3].bias, fa[6].weight, fa[6].bias, fa[8].weight, fa[8].bias]

    def _packed_cnn(self):
        ps = self._cnn_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if getattr(self, "_cnn_key", None) != key:
            c1, c2, c3 = (int(ps[i].shape[0]) for i in (0, 2, 4))
            n = lib().gww_qadapter_cnn_packed_bytes(c1, c2, c3)
            if n == 0:
                self._cnn_packed, self._cnn_ch = None, None       # channel widths the kernels are not built for
            else:
                dev = ps[0].device
                blob = torch.empty(n, dtype=torch.uint8, device=dev)
                f = [p.detach().to(torch.float32).contiguous() for p in ps]
                with torch.cuda.device(dev):
                    check(lib().gww_qadapter_cnn_pack_f32(*[t.data_ptr() for t in f], c1, c2, c3, blob.data_ptr(),
                                                          torch.cuda.current_stream().cuda_stream), "gww_qadapter_cnn_pack_f32")
                self._cnn_packed, self._cnn_ch = blob, (c1, c2, c3)
            self._cnn_key = key
        return self._cnn_packed, self._cnn_ch

    def cnn_forward(self, qspec: torch.Tensor) -> torch.Tensor:
        """``self.freq_adapter(qspec[:, None])[:, 0]`` by the HIP kernels: [B, H, W] fp32 -> [B, H/4, W/4] fp32."""
        packed, ch = self._packed_cnn()
        B, H, W = qspec.shape
        if packed is None or H % 32 or W % 128:
            raise _lib.GwwError(f"QTransformAdapter: no HIP CNN for channels {ch} on a {H} x {W} map")
        qspec = qspec.to(torch.float32).contiguous()
        y = torch.empty((B, H // 4, W // 4), dtype=torch.float32, device=qspec.device)
        need = lib().gww_qadapter_cnn_workspace_bytes(B, H, W, ch[0], ch[1])
        ws = getattr(self, "_cnn_ws", None)
        if ws is None or ws.numel() < need or ws.device != qspec.device:
            ws = self._cnn_ws = torch.empty(need, dtype=torch.uint8, device=qspec.device)
        with torch.cuda.device(qspec.device):
            check(lib().gww_qadapter_cnn_forward_f32(qspec.data_ptr(), B, H, W, packed.data_ptr(), *ch, ws.data_ptr(), ws.numel(),
                                                     y.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "gww_qadapter_cnn_forward_f32")
        return y

    def _use_hip_cnn(self, x) -> bool:
        return self._packed_cnn()[0] is not None

    def _cnn_needs_grad(self) -> bool:
        return torch.is_grad_enabled() and any(p.requires_grad for p in self._cnn_params())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, D, _ = x.shape
        F, T = self.target_shape
        if T % 4 != 0:
            raise _lib.GwwError("QTransformAdapter: target_shape[1] must be a multiple of 4")
        out = torch.empty((B, D, F, T), dtype=torch.float32, device=x.device)
        hip_cnn = self._use_hip_cnn(x)
        for i in range(D):
            with torch.no_grad():
                qspec = self.q_transform(x[:, i]).unsqueeze(1)        # [B, 1, F, T]  (plane chosen per call, per detector)
            if hip_cnn and self._cnn_needs_grad() and qspec.shape[-1] <= 512:
                y = _CnnFunction.apply(self, qspec[:, 0], *self._cnn_params())   # HIP forward + HIP backward
            elif hip_cnn and not self._cnn_needs_grad():
                y = self.cnn_forward(qspec[:, 0])                     # three HIP launches, no library call
            else:
                y = self.freq_adapter(qspec).squeeze(1)               # torch.nn (autograd for the adapter's training)
            # final_pool + scale / bias + FiLM and the stack over detectors: one kernel, one 960 KB write per window
            out = _AdapterTail.apply(y, self.scale, self.bias, self.film_gamma, self.film_beta, out, i)
        return out
