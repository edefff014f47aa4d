"""Tensor-level wrappers around the C ABI (device pointers + the current HIP stream).

PyTorch is used here only for device memory and streams.  Every function
requires CUDA(HIP) tensors and calls into libgww.so; none has a torch fallback.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._lib import check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype=None, name="tensor") -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.GwwError(f"{name} must live on the GPU (got {t.device}); gw_whisper_amd has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise _lib.GwwError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


@dataclass(frozen=True)
class FrontendConfig:
    """One configuration of the log-mel front end (``gww_frontend_cfg`` of include/gww.h): HF's
    ``WhisperFeatureExtractor(feature_size, sampling_rate, hop_length, chunk_length, n_fft)`` with
    ``n_samples = chunk_length * sampling_rate``, plus the band of the mel filterbank (HF fixes 0 .. 8000 Hz).  The
    defaults are Whisper's published configuration.  The library checks the supported set; its message names the field."""
    n_mels: int = 80
    sampling_rate: int = 16000
    n_fft: int = 400
    hop_length: int = 160
    n_samples: int = 480000
    min_frequency: float = 0.0
    max_frequency: float = 8000.0

    @property
    def n_frames(self) -> int:
        return self.n_samples // self.hop_length

    @property
    def n_freq(self) -> int:
        return self.n_fft // 2 + 1

    @property
    def is_published(self) -> bool:
        return (self.sampling_rate, self.n_fft, self.hop_length, self.n_samples, float(self.min_frequency),
                float(self.max_frequency)) == (16000, 400, 160, 480000, 0.0, 8000.0)

    def c_struct(self) -> "_lib.FrontendCfg":
        return _lib.FrontendCfg(int(self.n_mels), int(self.sampling_rate), int(self.n_fft), int(self.hop_length),
                                int(self.n_samples), float(self.min_frequency), float(self.max_frequency))


_frontend = {}


def _fe(device, n_mels: int = 80, config: FrontendConfig | None = None, general: bool = False) -> int:
    """The front-end handle of a device: per ``n_mels`` for the published configuration, per configuration otherwise
    (``general``: the published configuration through the general kernels, a handle of its own -- for tests)."""
    idx = torch.device(device).index or 0
    key = (idx, n_mels) if config is None else (idx, config, bool(general))
    if key not in _frontend:
        import ctypes as C
        h = C.c_void_p()
        with torch.cuda.device(idx):
            if config is not None:
                cfg = config.c_struct()
                check(lib().gww_frontend_create_cfg(C.byref(cfg), C.byref(h)), "gww_frontend_create_cfg")
                if general:
                    check(lib().gww_frontend_set_general(h, 1), "gww_frontend_set_general")
            elif n_mels == 80:
                check(lib().gww_frontend_create(C.byref(h)), "gww_frontend_create")
            else:
                check(lib().gww_frontend_create_nmel(n_mels, C.byref(h)), "gww_frontend_create_nmel")
        _frontend[key] = h
    return _frontend[key]


def _check_n_mels(n_mels: int) -> None:
    if n_mels not in (80, 128):
        raise _lib.GwwError(f"n_mels={n_mels}: the Whisper front end has 80 or 128 (large-v3) mel bins")


def logmel(wave: torch.Tensor, n_samples: int | None = None, n_mels: int = 80, config: FrontendConfig | None = None,
           general: bool = False) -> torch.Tensor:
    """[n, L] fp32 GPU waveform -> [n, n_mels, n_frames] fp32 ``input_features`` (16 kHz and [n, n_mels, 3000] without
    ``config``).

    Same arithmetic as ``WhisperFeatureExtractor(feature_size=n_mels)(...)`` (reference call site
    Signal_vs_Noise/src/dataset.py:20-21): zero-pad/truncate to 30 s, STFT, mel, log10,
    per-segment dynamic-range clamp, affine.  ``n_mels`` is 80, or 128 for whisper-large-v3.
    ``config`` (its ``n_mels`` then counts) selects any supported configuration: the published one runs the same kernels
    as no ``config`` at all, every other one the general kernels of csrc/logmel_any.hip.
    """
    if config is not None:
        n_mels = config.n_mels
    _check_n_mels(n_mels)
    if wave.dim() == 1:
        wave = wave[None]
    wave = _dev(wave, torch.float32, "wave")
    n, L = wave.shape
    n_samples = L if n_samples is None else n_samples
    fe = _fe(wave.device, n_mels, config, general)
    frames = 3000 if config is None else config.n_frames
    out = torch.empty((n, n_mels, frames), dtype=torch.float32, device=wave.device)
    seg_max = torch.empty((max(n, 1),), dtype=torch.float32, device=wave.device)
    with torch.cuda.device(wave.device):
        step = 32768   # gridDim.y limit
        for i in range(0, n, step):
            m = min(step, n - i)
            check(lib().gww_logmel_f32(fe, wave[i:].data_ptr(), m, n_samples, wave.stride(0),
                                       out[i:].data_ptr(), seg_max[i:].data_ptr(), _stream()), "gww_logmel_f32")
    return out


_WINDOW_ROUTES = {_lib.WINDOWS_PER_WINDOW: "per_window", _lib.WINDOWS_SHARED: "shared"}
_last_windows_route = None


def logmel_windows_plan(config: FrontendConfig, step: int, n_windows: int) -> dict:
    """What ``logmel_windows`` does for ``n_windows`` windows of ``config.n_samples`` samples every ``step`` (include/gww.h:
    ``gww_windows_plan``): ``route`` ("shared" or "per_window"), ``edge_lo`` / ``edge_hi`` / ``interior`` frames per window,
    ``stream_frames``, ``dft_frames_shared`` / ``dft_frames_per_window`` and ``workspace_bytes``, the last four per row.
    Plain C++, needs no GPU; ``step < 1`` and ``n_windows < 1`` raise ``GwwError`` naming the argument."""
    import ctypes as C
    cfg, plan = config.c_struct(), _lib.WindowsPlan()
    check(lib().gww_logmel_windows_plan(C.byref(cfg), int(step), int(n_windows), C.byref(plan)), "gww_logmel_windows_plan")
    out = {name: int(getattr(plan, name)) for name, _ in _lib.WindowsPlan._fields_}
    out["route"] = _WINDOW_ROUTES[plan.route]
    return out


def last_logmel_windows_route():
    """"shared" or "per_window": the route the last ``logmel_windows`` call ran (None before the first)."""
    return _last_windows_route


def logmel_windows(series: torch.Tensor, config: FrontendConfig, step: int, w0: int = 0, n_windows: int | None = None,
                   rows_major: bool = False, route: str | None = None) -> torch.Tensor:
    """[R, N] fp32 GPU series (any row stride) -> [n, R, n_mels, n_frames] (``rows_major``: [R, n, ...]) fp32: the
    features of windows ``w0 .. w0 + n - 1``, window ``w`` being samples ``[w step, w step + config.n_samples)`` of every
    row -- bit for bit ``logmel(window, config=config)`` of the materialised window (for Whisper's published configuration:
    ``general=True``, the general kernels), without materialising it.
    ``n_windows=None``: every window from ``w0`` on that fits.  Where ``step`` is a multiple of the hop and windows overlap,
    an STFT frame several windows hold is computed once per call (csrc/logmel_windows.hip, ``logmel_windows_plan``);
    ``route="per_window"`` forces the general kernels on every window, ``route="shared"`` raises where the plan refuses."""
    global _last_windows_route
    if route not in (None, "shared", "per_window"):
        raise _lib.GwwError(f"logmel_windows: route={route!r} (None, 'shared' or 'per_window')")
    if series.dim() == 1:
        series = series[None]
    if series.dim() != 2:
        raise _lib.GwwError(f"logmel_windows: series {tuple(series.shape)} is not [rows, samples]")
    R, N = series.shape
    step, w0, L = int(step), int(w0), int(config.n_samples)
    if step < 1:
        raise _lib.GwwError(f"logmel_windows: step={step} must be at least 1")
    if w0 < 0:
        raise _lib.GwwError(f"logmel_windows: w0={w0} must not be negative")
    fit = 0 if N < w0 * step + L else (N - L - w0 * step) // step + 1
    n = fit if n_windows is None else int(n_windows)
    if n < 1 or n > fit:
        raise _lib.GwwError(f"logmel_windows: n_windows={n}: a series of {N} samples holds {fit} window(s) of {L} every {step} "
                            f"from w0={w0} on")
    if R < 1:
        raise _lib.GwwError("logmel_windows: series has no rows")
    plan = logmel_windows_plan(config, step, n)
    if route == "shared" and plan["route"] != "shared":
        raise _lib.GwwError(f"logmel_windows: route='shared' is refused for step={step}, n_windows={n} (hop_length "
                            f"{config.hop_length}: {plan['dft_frames_shared']} shared against {plan['dft_frames_per_window']} "
                            f"per-window frames)")
    if not series.is_cuda:
        raise _lib.GwwError(f"series must live on the GPU (got {series.device}); gw_whisper_amd has no CPU path")
    if series.dtype != torch.float32:
        raise _lib.GwwError(f"series must be torch.float32, got {series.dtype}")
    if series.stride(1) != 1 or (R > 1 and series.stride(0) < 1):
        series = series.contiguous()
    per_window = route == "per_window" or plan["route"] == "per_window"
    ws_bytes = R * ((4 * n + 15) // 16 * 16 if per_window else plan["workspace_bytes"])
    shape = (R, n) if rows_major else (n, R)
    out = torch.empty((*shape, config.n_mels, config.n_frames), dtype=torch.float32, device=series.device)
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=series.device)
    fe = _fe(series.device, config.n_mels, config, general=config.is_published)
    with torch.cuda.device(series.device):
        check(lib().gww_logmel_windows_f32(fe, series.data_ptr(), R, N, series.stride(0) if R > 1 else N, step, w0, n,
                                           out.data_ptr(), int(rows_major), ws.data_ptr(), ws_bytes,
                                           _lib.WINDOWS_PER_WINDOW if route == "per_window" else -1, _stream()),
              "gww_logmel_windows_f32")
    _last_windows_route = "per_window" if per_window else "shared"
    return out


def logmel_host(wave, n_samples: int | None = None, n_mels: int = 80, config: FrontendConfig | None = None) -> torch.Tensor:
    """CPU twin of :func:`logmel`: [n, L] fp32 host waveform -> [n, n_mels, n_frames] fp32 CPU tensor.

    Runs ``gww_logmel_host_nmel_f32`` (``gww_logmel_host_cfg_f32`` with a ``config``; plain C++ inside libgww.so, no HIP
    call), so it works inside forked DataLoader
    workers, where the reference calls the extractor (Signal_vs_Noise/src/dataset.py:20-21 under
    src/train.py:224-225).  Not a fallback of the GPU path: callers pick it by handing over host data.
    """
    import numpy as np
    if config is not None:
        n_mels = config.n_mels
    _check_n_mels(n_mels)
    w = np.ascontiguousarray(wave.numpy() if isinstance(wave, torch.Tensor) else wave, dtype=np.float32)
    if w.ndim == 1:
        w = w[None]
    n, L = w.shape
    n_samples = L if n_samples is None else n_samples
    if config is not None:
        import ctypes as C
        frontend_validate(config)   # (before anything is allocated: an unsupported n_frames must not size the output)
        cfg = config.c_struct()
        out = torch.empty((n, n_mels, config.n_frames), dtype=torch.float32)
        check(lib().gww_logmel_host_cfg_f32(C.byref(cfg), w.ctypes.data, n, n_samples, max(L, 1) if n else 1,
                                            out.data_ptr()), "gww_logmel_host_cfg_f32")
        return out
    out = torch.empty((n, n_mels, 3000), dtype=torch.float32)
    check(lib().gww_logmel_host_nmel_f32(w.ctypes.data, n, n_samples, max(L, 1) if n else 1, n_mels, out.data_ptr()),
          "gww_logmel_host_nmel_f32")
    return out


def frontend_validate(config: FrontendConfig) -> None:
    """Raise ``GwwError`` (naming the field) unless the library supports ``config``; needs no GPU."""
    import ctypes as C
    cfg = config.c_struct()
    check(lib().gww_frontend_validate_cfg(C.byref(cfg)), "gww_frontend_validate_cfg")


def mel_filters(config: FrontendConfig, device=None):
    """float32 [n_mels, n_fft / 2 + 1]: the filterbank of ``config`` (numpy): the host twin's, or with a CUDA ``device`` the one
    that device's handle holds."""
    import ctypes as C
    import numpy as np
    frontend_validate(config)
    out = np.empty((config.n_mels, config.n_freq), np.float32)
    if device is None or torch.device(device).type == "cpu":
        cfg = config.c_struct()
        check(lib().gww_frontend_mel_filters_host_f32(C.byref(cfg), out.ctypes.data), "gww_frontend_mel_filters_host_f32")
    else:
        check(lib().gww_frontend_mel_filters_f32(_fe(device, config.n_mels, config), out.ctypes.data),
              "gww_frontend_mel_filters_f32")
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out_bf16: bool = False) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    M, d = x.shape
    y = torch.empty((M, d), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_layernorm(x.data_ptr(), _dev(w, torch.float32).data_ptr(), _dev(b, torch.float32).data_ptr(),
                                  y.data_ptr(), int(out_bf16), M, d, _stream()), "gww_layernorm")
    return y


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, torch.float32, "x")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_cast_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gww_cast_f32_bf16")
    return y


def gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, epilogue: int = 0,
         resid: torch.Tensor | None = None) -> torch.Tensor:
    """C = A[M,K] @ W[N,K]^T + bias with epilogue 0 none / 1 GELU / 2 += resid.

    bf16 A/W -> bf16 C (fp32 C for the residual epilogue); fp32 A/W -> fp32 C.
    """
    bf = a.dtype == torch.bfloat16
    a = _dev(a, torch.bfloat16 if bf else torch.float32, "A")
    w = _dev(w, a.dtype, "W")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise _lib.GwwError(f"gemm: A is [{M},{K}] but W is {tuple(w.shape)}")
    out_dtype = torch.float32 if (not bf or epilogue == _lib.EPI_RESID) else torch.bfloat16
    c = torch.empty((M, N), dtype=out_dtype, device=a.device)
    bptr = _dev(bias, torch.float32, "bias").data_ptr() if bias is not None else None
    rptr = _dev(resid, torch.float32, "resid").data_ptr() if resid is not None else None
    fn = lib().gww_gemm_bf16 if bf else lib().gww_gemm_f32
    with torch.cuda.device(a.device):
        check(fn(a.data_ptr(), w.data_ptr(), bptr, rptr, c.data_ptr(), M, N, K, epilogue, _stream()), "gww_gemm")
    return c


def gemm_v4_split(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, epilogue: int = 0,
                  resid: torch.Tensor | None = None, n_split: int = 0) -> torch.Tensor:
    """``gemm`` on the 256 x 256 x 64 kernel of the wide encoders with an explicit column split of its work items
    (``gww_gemm_bf16_v4_split``; 0 = the automatic choice).  bf16 A [M % 256 == 0, K] / W [N, K]."""
    a = _dev(a, torch.bfloat16, "A")
    w = _dev(w, torch.bfloat16, "W")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise _lib.GwwError(f"gemm_v4_split: A is [{M},{K}] but W is {tuple(w.shape)}")
    c = torch.empty((M, N), dtype=torch.float32 if epilogue == _lib.EPI_RESID else torch.bfloat16, device=a.device)
    bptr = _dev(bias, torch.float32, "bias").data_ptr() if bias is not None else None
    rptr = _dev(resid, torch.float32, "resid").data_ptr() if resid is not None else None
    with torch.cuda.device(a.device):
        check(lib().gww_gemm_bf16_v4_split(a.data_ptr(), w.data_ptr(), bptr, rptr, c.data_ptr(), M, N, K, epilogue,
                                           int(n_split), _stream()), "gww_gemm_bf16_v4_split")
    return c


def ln_fold_weights(w: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, bias=None, scale: float = 1.0):
    """Fold LayerNorm(gain ln_w, shift ln_b) into the Linear (w fp32 [N,K], bias) that follows it.
    Returns (w_folded bf16 [N,K], u fp32 [N], cb fp32 [N]) for ``gemm_astat(..., ln=(u, cb))``."""
    w = _dev(w, torch.float32, "w")
    N, K = w.shape
    wf = torch.empty((N, K), dtype=torch.bfloat16, device=w.device)
    u = torch.empty((N,), dtype=torch.float32, device=w.device)
    cb = torch.empty((N,), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        check(lib().gww_ln_fold_weights(w.data_ptr(), _dev(ln_w, torch.float32).data_ptr(),
                                        _dev(ln_b, torch.float32).data_ptr(),
                                        _dev(bias, torch.float32).data_ptr() if bias is not None else None,
                                        float(scale), N, K, wf.data_ptr(), u.data_ptr(), cb.data_ptr(), _stream()),
              "gww_ln_fold_weights")
    return wf, u, cb


def gemm_astat(a: torch.Tensor, w: torch.Tensor, bias=None, epilogue: int = 0, ln=None, delta=None,
               return_x: bool = False, out=None):
    """A-stationary bf16 GEMM (K in {256,384,512}) -> bf16 [M, N].

    ``ln=(u, cb)`` (from ``ln_fold_weights``, with ``w`` the folded panel): ``a`` is the fp32
    residual stream, ``x_new = a + delta`` (bf16 ``delta`` optional) and LayerNorm are fused
    into the GEMM in one pass; ``return_x`` also returns ``x_new``.  Output rows are padded
    to a multiple of 256 internally, or ``out`` (bf16, contiguous, >= roundup(M, 256) rows) is
    written.  ``epilogue=EPI_DGELU``: C = delta * gelu'(a w^T + bias) with ``delta`` the incoming
    bf16 [M, N] gradient; ``out`` may be ``delta`` itself (the encoder's in-place form)."""
    fused = ln is not None
    dgelu = epilogue == _lib.EPI_DGELU
    a = _dev(a, torch.float32 if fused else torch.bfloat16, "A")
    w = _dev(w, torch.bfloat16, "W")
    M, K = a.shape
    N = w.shape[0]
    Mp = (M + 255) // 256 * 256
    if out is None:
        c = torch.empty((Mp, N), dtype=torch.bfloat16, device=a.device)
    else:
        c = out
        if c.dtype != torch.bfloat16 or not c.is_cuda or not c.is_contiguous() or c.dim() != 2 or c.shape[0] < Mp \
                or c.shape[1] != N:
            raise _lib.GwwError(f"gemm_astat: out must be a contiguous bf16 GPU tensor of [>= {Mp}, {N}]")
    if dgelu and (delta is None or tuple(delta.shape[1:]) != (N,) or delta.shape[0] < M or not delta.is_contiguous()):
        raise _lib.GwwError(f"gemm_astat: the gelu-backward epilogue needs a contiguous delta of [>= {M}, {N}]")
    dl = _dev(delta, torch.bfloat16, "delta") if delta is not None else None
    # x_new is only materialised when there is a delta to add; otherwise x_new IS a
    x_out = torch.empty_like(a) if (fused and return_x and dl is not None) else None
    with torch.cuda.device(a.device):
        check(lib().gww_gemm_astat_bf16(
            a.data_ptr(), dl.data_ptr() if (dl is not None and (x_out is not None or dgelu)) else None,
            x_out.data_ptr() if x_out is not None else None,
            _dev(ln[0], torch.float32).data_ptr() if fused else None,
            _dev(ln[1], torch.float32).data_ptr() if fused else None, w.data_ptr(),
            _dev(bias, torch.float32).data_ptr() if bias is not None else None, c.data_ptr(), M, N, K,
            epilogue, _stream()), "gww_gemm_astat_bf16")
    return (c[:M], x_out if x_out is not None else a) if return_x else c[:M]


def gemm_fulln(a: torch.Tensor, w: torch.Tensor, bias=None, epilogue: int = 0) -> torch.Tensor:
    """Full-N bf16 GEMM (N in {384, 512}, K % 32 == 0): complete output rows per workgroup."""
    a = _dev(a, torch.bfloat16, "A")
    w = _dev(w, torch.bfloat16, "W")
    M, K = a.shape
    N = w.shape[0]
    Mp = (M + 127) // 128 * 128
    c = torch.empty((Mp, N), dtype=torch.bfloat16, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().gww_gemm_fulln_bf16(a.data_ptr(), w.data_ptr(),
                                        _dev(bias, torch.float32).data_ptr() if bias is not None else None,
                                        c.data_ptr(), M, N, K, epilogue, _stream()), "gww_gemm_fulln_bf16")
    return c[:M]


def mlp_pack(w1_folded: torch.Tensor, w2: torch.Tensor, wqkv_folded: torch.Tensor | None = None) -> torch.Tensor:
    """Weight stream of mlp_fused: folded fc1 panel [F, 384] + fc2 panel [384, F] (+ the next layer's folded
    q / k / v panel [NQ, 384]) -> bf16 [2 * 384 * F (+ NQ * 384)]."""
    wq = _dev(wqkv_folded, torch.bfloat16, "Wqkv") if wqkv_folded is not None else None
    if w1_folded is None:            # only the q / k / v panel: the stream of lnqkv_fused
        if wq is None:
            raise _lib.GwwError("mlp_pack: nothing to pack")
        w1 = w2 = None
        F, d = 0, wq.shape[1]
    else:
        w1 = _dev(w1_folded, torch.bfloat16, "W1")
        w2 = _dev(w2, torch.bfloat16, "W2")
        F, d = w1.shape
    NQ = wq.shape[0] if wq is not None else 0
    dev = wq.device if w1 is None else w1.device
    out = torch.empty((2 * d * F + NQ * d,), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_mlp_pack_bf16(w1.data_ptr() if w1 is not None else None, w2.data_ptr() if w2 is not None else None,
                                      wq.data_ptr() if wq is not None else None, out.data_ptr(), d, F, NQ, _stream()),
              "gww_mlp_pack_bf16")
    return out


def attn_out_mlp_fused(x, ctx, wo, bo, w1_folded, w2, ln_u, ln_cb, b2, qkv=None):
    """The attention output projection fused in front of ``mlp_fused``: x_new = x + bf16(ctx Wo^T + bo), then the block.
    ``qkv=(wqkv_folded, u, cb)`` appends the next layer's LN1 + q / k / v.  Returns (C or qkv, x_new or x_next)."""
    x = _dev(x, torch.float32, "x")
    ctx = _dev(ctx, torch.bfloat16, "ctx")
    wo = _dev(wo, torch.bfloat16, "Wo")
    w1 = _dev(w1_folded, torch.bfloat16, "W1")
    w2 = _dev(w2, torch.bfloat16, "W2")
    wq = _dev(qkv[0], torch.bfloat16, "Wqkv") if qkv is not None else None
    F, d = w1.shape
    NQ = wq.shape[0] if wq is not None else 0
    M = x.shape[0]
    Mp = (M + 127) // 128 * 128
    f = lambda t: _dev(t, torch.float32)
    bo, u, cb, b2 = f(bo), f(ln_u), f(ln_cb), f(b2)
    wt = torch.empty((d * d + 2 * d * F + NQ * d,), dtype=torch.bfloat16, device=x.device)
    if qkv is not None:
        x = x.clone()      # the library writes x_next back over x (include/gww.h): the caller's tensor stays untouched
    x_out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().gww_mlp_pack_op_bf16(wo.data_ptr(), w1.data_ptr(), w2.data_ptr(), wq.data_ptr() if wq is not None else None,
                                         wt.data_ptr(), d, F, NQ, _stream()), "gww_mlp_pack_op_bf16")
        if qkv is None:
            out = torch.empty((Mp, d), dtype=torch.bfloat16, device=x.device)
            qu = qc = None
        else:
            qu, qc = f(qkv[1]), f(qkv[2])
            out = torch.empty((Mp, NQ), dtype=torch.bfloat16, device=x.device)
        check(lib().gww_attn_out_mlp_fused_bf16(x.data_ptr(), ctx.data_ptr(), bo.data_ptr(), x_out.data_ptr(), u.data_ptr(),
                                                cb.data_ptr(), wt.data_ptr(), b2.data_ptr(),
                                                out.data_ptr() if qkv is None else None, M, d, F,
                                                qu.data_ptr() if qu is not None else None,
                                                qc.data_ptr() if qc is not None else None,
                                                out.data_ptr() if qkv is not None else None, NQ, _stream()),
              "gww_attn_out_mlp_fused_bf16")
    return out[:M], (x_out if qkv is None else x)


def attn_out_mlp_final(x, ctx, wo, bo, w1_folded, w2, ln_u, ln_cb, b2, lnf_w, lnf_b):
    """The LAST block with the encoder's final LayerNorm as its epilogue (``gww_attn_out_mlp_final_bf16``): returns
    (y fp32 [M, 384] = LayerNorm_final(x_mid + bf16(mlp(LayerNorm2(x_mid)) + b2)), x_mid = x + bf16(ctx Wo^T + bo))."""
    x = _dev(x, torch.float32, "x")
    ctx = _dev(ctx, torch.bfloat16, "ctx")
    wo, w1, w2 = _dev(wo, torch.bfloat16, "Wo"), _dev(w1_folded, torch.bfloat16, "W1"), _dev(w2, torch.bfloat16, "W2")
    F, d = w1.shape
    M = x.shape[0]
    f = lambda t: _dev(t, torch.float32)
    bo, u, cb, b2, lw, lb = f(bo), f(ln_u), f(ln_cb), f(b2), f(lnf_w), f(lnf_b)
    wt = torch.empty((d * d + 2 * d * F,), dtype=torch.bfloat16, device=x.device)
    x_mid, y = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().gww_mlp_pack_op_bf16(wo.data_ptr(), w1.data_ptr(), w2.data_ptr(), None, wt.data_ptr(), d, F, 0, _stream()),
              "gww_mlp_pack_op_bf16")
        check(lib().gww_attn_out_mlp_final_bf16(x.data_ptr(), ctx.data_ptr(), bo.data_ptr(), x_mid.data_ptr(), u.data_ptr(),
                                                cb.data_ptr(), wt.data_ptr(), b2.data_ptr(), lw.data_ptr(), lb.data_ptr(),
                                                y.data_ptr(), M, d, F, _stream()), "gww_attn_out_mlp_final_bf16")
    return y, x_mid


def lnqkv_fused(x, wt, qkv_u, qkv_cb):
    """qkv bf16 [M, NQ] = LayerNorm(x) Wqkv'^T + cb for a residual stream without a pending delta (layer 0): the panel
    prologue and the q / k / v tail of the fused MLP kernel; ``wt = mlp_pack(None, None, wqkv_folded)``."""
    x = _dev(x, torch.float32, "x")
    wt = _dev(wt, torch.bfloat16, "Wt")
    M, d = x.shape
    qu, qc = _dev(qkv_u, torch.float32), _dev(qkv_cb, torch.float32)
    NQ = qu.numel()
    qo = torch.empty(((M + 127) // 128 * 128, NQ), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_lnqkv_fused_bf16(x.data_ptr(), qu.data_ptr(), qc.data_ptr(), wt.data_ptr(), qo.data_ptr(), M, d, NQ,
                                         _stream()), "gww_lnqkv_fused_bf16")
    return qo[:M]


def _x0_operands(xs, tr, pos, flag, x=None):
    """The compact stem's description of layer 0's residual stream: xs fp32 [B, Tt, 384], tr fp32 [B, 384], pos fp32 [T, 384],
    flag int32 [1] (on the device), x fp32 [B * T, 384] or None (allocated uninitialised: unread where flag == 1)."""
    xs, tr, pos = _dev(xs, torch.float32, "xs"), _dev(tr, torch.float32, "tr"), _dev(pos, torch.float32, "pos")
    if flag.dtype != torch.int32 or not flag.is_cuda or flag.numel() != 1:
        raise _lib.GwwError("flag must be one int32 on the device")
    B, Tt, d = xs.shape
    T = pos.shape[0]
    if tr.shape != (B, d) or pos.shape[1] != d:
        raise _lib.GwwError("tr must be [B, d] and pos [T, d]")
    if x is None:
        x = torch.empty((B * T, d), dtype=torch.float32, device=xs.device)
    else:
        x = _dev(x, torch.float32, "x")
        if x.numel() != B * T * d:
            raise _lib.GwwError("x must hold B * T rows")
    return xs, tr, pos, flag, x, B, T, Tt, d


def stem_fill(xs, tr, pos, flag, x=None):
    """x fp32 [B * T, d]: the residual stream behind the compact conv stem written out (``gww_stem_fill_f32``):
    x[b, j] = xs[b, j] (j <= Tt - 3), fma(xs[b, Tt - 2], tr[b], pos[j]) (Tt - 2 <= j <= T - 2), xs[b, Tt - 1] (j = T - 1).
    Leaves ``x`` as it is where the device flag is 0."""
    xs, tr, pos, flag, x, B, T, Tt, d = _x0_operands(xs, tr, pos, flag, x)
    with torch.cuda.device(xs.device):
        check(lib().gww_stem_fill_f32(xs.data_ptr(), tr.data_ptr(), pos.data_ptr(), flag.data_ptr(), x.data_ptr(), B, T, Tt, d,
                                      _stream()), "gww_stem_fill_f32")
    return x


def lnqkv_fused_x0(xs, tr, pos, flag, wt, qkv_u, qkv_cb, x=None):
    """``lnqkv_fused`` on the stream ``stem_fill`` would write, formed in registers instead (flag 1: ``x`` is not read;
    flag 0: the kernel reads ``x``).  Bitwise ``lnqkv_fused(stem_fill(...))``."""
    xs, tr, pos, flag, x, B, T, Tt, d = _x0_operands(xs, tr, pos, flag, x)
    wt = _dev(wt, torch.bfloat16, "Wt")
    qu, qc = _dev(qkv_u, torch.float32), _dev(qkv_cb, torch.float32)
    NQ, M = qu.numel(), B * T
    qo = torch.empty(((M + 127) // 128 * 128, NQ), dtype=torch.bfloat16, device=xs.device)
    with torch.cuda.device(xs.device):
        check(lib().gww_lnqkv_fused_x0_bf16(xs.data_ptr(), tr.data_ptr(), pos.data_ptr(), flag.data_ptr(), x.data_ptr(), T, Tt,
                                            qu.data_ptr(), qc.data_ptr(), wt.data_ptr(), qo.data_ptr(), M, d, NQ, _stream()),
              "gww_lnqkv_fused_x0_bf16")
    return qo[:M]


def attn_out_mlp_fused_x0(xs, tr, pos, flag, ctx, wo, bo, w1_folded, w2, ln_u, ln_cb, b2, qkv, x=None):
    """``attn_out_mlp_fused`` with the q / k / v tail on the stream ``stem_fill`` would write, formed in the kernel's accumulators
    (flag 1: ``x`` is not read; flag 0: the kernel reads ``x``).  Returns (qkv, x_next); the caller's ``x`` stays untouched."""
    xs, tr, pos, flag, x, B, T, Tt, d = _x0_operands(xs, tr, pos, flag, x)
    x = x.clone().view(B * T, d)   # x_next is written over x
    ctx = _dev(ctx, torch.bfloat16, "ctx")
    wo, w1, w2 = _dev(wo, torch.bfloat16, "Wo"), _dev(w1_folded, torch.bfloat16, "W1"), _dev(w2, torch.bfloat16, "W2")
    wq = _dev(qkv[0], torch.bfloat16, "Wqkv")
    F, NQ, M = w1.shape[0], wq.shape[0], B * T
    f = lambda t: _dev(t, torch.float32)
    bo, u, cb, b2, qu, qc = f(bo), f(ln_u), f(ln_cb), f(b2), f(qkv[1]), f(qkv[2])
    wt = torch.empty((d * d + 2 * d * F + NQ * d,), dtype=torch.bfloat16, device=x.device)
    out = torch.empty(((M + 127) // 128 * 128, NQ), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_mlp_pack_op_bf16(wo.data_ptr(), w1.data_ptr(), w2.data_ptr(), wq.data_ptr(), wt.data_ptr(), d, F, NQ,
                                         _stream()), "gww_mlp_pack_op_bf16")
        check(lib().gww_attn_out_mlp_fused_x0_bf16(xs.data_ptr(), tr.data_ptr(), pos.data_ptr(), flag.data_ptr(), x.data_ptr(), T, Tt,
                                                   ctx.data_ptr(), bo.data_ptr(), u.data_ptr(), cb.data_ptr(), wt.data_ptr(),
                                                   b2.data_ptr(), M, d, F, qu.data_ptr(), qc.data_ptr(), out.data_ptr(), NQ,
                                                   _stream()), "gww_attn_out_mlp_fused_x0_bf16")
    return out[:M], x


def mlp_fused(x, delta, wt, ln_u, ln_cb, b2, qkv=None):
    """(C bf16 [M, 384], x_new fp32 [M, 384]) = fused LayerNorm -> fc1 -> GELU -> fc2 of x + delta.
    ``qkv=(u, cb)`` of the next layer's folded q / k / v projection (panel appended to ``wt``): returns
    (qkv bf16 [M, NQ], x_next fp32 [M, 384]) instead, x_next = x + delta + bf16(mlp output)."""
    x = _dev(x, torch.float32, "x")
    delta = _dev(delta, torch.bfloat16, "delta")
    wt = _dev(wt, torch.bfloat16, "Wt")
    M, d = x.shape
    F = ln_u.numel()
    Mp = (M + 127) // 128 * 128
    if qkv is not None:
        x = x.clone()      # the library writes x_next back over x (include/gww.h): the caller's tensor stays untouched
    x_out = torch.empty_like(x)
    f = lambda t: _dev(t, torch.float32)
    u, cb, b2 = f(ln_u), f(ln_cb), f(b2)
    if qkv is None:
        c = torch.empty((Mp, d), dtype=torch.bfloat16, device=x.device)
        qu = qc = qo = None
        NQ = 0
    else:
        qu, qc = f(qkv[0]), f(qkv[1])
        NQ = qu.numel()
        qo = torch.empty((Mp, NQ), dtype=torch.bfloat16, device=x.device)
        c = None
    with torch.cuda.device(x.device):
        check(lib().gww_mlp_fused_bf16(x.data_ptr(), delta.data_ptr(), x_out.data_ptr(), u.data_ptr(), cb.data_ptr(),
                                       wt.data_ptr(), b2.data_ptr(), c.data_ptr() if c is not None else None, M, d, F,
                                       qu.data_ptr() if qu is not None else None,
                                       qc.data_ptr() if qc is not None else None,
                                       qo.data_ptr() if qo is not None else None, NQ, _stream()),
              "gww_mlp_fused_bf16")
    return ((c if qkv is None else qo)[:M], x_out if qkv is None else x)


def attention(qkv: torch.Tensor, n_heads: int) -> torch.Tensor:
    """qkv [B, T, 3 d] (q pre-scaled) -> ctx [B, T, d]; bf16 or fp32."""
    bf = qkv.dtype == torch.bfloat16
    qkv = _dev(qkv, torch.bfloat16 if bf else torch.float32, "qkv")
    B, T, d3 = qkv.shape
    d = d3 // 3
    if d != n_heads * 64:
        raise _lib.GwwError(f"attention: d={d} != n_heads*64")
    ctx = torch.empty((B, T, d), dtype=qkv.dtype, device=qkv.device)
    fn = lib().gww_attention_bf16 if bf else lib().gww_attention_f32
    with torch.cuda.device(qkv.device):
        check(fn(qkv.data_ptr(), ctx.data_ptr(), B, T, n_heads, _stream()), "gww_attention")
    return ctx


def attention_log2q(qkv: torch.Tensor, n_heads: int, want_lse: bool = False):
    """The attention kernel of the encoder's bf16 paths: like :func:`attention`, but the q section is in log2 units
    (projected with log2(e) / 8 instead of 1 / 8).  Returns ctx, or (ctx, lse [B, H, T] natural log)."""
    qkv = _dev(qkv, torch.bfloat16, "qkv")
    B, T, d3 = qkv.shape
    if d3 != 3 * n_heads * 64:
        raise _lib.GwwError(f"attention: d={d3 // 3} != n_heads*64")
    ctx = torch.empty((B, T, d3 // 3), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, n_heads, T), dtype=torch.float32, device=qkv.device) if want_lse else None
    with torch.cuda.device(qkv.device):
        check(lib().gww_attention_log2q_bf16(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr() if want_lse else None, B, T,
                                             n_heads, _stream()), "gww_attention_log2q_bf16")
    return (ctx, lse) if want_lse else ctx


def attention_probs(qkv: torch.Tensor, n_heads: int, q_log2: bool = False) -> torch.Tensor:
    """qkv [B, T, 3 d] (q pre-scaled; in log2 units when q_log2, bf16 only) -> the softmax maps P [B, H, T, T], fp32:
    the ``output_attentions`` kernel on its own.  T must be a multiple of 4."""
    bf = qkv.dtype == torch.bfloat16
    qkv = _dev(qkv, torch.bfloat16 if bf else torch.float32, "qkv")
    B, T, d3 = qkv.shape
    if d3 != 3 * n_heads * 64:
        raise _lib.GwwError(f"attention_probs: d={d3 // 3} != n_heads*64")
    probs = torch.empty((B, n_heads, T, T), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        if bf:
            check(lib().gww_attention_probs_bf16(qkv.data_ptr(), int(bool(q_log2)), probs.data_ptr(), B, T, n_heads,
                                                 _stream()), "gww_attention_probs_bf16")
        elif q_log2:
            raise _lib.GwwError("attention_probs: q in log2 units is a bf16-path convention")
        else:
            check(lib().gww_attention_probs_f32(qkv.data_ptr(), probs.data_ptr(), B, T, n_heads, _stream()),
                  "gww_attention_probs_f32")
    return probs


def dora_merge(w0: torch.Tensor, a: torch.Tensor, b: torch.Tensor, m: torch.Tensor, scaling: float,
               return_norm: bool = False):
    """W_eff = (m / ||W0 + s B A||_row) * (W0 + s B A)  (peft 0.12.0 dora.py), fp32."""
    w0 = _dev(w0, torch.float32, "w0")
    d_out, d_in = w0.shape
    r = a.shape[0]
    out = torch.empty_like(w0)
    nrm = torch.empty((d_out,), dtype=torch.float32, device=w0.device)
    with torch.cuda.device(w0.device):
        check(lib().gww_dora_merge_f32(w0.data_ptr(), _dev(a, torch.float32).data_ptr(),
                                       _dev(b, torch.float32).data_ptr(), _dev(m, torch.float32).data_ptr(),
                                       float(scaling), d_out, d_in, r, out.data_ptr(), nrm.data_ptr(), _stream()),
              "gww_dora_merge_f32")
    return (out, nrm) if return_norm else out


def conv1_gelu(mel: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``gelu(conv1(input_features))`` of the Whisper stem (HF:modeling_whisper.py:619-620) read straight from the
    ``[B, 80, T]`` feature layout -> token-major bf16 ``[B, T + 2, d]`` with zero rows 0 and T + 1 (conv2's padding)."""
    mel = _dev(mel, torch.float32, "mel")
    weight, bias = _dev(weight, torch.float32, "weight"), _dev(bias, torch.float32, "bias")
    B, C_, T = mel.shape
    d = weight.shape[0]
    if C_ != 80 or tuple(weight.shape) != (d, 80, 3) or tuple(bias.shape) != (d,):
        raise _lib.GwwError(f"conv1_gelu: mel {tuple(mel.shape)}, weight {tuple(weight.shape)}, bias {tuple(bias.shape)}")
    scratch = torch.empty((d, 256), dtype=torch.bfloat16, device=mel.device)
    out = torch.empty((B, T + 2, d), dtype=torch.bfloat16, device=mel.device)
    with torch.cuda.device(mel.device):
        check(lib().gww_conv1_gelu_bf16(mel.data_ptr(), weight.data_ptr(), bias.data_ptr(), scratch.data_ptr(), out.data_ptr(),
                                        B, T, d, _stream()), "gww_conv1_gelu_bf16")
    return out


def dora_merge_batch(items, return_norm: bool = True):
    """``dora_merge`` for a list of ``(w0, a, b, m, scaling)`` tuples in ONE launch (an optimizer step changes every
    adapted projection at once; a launch per 384 x 384 matrix is launch-bound).  Returns a list of ``(w_eff, norm)``."""
    if not items:
        return []
    dev = items[0][0].device
    arr = (_lib.DoraMergeItem * len(items))()
    out, keep = [], []
    for i, (w0, a, b, m, scaling) in enumerate(items):
        w0, a, b, m = (_dev(t, torch.float32) for t in (w0, a, b, m))
        d_out, d_in = w0.shape
        r = a.shape[0]
        if a.shape != (r, d_in) or b.shape != (d_out, r) or m.shape != (d_out,) or w0.device != dev:
            raise _lib.GwwError(f"dora_merge_batch: item {i}: shapes {tuple(w0.shape)} {tuple(a.shape)} {tuple(b.shape)} "
                                f"{tuple(m.shape)} or device do not fit")
        w = torch.empty_like(w0)
        nrm = torch.empty((d_out,), dtype=torch.float32, device=dev)
        keep += [w0, a, b, m]
        arr[i] = _lib.DoraMergeItem(w0.data_ptr(), a.data_ptr(), b.data_ptr(), m.data_ptr(), w.data_ptr(), nrm.data_ptr(),
                                    float(scaling), d_out, d_in, r)
        out.append((w, nrm))
    with torch.cuda.device(dev):
        check(lib().gww_dora_merge_batch_f32(arr, len(items), _stream()), "gww_dora_merge_batch_f32")
    return out if return_norm else [w for w, _ in out]


# ------------------------------------------------------------------ training-step kernels
def attention_lse(qkv: torch.Tensor, n_heads: int):
    """bf16 attention forward that also returns the row log-sum-exp [B, H, T] (fp32)."""
    qkv = _dev(qkv, torch.bfloat16, "qkv")
    B, T, d3 = qkv.shape
    ctx = torch.empty((B, T, d3 // 3), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, n_heads, T), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(lib().gww_attention_lse_bf16(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, T, n_heads, _stream()),
              "gww_attention_lse_bf16")
    return ctx, lse


def attention_bwd(qkv, ctx, dctx, lse, n_heads: int, q_log2: bool = False) -> torch.Tensor:
    """dqkv [B, T, 3 d] (bf16) of softmax(q k^T) v given dctx; ``q_log2``: the q section is in log2 units and its
    gradient is taken with respect to that stored q."""
    qkv, ctx, dctx = (_dev(t, torch.bfloat16) for t in (qkv, ctx, dctx))
    lse = _dev(lse, torch.float32, "lse")
    B, T, d3 = qkv.shape
    dqkv = torch.empty_like(qkv)
    scratch = torch.empty(B * n_heads * (T + (T + 63) // 64), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        fn = lib().gww_attention_bwd_log2q_bf16 if q_log2 else lib().gww_attention_bwd_bf16
        check(fn(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), scratch.data_ptr(), dqkv.data_ptr(),
                 B, T, n_heads, _stream()), "gww_attention_bwd_bf16")
    return dqkv


def attention_lse_f32(qkv: torch.Tensor, n_heads: int):
    """fp32 attention forward that also returns the row log-sum-exp [B, H, T]; ctx is bit-identical to
    ``gww_attention_f32``'s (``gww_attention_lse_f32``)."""
    qkv = _dev(qkv, torch.float32, "qkv")
    B, T, d3 = qkv.shape
    ctx = torch.empty((B, T, d3 // 3), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, n_heads, T), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(lib().gww_attention_lse_f32(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, T, n_heads, _stream()),
              "gww_attention_lse_f32")
    return ctx, lse


def attention_bwd_f32(qkv, ctx, dctx, lse, n_heads: int) -> torch.Tensor:
    """dqkv [B, T, 3 d] (fp32) of softmax(q k^T) v given dctx, exact fp32 (``gww_attention_bwd_f32``); the q section is
    the gradient with respect to the stored (pre-scaled) q."""
    qkv, ctx, dctx, lse = (_dev(t, torch.float32) for t in (qkv, ctx, dctx, lse))
    B, T, d3 = qkv.shape
    dqkv = torch.empty_like(qkv)
    scratch = torch.empty(lib().gww_attention_bwd_f32_scratch_bytes(B, T, n_heads) // 4, dtype=torch.float32,
                          device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(lib().gww_attention_bwd_f32(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(),
                                          scratch.data_ptr(), dqkv.data_ptr(), B, T, n_heads, _stream()),
              "gww_attention_bwd_f32")
    return dqkv


def layernorm_bwd(x, gamma, dy, dx=None, want_bf16: bool = False):
    """dx (+)= LayerNorm'(x)^T dy; dy fp32 or bf16.  Returns (dx fp32, dx bf16 | None)."""
    x = _dev(x, torch.float32, "x")
    M, d = x.shape
    dy = _dev(dy)
    acc = dx is not None
    if dx is None:
        dx = torch.empty_like(x)
    dxb = torch.empty((M, d), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    with torch.cuda.device(x.device):
        check(lib().gww_layernorm_bwd(x.data_ptr(), _dev(gamma, torch.float32).data_ptr(), dy.data_ptr(),
                                      int(dy.dtype == torch.float32), dx.data_ptr(), int(acc),
                                      dxb.data_ptr() if dxb is not None else None, M, d, _stream()), "gww_layernorm_bwd")
    return dx, dxb


def gemm_wgrad(dy, x, dw=None, db=None, alpha: float = 1.0, rows: int | None = None, k: int | None = None):
    """Weight-gradient GEMM: dw[N, K] += alpha dy[:rows]^T x[:rows, :K] (fp32, created as zeros when None) and, with
    ``db`` (a tensor, or True for a fresh one), db[N] += alpha sum_m dy[m].  dy / x are bf16 2-D tensors whose rows may
    be strided (``x`` may be an overlapping im2col view made with ``as_strided``: then pass ``k``).  Deterministic:
    the M reduction runs in a fixed order.  Returns (dw, db | None)."""
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or not dy.is_cuda or not x.is_cuda:
        raise _lib.GwwError("gemm_wgrad: dy and x must be bf16 GPU tensors")
    if dy.stride(1) != 1 or x.stride(1) != 1:
        raise _lib.GwwError("gemm_wgrad: rows must be contiguous")
    M = dy.shape[0] if rows is None else int(rows)
    N = dy.shape[1]
    K = x.shape[1] if k is None else int(k)
    if dw is None:
        dw = torch.zeros((N, K), dtype=torch.float32, device=dy.device)
    if db is True:
        db = torch.zeros((N,), dtype=torch.float32, device=dy.device)
    need = lib().gww_gemm_wgrad_workspace_bytes(M, N, K)
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dy.device)
    with torch.cuda.device(dy.device):
        check(lib().gww_gemm_wgrad_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), M, N, K, float(alpha),
                                        dw.data_ptr(), db.data_ptr() if db is not None else None, ws.data_ptr(),
                                        ws.numel(), _stream()), "gww_gemm_wgrad_bf16")
    return dw, db


def layernorm_param_grads(x, dy, dgamma=None, dbeta=None):
    """dgamma += sum_m dy * LayerNorm-normalised x, dbeta += sum_m dy (eps 1e-5; fp32, zeros when None; dy fp32 or
    bf16).  Deterministic fixed-order reduction.  Returns (dgamma, dbeta)."""
    x = _dev(x, torch.float32, "x")
    M, d = x.shape
    dy = _dev(dy)
    dgamma = torch.zeros(d, dtype=torch.float32, device=x.device) if dgamma is None else dgamma
    dbeta = torch.zeros(d, dtype=torch.float32, device=x.device) if dbeta is None else dbeta
    ws = torch.empty((lib().gww_layernorm_param_grads_workspace_bytes(M, d),), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_layernorm_param_grads(x.data_ptr(), dy.data_ptr(), int(dy.dtype == torch.float32), M, d,
                                              dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "gww_layernorm_param_grads")
    return dgamma, dbeta


def gelu_bf16(z, dgelu=None):
    z = _dev(z, torch.bfloat16, "z")
    out = torch.empty_like(z)
    with torch.cuda.device(z.device):
        check(lib().gww_gelu_bf16(z.data_ptr(), _dev(dgelu, torch.bfloat16).data_ptr() if dgelu is not None else None,
                                  out.data_ptr(), z.numel(), _stream()), "gww_gelu_bf16")
    return out


def dora_grads_multi(x, dy, y, col_off, bias_st, yscale, scaling, A, B, mag, nrm):
    """[(dA, dB, dm)] of up to three DoRA projections that read the same x (q, k, v of a layer) in one pass:
    x bf16 [M, d]; dy, y bf16 [M, W] with projection p in columns col_off[p] .. col_off[p] + d; the other arguments
    are per-projection lists.  d in {384, 512}, r = 8."""
    import ctypes as C
    x, dy, y = (_dev(t, torch.bfloat16) for t in (x, dy, y))
    M, d = x.shape
    n = len(col_off)
    keep = [[_dev(t, torch.float32) for t in lst] for lst in (bias_st, A, B, mag, nrm)]
    out = [(torch.zeros((8, d), dtype=torch.float32, device=x.device),
            torch.zeros((d, 8), dtype=torch.float32, device=x.device),
            torch.zeros((d,), dtype=torch.float32, device=x.device)) for _ in range(n)]
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    with torch.cuda.device(x.device):
        check(lib().gww_dora_grads_multi(x.data_ptr(), x.stride(0), dy.data_ptr(), y.data_ptr(), dy.stride(0), n,
                                         (C.c_long * n)(*col_off), ptrs(keep[0]), (C.c_float * n)(*yscale),
                                         (C.c_float * n)(*scaling), ptrs(keep[1]), ptrs(keep[2]), ptrs(keep[3]),
                                         ptrs(keep[4]), ptrs([o[0] for o in out]), ptrs([o[1] for o in out]),
                                         ptrs([o[2] for o in out]), M, d, _stream()), "gww_dora_grads_multi")
    return out


def dora_grads(x, dy, y, bias_st, yscale, scaling, A, B, mag, nrm, col_off: int = 0):
    """(dA [r,d], dB [d,r], dm [d]) of one DoRA projection.  x bf16 [M, d]; dy, y bf16 [M, W] (W >= col_off + d)
    whose columns col_off .. col_off + d hold the projection -- with W = 3 d and col_off 0 / d / 2 d, the q / k / v
    sections of the packed qkv / dqkv the encoder passes.  Rows of x and of dy / y may be strided (stride(1) == 1)."""
    if any(t.dtype != torch.bfloat16 or not t.is_cuda for t in (x, dy, y)):
        raise _lib.GwwError("dora_grads: x, dy and y must be bf16 GPU tensors")
    if x.dim() != 2 or dy.dim() != 2 or x.stride(1) != 1 or dy.stride(1) != 1 or dy.stride() != y.stride() \
            or dy.shape != y.shape:
        raise _lib.GwwError("dora_grads: 2-D x, dy, y with contiguous rows; dy and y of the same shape and strides")
    M, d = x.shape
    r = A.shape[0]
    if dy.shape[0] != M or col_off < 0 or col_off + d > dy.shape[1]:
        raise _lib.GwwError(f"dora_grads: dy / y {tuple(dy.shape)} hold no [{M}, {d}] section at column {col_off}")
    dA = torch.zeros((r, d), dtype=torch.float32, device=x.device)
    dB = torch.zeros((d, r), dtype=torch.float32, device=x.device)
    dm = torch.zeros((d,), dtype=torch.float32, device=x.device)
    f = lambda t: _dev(t, torch.float32).data_ptr()
    off = col_off * dy.element_size()
    with torch.cuda.device(x.device):
        check(lib().gww_dora_grads(x.data_ptr(), x.stride(0), dy.data_ptr() + off, y.data_ptr() + off, dy.stride(0),
                                   f(bias_st), float(yscale), float(scaling), f(A), f(B), f(mag), f(nrm),
                                   dA.data_ptr(), dB.data_ptr(), dm.data_ptr(), M, d, r, _stream()), "gww_dora_grads")
    return dA, dB, dm


def adapter_grads(x, dy, y, bias_st, yscale, scaling, A, B, mag, nrm):
    """(dA [r, d_in], dB [d_out, r], dm [d_out]) of one adapted linear layer of any shape the encoder has -- [d, d],
    fc1 [4d, d], fc2 [d, 4d] -- and rank 1..64 (``gww_adapter_grads``, matrix cores).  x bf16 [M, d_in]; dy, y bf16
    [M, d_out] (the stored output, bias included); rows may be strided (stride(1) == 1, dy and y with the same stride).
    Plain LoRA: mag = nrm = ones.  r > 64 raises GwwError."""
    if any(t.dtype != torch.bfloat16 or not t.is_cuda for t in (x, dy, y)):
        raise _lib.GwwError("adapter_grads: x, dy and y must be bf16 GPU tensors")
    if x.dim() != 2 or dy.dim() != 2 or x.stride(1) != 1 or dy.stride(1) != 1 or dy.stride() != y.stride() \
            or dy.shape != y.shape or dy.shape[0] != x.shape[0]:
        raise _lib.GwwError("adapter_grads: 2-D x [M, d_in], dy / y [M, d_out] with contiguous rows; dy and y of the same "
                            "shape and strides")
    M, d_in = x.shape
    d_out = dy.shape[1]
    r = A.shape[0]
    if tuple(A.shape) != (r, d_in) or tuple(B.shape) != (d_out, r):
        raise _lib.GwwError(f"adapter_grads: A {tuple(A.shape)} / B {tuple(B.shape)} do not fit x [{M}, {d_in}] and dy "
                            f"[{M}, {d_out}]")
    dA = torch.zeros((r, d_in), dtype=torch.float32, device=x.device)
    dB = torch.zeros((d_out, r), dtype=torch.float32, device=x.device)
    dm = torch.zeros((d_out,), dtype=torch.float32, device=x.device)
    f = lambda t: _dev(t, torch.float32).data_ptr()
    with torch.cuda.device(x.device):
        check(lib().gww_adapter_grads(x.data_ptr(), x.stride(0), dy.data_ptr(), y.data_ptr(), dy.stride(0), f(bias_st),
                                      float(yscale), float(scaling), f(A), f(B), f(mag), f(nrm), dA.data_ptr(),
                                      dB.data_ptr(), dm.data_ptr(), M, d_in, d_out, r, None, 0, _stream()),
              "gww_adapter_grads")
    return dA, dB, dm


def adapter_grads_f32(x, dy, y, bias_st, yscale, scaling, A, B, mag, nrm):
    """``adapter_grads`` in exact fp32 (``gww_adapter_grads_f32``): x fp32 [M, d_in]; dy, y fp32 [M, d_out] (rows may
    be strided, stride(1) == 1, dy and y with the same strides).  Returns fresh (dA, dB, dm).  r > 64 raises GwwError."""
    if any(t.dtype != torch.float32 or not t.is_cuda for t in (x, dy, y)):
        raise _lib.GwwError("adapter_grads_f32: x, dy and y must be fp32 GPU tensors")
    if x.dim() != 2 or dy.dim() != 2 or x.stride(1) != 1 or dy.stride(1) != 1 or dy.stride() != y.stride() \
            or dy.shape != y.shape or dy.shape[0] != x.shape[0]:
        raise _lib.GwwError("adapter_grads_f32: 2-D x [M, d_in], dy / y [M, d_out] with contiguous rows; dy and y of "
                            "the same shape and strides")
    M, d_in = x.shape
    d_out = dy.shape[1]
    r = A.shape[0]
    if tuple(A.shape) != (r, d_in) or tuple(B.shape) != (d_out, r):
        raise _lib.GwwError(f"adapter_grads_f32: A {tuple(A.shape)} / B {tuple(B.shape)} do not fit x [{M}, {d_in}] "
                            f"and dy [{M}, {d_out}]")
    dA = torch.zeros((r, d_in), dtype=torch.float32, device=x.device)
    dB = torch.zeros((d_out, r), dtype=torch.float32, device=x.device)
    dm = torch.zeros((d_out,), dtype=torch.float32, device=x.device)
    f = lambda t: _dev(t, torch.float32).data_ptr()
    with torch.cuda.device(x.device):
        check(lib().gww_adapter_grads_f32(x.data_ptr(), x.stride(0), dy.data_ptr(), y.data_ptr(), dy.stride(0),
                                          f(bias_st), float(yscale), float(scaling), f(A), f(B), f(mag), f(nrm),
                                          dA.data_ptr(), dB.data_ptr(), dm.data_ptr(), M, d_in, d_out, r, None, 0,
                                          _stream()), "gww_adapter_grads_f32")
    return dA, dB, dm


def info_nce_forward(z1, z2, temperature: float):
    """InfoNCE of the reference's ContrastivePretrainer (``gww_info_nce_forward_f32``): z1, z2 fp32 [B, P] (P <= 1024) ->
    (loss [1] device scalar, saved = (n [2B, P], nrm [2B], lse [2B], term [2B]) for ``info_nce_backward``).
    A row's norm is the square root of an fp32 sum of squares, as in the fp32 reference: rows with |z| above about
    1.8e19 overflow that sum (inf norm, zero direction) and are outside what this computes."""
    z1 = _dev(z1, torch.float32, "z1")
    z2 = _dev(z2, torch.float32, "z2")
    if z1.dim() != 2 or z1.shape != z2.shape:
        raise _lib.GwwError(f"info_nce: z1 {tuple(z1.shape)} and z2 {tuple(z2.shape)} must be the same [B, P]")
    B, P = z1.shape
    dev = z1.device
    n = torch.empty((2 * B, P), dtype=torch.float32, device=dev)
    rows = torch.empty((3, 2 * B), dtype=torch.float32, device=dev)          # nrm | lse | per-row term
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_info_nce_forward_f32(z1.data_ptr(), z2.data_ptr(), B, P, float(temperature), n.data_ptr(),
                                             rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), loss.data_ptr(),
                                             _stream()), "gww_info_nce_forward_f32")
    return loss, (n, rows[0], rows[1], rows[2])


def info_nce_backward(saved, temperature: float, dloss):
    """(dz1, dz2) [B, P] of ``info_nce_forward``'s loss times the device scalar ``dloss``."""
    n, nrm, lse, term = saved
    dloss = _dev(dloss.reshape(1), torch.float32, "dloss")
    B, P = n.shape[0] // 2, n.shape[1]
    dz = torch.empty((2, B, P), dtype=torch.float32, device=n.device)
    with torch.cuda.device(n.device):
        check(lib().gww_info_nce_backward_f32(n.data_ptr(), nrm.data_ptr(), lse.data_ptr(), term.data_ptr(), B, P,
                                              float(temperature),
                                              dloss.data_ptr(), dz[0].data_ptr(), dz[1].data_ptr(), _stream()),
              "gww_info_nce_backward_f32")
    return dz[0], dz[1]


def qadapter_tail_backward(g, y, scale, bias, gamma_i, F: int, T: int):
    """Backward of ``gww_qadapter_tail_f32`` for one detector (``gww_qadapter_tail_backward_f32``): g fp32 [B, F, T] (rows
    contiguous; any batch stride, e.g. ``g_out[:, det]``), y fp32 [B, Hin, Win]; scale, bias, gamma_i device scalars.
    Returns (d_y, d_scale [1], d_bias [1], d_gamma_i [1], d_beta_i [1])."""
    if not g.is_cuda:
        raise _lib.GwwError("qadapter_tail_backward: g must live on the GPU")
    if g.dtype != torch.float32 or g.stride(-1) != 1 or g.stride(-2) != T:
        g = g.to(torch.float32).contiguous()
    y = _dev(y, torch.float32, "y")
    B, Hin, Win = y.shape
    dev = y.device
    d_y = torch.empty_like(y)
    d = torch.empty((4, 1), dtype=torch.float32, device=dev)
    ws = torch.empty((lib().gww_qadapter_tail_backward_workspace_bytes(B, Hin),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_qadapter_tail_backward_f32(g.data_ptr(), g.stride(0), y.data_ptr(), B, Hin, Win, F, T,
                                                   _dev(scale, torch.float32, "scale").data_ptr(),
                                                   _dev(bias, torch.float32, "bias").data_ptr(),
                                                   _dev(gamma_i, torch.float32, "gamma_i").data_ptr(), d_y.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), d[0].data_ptr(), d[1].data_ptr(),
                                                   d[2].data_ptr(), d[3].data_ptr(), _stream()),
              "gww_qadapter_tail_backward_f32")
    return d_y, d[0], d[1], d[2], d[3]


def assemble_batch(noise, wave, idx_noise, idx_wave, snr):
    """Rows ``noise[idx_noise[r]] + snr[r] * wave[idx_wave[r]]`` (``idx_wave[r] < 0``: the noise row alone) of device-resident
    ``noise [N, ...]`` / ``wave [M, ...]`` fp32, bit for bit torch's fp32 arithmetic (``gww_assemble_batch_f32``).  The
    plan (host int / float arrays of R entries) is checked against the array sizes here, then uploaded in one copy.
    Returns [R, *noise.shape[1:]]."""
    import numpy as np
    noise = _dev(noise, torch.float32, "noise")
    wave = _dev(wave, torch.float32, "wave")
    if wave.shape[1:] != noise.shape[1:]:
        raise _lib.GwwError(f"assemble_batch: noise rows {tuple(noise.shape[1:])} != wave rows {tuple(wave.shape[1:])}")
    idx_noise = np.asarray(idx_noise, np.int64).reshape(-1)
    idx_wave = np.asarray(idx_wave, np.int64).reshape(-1)
    snr = np.asarray(snr, np.float32).reshape(-1)
    R = len(idx_noise)
    if len(idx_wave) != R or len(snr) != R or R < 1:
        raise _lib.GwwError("assemble_batch: idx_noise, idx_wave and snr must have the same length >= 1")
    if idx_noise.min() < 0 or idx_noise.max() >= noise.shape[0] or idx_wave.max() >= wave.shape[0]:
        raise _lib.GwwError(f"assemble_batch: index out of range (noise {noise.shape[0]}, wave {wave.shape[0]})")
    plan = np.empty((3, R), np.int32)
    plan[0], plan[1] = idx_noise, idx_wave
    plan[2] = snr.view(np.int32)
    plan_d = torch.from_numpy(plan).to(noise.device, non_blocking=False)
    out = torch.empty((R, *noise.shape[1:]), dtype=torch.float32, device=noise.device)
    with torch.cuda.device(noise.device):
        check(lib().gww_assemble_batch_f32(noise.data_ptr(), noise.shape[0], wave.data_ptr(), wave.shape[0],
                                           noise[0].numel(), plan_d[0].data_ptr(), plan_d[1].data_ptr(),
                                           plan_d[2].data_ptr(), R, out.data_ptr(), _stream()), "gww_assemble_batch_f32")
    return out


HEAD_WIDTHS = (512, 256, 128)      # hidden widths of models.glitch_classifier's head (Glitch_classification/src/model.py)
DET_WIDTHS = (512, 256, 128, 64)   # hidden widths of models.efficiency_classifier's head (Efficiency_test/src/network.py:73-85)


def _mlp_params(params, widths, who, chain):
    """The ``nn.Linear`` tensors (w1, b1, ...) of the chain d_in -> widths -> C, checked: (fp32 GPU tensors, d_in, C)."""
    n = len(widths) + 1
    if len(params) != 2 * n:
        raise _lib.GwwError(f"{who}: expected ({', '.join(f'w{i}, b{i}' for i in range(1, n + 1))})")
    ps = [_dev(p, torch.float32, "head parameter") for p in params]
    d_in, C = ps[0].shape[1], ps[-2].shape[0]
    dims = (d_in, *widths, C)
    for i, p in enumerate(ps):
        s = (dims[i // 2 + 1], dims[i // 2]) if i % 2 == 0 else (dims[i // 2 + 1],)
        if tuple(p.shape) != s:
            raise _lib.GwwError(f"{who}: parameter of shape {tuple(p.shape)} where the {chain} d_in -> "
                                f"{' -> '.join(map(str, widths))} -> C has {s}")
    return ps, d_in, C


def _mlp_outputs(x, widths, C, n_bc):
    """What a head's forward fills: the saved activations, ``n_bc`` [B, C] tensors, row_loss [B], loss [1]."""
    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=x.device)
    B = x.shape[0]
    return [new(B, w) for w in widths], [new(B, C) for _ in range(n_bc)], new(B), new(1)


def _mlp_grads(x, ps, dloss, ws, ws_bytes):
    """What a head's backward takes and fills: dloss' pointer (or None), the fp32 workspace, dx, the parameter gradients."""
    if dloss is not None:
        dloss = _dev(dloss.reshape(1), torch.float32, "dloss").data_ptr()
    if ws is None:
        ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=x.device)
    return dloss, _dev(ws, torch.float32, "ws"), torch.empty_like(x), [torch.empty_like(t) for t in ps]


def _mlp_blocks(ps, h=None, logits=None, grads=None):
    """The blocks the C entries of the heads take (``gww_mlp_params``, ``gww_mlp_acts``, ``gww_mlp_grads``, by reference; None
    for a list that is not given) from the checked tensors: ps = [w1, b1, ...], the activations h, grads = [dw1, db1, ...]."""
    def ptrs(ts, n):
        return (_lib.C.c_void_p * n)(*[t.data_ptr() for t in ts])
    n = _lib.MLP_MAX_LAYERS
    blocks = (_lib.MlpParams(len(ps) // 2, ptrs(ps[0::2], n), ptrs(ps[1::2], n)),
              None if h is None else _lib.MlpActs(ptrs(h, n - 1), None if logits is None else logits.data_ptr()),
              None if grads is None else _lib.MlpGrads(ptrs(grads[0::2], n), ptrs(grads[1::2], n)))
    return [b if b is None else _lib.C.byref(b) for b in blocks]


def _state(t, dt, shape, who, name):
    if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
        raise _lib.GwwError(f"{who}: {name} must be a contiguous GPU {dt} tensor of shape {shape}")


def head_forward(x, params, labels, p: float = 0.3, train: bool = False, seed: int = 0, offset: int = 0):
    """Glitch head + CrossEntropyLoss forward (``gww_head_forward_f32``, 2 launches): x fp32 [B, d_in], params the eight
    ``nn.Linear`` tensors of ``glitch_classifier.classifier`` in order, labels int64 [B].  Returns (loss [1] device
    scalar, logits [B, C], row_loss [B], pred [B] int64, saved) with ``saved`` what ``head_backward`` needs."""
    x = _dev(x, torch.float32, "x")
    labels = _dev(labels, torch.int64, "labels")
    ps, d_in, C = _mlp_params(params, HEAD_WIDTHS, "head", "glitch head")
    if x.dim() != 2 or x.shape[1] != d_in or labels.shape != (x.shape[0],):
        raise _lib.GwwError(f"head_forward: x {tuple(x.shape)} / labels {tuple(labels.shape)} do not fit d_in = {d_in}")
    B, dev = x.shape[0], x.device
    h, (logits, dz), row_loss, loss = _mlp_outputs(x, HEAD_WIDTHS, C, 2)
    pred = torch.empty((B,), dtype=torch.int64, device=dev)
    P, A, _ = _mlp_blocks(ps, h, logits)
    with torch.cuda.device(dev):
        check(lib().gww_head_forward_f32(x.data_ptr(), P, labels.data_ptr(), B, d_in, C, float(p), int(bool(train)),
                                         int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), A, row_loss.data_ptr(),
                                         pred.data_ptr(), dz.data_ptr(), loss.data_ptr(), _stream()), "gww_head_forward_f32")
    return loss, logits, row_loss, pred, (x, ps, h, dz, float(p), bool(train))


def head_scan(x, params, cls=None, prob=None, probs=None, row_offset: int = 0, n_rows: int | None = None,
              want_probs: bool = False):
    """The glitch head in eval mode (``gww_head_scan_f32``, one launch, nothing saved): x fp32 [B, d_in], params as
    ``head_forward`` takes them.  Row r of the batch writes element ``row_offset + r`` of ``cls`` (int32: the class, by
    ``head_forward``'s argmax rule), ``prob`` (fp32: its softmax probability) and, if there, ``probs`` [., C].  Without
    ``cls`` / ``prob`` they are allocated here with ``n_rows`` rows (default: ``row_offset + B``; ``probs`` with
    ``want_probs``) -- a scan allocates them series-long with its first batch and hands them back with every later one.
    Returns (cls, prob, probs or None)."""
    x = _dev(x, torch.float32, "x")
    ps, d_in, C = _mlp_params(params, HEAD_WIDTHS, "head", "glitch head")
    if x.dim() != 2 or x.shape[1] != d_in:
        raise _lib.GwwError(f"head_scan: x {tuple(x.shape)} does not fit d_in = {d_in}")
    B, dev, row_offset = x.shape[0], x.device, int(row_offset)
    if (cls is None) != (prob is None):
        raise _lib.GwwError("head_scan: give both cls and prob, or neither")
    if cls is None:
        n_rows = row_offset + B if n_rows is None else int(n_rows)
        cls = torch.empty((n_rows,), dtype=torch.int32, device=dev)
        prob = torch.empty((n_rows,), dtype=torch.float32, device=dev)
        if want_probs:
            probs = torch.empty((n_rows, C), dtype=torch.float32, device=dev)
    n_rows = int(cls.shape[0]) if cls.dim() == 1 else -1
    _state(cls, torch.int32, (n_rows,), "head_scan", "cls")
    _state(prob, torch.float32, (n_rows,), "head_scan", "prob")
    if probs is not None:
        _state(probs, torch.float32, (n_rows, C), "head_scan", "probs")
    if row_offset < 0 or row_offset + B > n_rows:
        raise _lib.GwwError(f"head_scan: rows {row_offset} .. {row_offset + B - 1} do not fit outputs of {n_rows} rows")
    P, _, _ = _mlp_blocks(ps)
    with torch.cuda.device(dev):
        check(lib().gww_head_scan_f32(x.data_ptr(), P, B, d_in, C, row_offset, cls.data_ptr(), prob.data_ptr(),
                                      None if probs is None else probs.data_ptr(), _stream()), "gww_head_scan_f32")
    return cls, prob, probs


def glitch_events(times, cls, prob, prob_threshold: float = 0.5, gap: float = 0.35, ignore: int = 0, cap: int | None = None):
    """The events of every class from the per-window results of one series (``gww_glitch_events``, two launches, no host
    sync): times fp64 [n], cls int32 [n], prob fp32 [n]; ``ignore``: bit c set skips class c.  Returns a dict of device
    tensors of ``cap`` entries (default n, which cannot overflow) -- ``cls`` ``first`` ``n`` (int32), ``t_start`` ``t_end``
    ``t_peak`` (fp64), ``p_peak`` (fp32) -- and ``count`` int32 [1], which counts on past ``cap``; the semantics are
    ``glitch_scan.build_events_host``'s, bit for bit."""
    times = _dev(times, torch.float64, "times")
    cls = _dev(cls, torch.int32, "cls")
    prob = _dev(prob, torch.float32, "prob")
    if times.dim() != 1 or cls.shape != times.shape or prob.shape != times.shape:
        raise _lib.GwwError(f"glitch_events: times {tuple(times.shape)}, cls {tuple(cls.shape)} and prob {tuple(prob.shape)} "
                            "must be [n]")
    n, dev = int(times.shape[0]), times.device
    cap = n if cap is None else int(cap)
    ignore = int(ignore)
    if cap < 0 or not 0 <= ignore < 2 ** 64:
        raise _lib.GwwError(f"glitch_events: cap={cap} must be >= 0 and ignore a 64-bit mask")
    ev = {k: torch.empty((cap,), dtype=dt, device=dev)
          for k, dt in (("cls", torch.int32), ("first", torch.int32), ("n", torch.int32), ("t_start", torch.float64),
                        ("t_end", torch.float64), ("t_peak", torch.float64), ("p_peak", torch.float32))}
    ev["count"] = torch.empty((1,), dtype=torch.int32, device=dev)
    ws_bytes = lib().gww_glitch_events_workspace_bytes(n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_glitch_events(times.data_ptr(), cls.data_ptr(), prob.data_ptr(), n, float(prob_threshold), float(gap),
                                      ignore, cap, *[ev[k].data_ptr() for k in ("cls", "first", "n", "t_start", "t_end",
                                                                                "t_peak", "p_peak", "count")],
                                      ws.data_ptr(), ws_bytes, _stream()), "gww_glitch_events")
    return ev


def head_backward(saved, dloss=None):
    """(dx [B, d_in], [dw1, db1, ..., dw4, db4]) of ``head_forward``'s loss times the device scalar ``dloss``
    (``gww_head_backward_f32``, 2 launches; no host sync)."""
    x, ps, h, dz, p, train = saved
    B, d_in, C, dev = x.shape[0], x.shape[1], dz.shape[1], x.device
    dloss, ws, dx, grads = _mlp_grads(x, ps, dloss, None, lib().gww_head_workspace_bytes(B, C))
    P, A, G = _mlp_blocks(ps, h, None, grads)
    with torch.cuda.device(dev):
        check(lib().gww_head_backward_f32(x.data_ptr(), P, A, dz.data_ptr(), dloss, B, d_in, C, p, int(train), ws.data_ptr(),
                                          ws.numel() * 4, dx.data_ptr(), G, _stream()), "gww_head_backward_f32")
    return dx, grads


def head_dropout_mask(seed: int, offset: int, layer: int, B: int, width: int, p: float = 0.3, device="cuda"):
    """The [B, width] fp32 mask (1 kept / 0 dropped) ``head_forward(train=True)`` applies after hidden layer ``layer``
    (0, 1, 2) for this (seed, offset): Philox4x32-10 on the element index, independent of B and of launch geometry."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.GwwError(f"head_dropout_mask: device must be a GPU (got {device}); gw_whisper_amd has no CPU path")
    mask = torch.empty((B, width), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(lib().gww_head_dropout_mask_f32(int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), layer, B, width,
                                              float(p), mask.data_ptr(), _stream()), "gww_head_dropout_mask_f32")
    return mask


def eval_accumulate(logits, labels, row_loss, confusion, loss_sum, n):
    """One batch into the device-resident evaluation state (``gww_eval_accumulate``, one launch, no host sync):
    confusion int64 [C, C] (rows = true class), loss_sum fp64 [1], n int64 [1] are updated in place."""
    logits = _dev(logits, torch.float32, "logits")
    labels = _dev(labels, torch.int64, "labels")
    row_loss = _dev(row_loss, torch.float32, "row_loss")
    B, C = logits.shape
    for t, dt, shape, name in ((confusion, torch.int64, (C, C), "confusion"), (loss_sum, torch.float64, (1,), "loss_sum"),
                               (n, torch.int64, (1,), "n")):
        _state(t, dt, shape, "eval_accumulate", name)
    if labels.shape != (B,) or row_loss.shape != (B,):
        raise _lib.GwwError("eval_accumulate: labels and row_loss must be [B]")
    with torch.cuda.device(logits.device):
        check(lib().gww_eval_accumulate(logits.data_ptr(), labels.data_ptr(), row_loss.data_ptr(), B, C,
                                        confusion.data_ptr(), loss_sum.data_ptr(), n.data_ptr(), _stream()),
              "gww_eval_accumulate")


CNN_CHANNELS = (2, 64, 128, 256)   # models.TwoChannelLIGOBinaryClassifierCNN's conv chain (Signal_vs_Noise/src/model.py:63-73)


def _cnn_params(params, who):
    """The eight tensors of the CNN head (conv weights [Cout, Cin, 3], Linear [C, 256]) checked: (fp32 GPU tensors, C)."""
    if len(params) != 8:
        raise _lib.GwwError(f"{who}: expected (w1, b1, w2, b2, w3, b3, w4, b4)")
    ps = [_dev(p, torch.float32, "head parameter") for p in params]
    C = ps[6].shape[0] if ps[6].dim() == 2 else -1
    shapes = []
    for i in range(3):
        shapes += [(CNN_CHANNELS[i + 1], CNN_CHANNELS[i], 3), (CNN_CHANNELS[i + 1],)]
    shapes += [(C, CNN_CHANNELS[3]), (C,)]
    for p, s in zip(ps, shapes):
        if tuple(p.shape) != s:
            raise _lib.GwwError(f"{who}: parameter of shape {tuple(p.shape)} where the CNN head 2 -> 64 -> 128 -> 256 -> C "
                                f"has {s}")
    return ps, C


def cnn_head_forward(x, params, train: bool = False):
    """CNN decoder head forward (``gww_cnn_head_forward_f32``, one launch): x fp32 [B, 2, d], params the eight tensors of
    ``TwoChannelLIGOBinaryClassifierCNN.classifier`` in order.  Returns logits [B, C]; with ``train`` (logits, saved), the
    logits bit for bit the same, ``saved`` what ``cnn_head_backward`` needs (``saved[2]``: the post-ReLU activations
    [B, 64 + 128 + 256, d])."""
    x = _dev(x, torch.float32, "x")
    ps, C = _cnn_params(params, "cnn_head_forward")
    if x.dim() != 3 or x.shape[1] != 2:
        raise _lib.GwwError(f"cnn_head_forward: x {tuple(x.shape)} is not [B, 2, d]")
    B, d = x.shape[0], x.shape[2]
    logits = torch.empty((B, C), dtype=torch.float32, device=x.device)
    acts = torch.empty((B, sum(CNN_CHANNELS[1:]), d), dtype=torch.float32, device=x.device) if train else None
    with torch.cuda.device(x.device):
        check(lib().gww_cnn_head_forward_f32(x.data_ptr(), *[t.data_ptr() for t in ps], B, d, C, logits.data_ptr(),
                                             acts.data_ptr() if train else None, _stream()), "gww_cnn_head_forward_f32")
    return (logits, (x, ps, acts)) if train else logits


def cnn_head_backward(saved, dlogits, ws=None):
    """(dx [B, 2, d], [dw1, db1, ..., dw4, db4]) of ``cnn_head_forward(train=True)`` for the upstream gradient dlogits
    [B, C] (``gww_cnn_head_backward_f32``; no host sync, no float atomics).  ``ws``: a caller's fp32 workspace of at least
    ``gww_cnn_head_workspace_bytes(B, d, C)`` bytes (allocated here when None)."""
    x, ps, acts = saved
    B, d, C = x.shape[0], x.shape[2], ps[6].shape[0]
    dlogits = _dev(dlogits, torch.float32, "dlogits")
    if tuple(dlogits.shape) != (B, C):
        raise _lib.GwwError(f"cnn_head_backward: dlogits {tuple(dlogits.shape)} is not [B, C] = {(B, C)}")
    if ws is None:
        ws = torch.empty((lib().gww_cnn_head_workspace_bytes(B, d, C) // 4,), dtype=torch.float32, device=x.device)
    ws = _dev(ws, torch.float32, "ws")
    dx = torch.empty_like(x)
    grads = [torch.empty_like(t) for t in ps]
    with torch.cuda.device(x.device):
        check(lib().gww_cnn_head_backward_f32(x.data_ptr(), acts.data_ptr(), dlogits.data_ptr(),
                                              *[t.data_ptr() for t in ps[0::2]], B, d, C, dx.data_ptr(),
                                              *[g.data_ptr() for g in grads], ws.data_ptr(), ws.numel() * 4, _stream()),
              "gww_cnn_head_backward_f32")
    return dx, grads


SCORE_PROB0, SCORE_LOGIT_DIFF = 0, 1
MAX_FAPS = 8


def det_head_forward(x, params, targets, epsilon: float = 1e-6):
    """Detection head + Softmax + regularised BCELoss forward (``gww_det_head_forward_f32``, 2 launches): x fp32 [B, d_in],
    params the ten ``nn.Linear`` tensors of ``efficiency_classifier.classifier`` in order, targets fp32 [B, C] in [0, 1].
    Returns (loss [1] device scalar, logits [B, C], probs [B, C], row_loss [B], saved) with ``saved`` what
    ``det_head_backward`` needs."""
    x = _dev(x, torch.float32, "x")
    targets = _dev(targets, torch.float32, "targets")
    ps, d_in, C = _mlp_params(params, DET_WIDTHS, "det_head", "detection head")
    if x.dim() != 2 or x.shape[1] != d_in or tuple(targets.shape) != (x.shape[0], C):
        raise _lib.GwwError(f"det_head_forward: x {tuple(x.shape)} / targets {tuple(targets.shape)} do not fit d_in = {d_in}, "
                            f"C = {C}")
    h, (logits, probs, dz), row_loss, loss = _mlp_outputs(x, DET_WIDTHS, C, 3)
    P, A, _ = _mlp_blocks(ps, h, logits)
    with torch.cuda.device(x.device):
        check(lib().gww_det_head_forward_f32(x.data_ptr(), P, targets.data_ptr(), x.shape[0], d_in, C, float(epsilon), A,
                                             probs.data_ptr(), row_loss.data_ptr(), dz.data_ptr(), loss.data_ptr(), _stream()),
              "gww_det_head_forward_f32")
    return loss, logits, probs, row_loss, (x, ps, h, dz)


def det_head_backward(saved, dloss=None, ws=None):
    """(dx [B, d_in], [dw1, db1, ..., dw5, db5]) of ``det_head_forward``'s loss times the device scalar ``dloss``
    (``gww_det_head_backward_f32``, 2 launches; no host sync).  ``ws``: a caller's fp32 workspace of at least
    ``gww_det_head_workspace_bytes(B, C)`` bytes (allocated here when None)."""
    x, ps, h, dz = saved
    B, d_in, C, dev = x.shape[0], x.shape[1], dz.shape[1], x.device
    dloss, ws, dx, grads = _mlp_grads(x, ps, dloss, ws, lib().gww_det_head_workspace_bytes(B, C))
    P, A, G = _mlp_blocks(ps, h, None, grads)
    with torch.cuda.device(dev):
        check(lib().gww_det_head_backward_f32(x.data_ptr(), P, A, dz.data_ptr(), dloss, B, d_in, C, ws.data_ptr(), ws.numel() * 4,
                                              dx.data_ptr(), G, _stream()), "gww_det_head_backward_f32")
    return dx, grads


def det_head_scores(x, params, out, mode: int = SCORE_PROB0):
    """One score per row of x into ``out`` (``gww_det_head_scores_f32``, one launch, inference only): ``probs[:, 0]``
    (mode SCORE_PROB0) or ``z0 - z1`` (SCORE_LOGIT_DIFF, C = 2).  ``out``: a 1-d fp32 GPU view of B elements, of any
    stride -- a slice of the score buffer of a whole pass."""
    x = _dev(x, torch.float32, "x")
    ps, d_in, C = _mlp_params(params, DET_WIDTHS, "det_head", "detection head")
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != d_in:
        raise _lib.GwwError(f"det_head_scores: x {tuple(x.shape)} does not fit d_in = {d_in}")
    if not out.is_cuda or out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != B or (B > 1 and out.stride(0) < 1):
        raise _lib.GwwError(f"det_head_scores: out must be a 1-d fp32 GPU view of {B} elements with a positive stride")
    with torch.cuda.device(x.device):
        check(lib().gww_det_head_scores_f32(x.data_ptr(), _mlp_blocks(ps)[0], B, d_in, C, int(mode), out.data_ptr(),
                                            max(out.stride(0), 1), _stream()), "gww_det_head_scores_f32")
    return out


def det_head_scores2(x, params, out=None, remove_softmax: bool = False):
    """Both outputs of the detection head per row of x (``gww_det_head_scores2_f32``, one launch, inference only): the
    softmax ``probs`` [B, C], or with ``remove_softmax`` (C = 2) the pair ``(z0 - z1, z1 - z0)`` of the reference's
    mutual-subtraction layer (``test_network.py:89-99``).  ``out``: a 2-d fp32 GPU view [B, C] with unit column stride and
    any row pitch >= C -- rows of the output of a whole file -- allocated here when None."""
    x = _dev(x, torch.float32, "x")
    ps, d_in, C = _mlp_params(params, DET_WIDTHS, "det_head", "detection head")
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != d_in:
        raise _lib.GwwError(f"det_head_scores2: x {tuple(x.shape)} does not fit d_in = {d_in}")
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    if (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (B, C) or out.stride(1) != 1
            or (B > 1 and out.stride(0) < C)):
        raise _lib.GwwError(f"det_head_scores2: out must be an fp32 GPU view [{B}, {C}] with unit column stride")
    with torch.cuda.device(x.device):
        check(lib().gww_det_head_scores2_f32(x.data_ptr(), _mlp_blocks(ps)[0], B, d_in, C, 1 if remove_softmax else 0,
                                             out.data_ptr(), max(out.stride(0), C), _stream()), "gww_det_head_scores2_f32")
    return out


BIN_HEAD_ONE, BIN_HEAD_TWO = 1, 2           # include/gww.h GWW_BIN_HEAD_*: the number of detectors
# hidden widths of models.one_channel_ligo_binary_classifier / two_channel_ligo_binary_classifier (Signal_vs_Noise/src/model.py)
BIN_HEAD_WIDTHS = {BIN_HEAD_ONE: (512, 256, 128, 64), BIN_HEAD_TWO: (1024, 512, 256)}


def _bin_layout(layout, params, who):
    if layout not in BIN_HEAD_WIDTHS:
        raise _lib.GwwError(f"{who}: layout={layout!r} must be BIN_HEAD_ONE ({BIN_HEAD_ONE}) or BIN_HEAD_TWO ({BIN_HEAD_TWO})")
    widths = BIN_HEAD_WIDTHS[layout]
    return (widths, *_mlp_params(params, widths, who, "one-detector binary head" if layout == BIN_HEAD_ONE
                                 else "two-detector binary head"))


def bin_head_forward(layout: int, x, params, targets):
    """Binary head + BCEWithLogitsLoss forward (``gww_bin_head_forward_f32``, 2 launches): x fp32 [B, d_in], params the
    ``nn.Linear`` tensors of the classifier in order (ten for BIN_HEAD_ONE, eight for BIN_HEAD_TWO), targets fp32 [B, C] in
    [0, 1].  Returns (loss [1] device scalar, logits [B, C], probs [B, C], row_loss [B], saved) with ``saved`` what
    ``bin_head_backward`` needs (``saved[3]``: the post-ReLU activations, ``saved[4]``: dz)."""
    x = _dev(x, torch.float32, "x")
    targets = _dev(targets, torch.float32, "targets")
    widths, ps, d_in, C = _bin_layout(layout, params, "bin_head_forward")
    if x.dim() != 2 or x.shape[1] != d_in or tuple(targets.shape) != (x.shape[0], C):
        raise _lib.GwwError(f"bin_head_forward: x {tuple(x.shape)} / targets {tuple(targets.shape)} do not fit d_in = {d_in}, "
                            f"C = {C}")
    h, (logits, probs, dz), row_loss, loss = _mlp_outputs(x, widths, C, 3)
    P, A, _ = _mlp_blocks(ps, h, logits)
    with torch.cuda.device(x.device):
        check(lib().gww_bin_head_forward_f32(int(layout), x.data_ptr(), P, targets.data_ptr(), x.shape[0], d_in, C, A,
                                             probs.data_ptr(), row_loss.data_ptr(), dz.data_ptr(), loss.data_ptr(), _stream()),
              "gww_bin_head_forward_f32")
    return loss, logits, probs, row_loss, (int(layout), x, ps, h, dz)


def bin_head_backward(saved, dloss=None, ws=None):
    """(dx [B, d_in], [dw1, db1, ...]) of ``bin_head_forward``'s loss times the device scalar ``dloss``
    (``gww_bin_head_backward_f32``, 2 launches; no host sync).  ``ws``: a caller's fp32 workspace of at least
    ``gww_bin_head_workspace_bytes(layout, B, C)`` bytes (allocated here when None)."""
    layout, x, ps, h, dz = saved
    B, d_in, C, dev = x.shape[0], x.shape[1], dz.shape[1], x.device
    dloss, ws, dx, grads = _mlp_grads(x, ps, dloss, ws, lib().gww_bin_head_workspace_bytes(layout, B, C))
    P, A, G = _mlp_blocks(ps, h, None, grads)
    with torch.cuda.device(dev):
        check(lib().gww_bin_head_backward_f32(layout, x.data_ptr(), P, A, dz.data_ptr(), dloss, B, d_in, C, ws.data_ptr(),
                                              ws.numel() * 4, dx.data_ptr(), G, _stream()), "gww_bin_head_backward_f32")
    return dx, grads


def bin_head_scores(layout: int, x, params):
    """logits [B, C] of the binary head (``gww_bin_head_scores_f32``, one launch, inference only): bit for bit what
    ``bin_head_forward`` gives."""
    x = _dev(x, torch.float32, "x")
    _widths, ps, d_in, C = _bin_layout(layout, params, "bin_head_scores")
    if x.dim() != 2 or x.shape[1] != d_in:
        raise _lib.GwwError(f"bin_head_scores: x {tuple(x.shape)} does not fit d_in = {d_in}")
    logits = torch.empty((x.shape[0], C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().gww_bin_head_scores_f32(int(layout), x.data_ptr(), _mlp_blocks(ps)[0], x.shape[0], d_in, C,
                                            logits.data_ptr(), _stream()), "gww_bin_head_scores_f32")
    return logits


SLIDE_LOGIT0, SLIDE_PROB0 = 0, 1
SLIDE_WIDTHS = (256, 128, 64)      # layers 2..5 of the search head behind its 512-wide first layer
SLIDE_MAX_D, SLIDE_MAX_S = 4, 65535


def slide_scores(partials, params, offsets, mode: int = SLIDE_LOGIT0, out=None):
    """Scores of time-slid detector pairs (``gww_slide_scores_f32``, one launch): ``partials`` fp32 [D, N, 512], the first
    layer's per-detector partial products (bias in detector 0); ``params`` the eight tensors (w2, b2, ..., w5, b5) of
    layers 2..5; ``offsets`` the S window offsets (python ints, checked here: 0 <= o < N).  Returns fp32 [S, N] with
    row s = the head on ``relu(sum_g partials[g][(i + g * offsets[s]) mod N])``: ``z[0]`` (SLIDE_LOGIT0) or
    ``softmax(z)[0]`` (SLIDE_PROB0).  ``out``: a contiguous fp32 [S, N] GPU tensor to write instead of a new one."""
    partials = _dev(partials, torch.float32, "partials")
    if partials.dim() != 3 or partials.shape[2] != 512 or partials.shape[1] < 1:
        raise _lib.GwwError(f"slide_scores: partials must be [D, N >= 1, 512], got {tuple(partials.shape)}")
    D, N = int(partials.shape[0]), int(partials.shape[1])
    if not 2 <= D <= SLIDE_MAX_D:
        raise _lib.GwwError(f"slide_scores: D={D} detectors; time slides need 2..{SLIDE_MAX_D}")
    ps, d_in, C = _mlp_params(params, SLIDE_WIDTHS, "slide_scores", "slide head")
    if d_in != 512:
        raise _lib.GwwError(f"slide_scores: w2 must be [256, 512], got {tuple(ps[0].shape)}")
    if mode not in (SLIDE_LOGIT0, SLIDE_PROB0):
        raise _lib.GwwError(f"slide_scores: mode={mode} must be SLIDE_LOGIT0 or SLIDE_PROB0")
    if mode == SLIDE_PROB0 and C < 2:
        raise _lib.GwwError("slide_scores: the softmax score needs C >= 2 classes")
    offs = [int(o) for o in offsets]
    if not 1 <= len(offs) <= SLIDE_MAX_S:
        raise _lib.GwwError(f"slide_scores: {len(offs)} offsets, must be 1..{SLIDE_MAX_S}")
    if any(o < 0 or o >= N for o in offs):
        raise _lib.GwwError(f"slide_scores: every offset must be in [0, N = {N})")
    S = len(offs)
    if out is None:
        out = torch.empty((S, N), dtype=torch.float32, device=partials.device)
    elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (S, N) or not out.is_contiguous():
        raise _lib.GwwError(f"slide_scores: out must be a contiguous fp32 GPU tensor of [{S}, {N}]")
    offs_d = torch.tensor(offs, dtype=torch.int64).to(partials.device)
    with torch.cuda.device(partials.device):
        check(lib().gww_slide_scores_f32(partials.data_ptr(), *[t.data_ptr() for t in ps], offs_d.data_ptr(), N, D, S, C,
                                         int(mode), out.data_ptr(), _stream()), "gww_slide_scores_f32")
    return out


def cluster_slides(times, scores, trigger_threshold: float, cluster_threshold: float, cap: int | None = None):
    """``get_clusters`` of every row of ``scores`` fp32 [S, N] against the shared fp64 stamps ``times`` [N]
    (``gww_cluster_slides_f64``, one launch, one wave per slide; no host sync).  Returns (out_t fp64 [S, cap], out_v fp32
    [S, cap], count int32 [S]); a count above ``cap`` (default N, which cannot overflow) means that slide's list was cut."""
    times = _dev(times, torch.float64, "times")
    scores = _dev(scores, torch.float32, "scores")
    if scores.dim() != 2 or scores.shape[1] < 1 or times.shape != (scores.shape[1],):
        raise _lib.GwwError(f"cluster_slides: scores must be [S, N >= 1] and times [N], got {tuple(scores.shape)} and "
                            f"{tuple(times.shape)}")
    S, N = int(scores.shape[0]), int(scores.shape[1])
    if not 1 <= S <= SLIDE_MAX_S:
        raise _lib.GwwError(f"cluster_slides: S={S} slides, must be 1..{SLIDE_MAX_S}")
    cap = N if cap is None else int(cap)
    if cap < 1:
        raise _lib.GwwError(f"cluster_slides: cap={cap} must be >= 1")
    out_t = torch.empty((S, cap), dtype=torch.float64, device=scores.device)
    out_v = torch.empty((S, cap), dtype=torch.float32, device=scores.device)
    cnt = torch.empty((S,), dtype=torch.int32, device=scores.device)
    with torch.cuda.device(scores.device):
        check(lib().gww_cluster_slides_f64(times.data_ptr(), scores.data_ptr(), N, S, float(trigger_threshold),
                                           float(cluster_threshold), out_t.data_ptr(), out_v.data_ptr(), cnt.data_ptr(), cap,
                                           _stream()), "gww_cluster_slides_f64")
    return out_t, out_v, cnt


def det_eval_accumulate(probs, targets, row_loss, correct, loss_sum, n, batches):
    """One batch into the device-resident evaluation state (``gww_det_eval_accumulate``, one launch, no host sync):
    correct int64 [1], loss_sum fp64 [1] (sum of the batches' mean losses), n int64 [1], batches int64 [1]."""
    probs = _dev(probs, torch.float32, "probs")
    targets = _dev(targets, torch.float32, "targets")
    row_loss = _dev(row_loss, torch.float32, "row_loss")
    B, C = probs.shape
    if tuple(targets.shape) != (B, C) or tuple(row_loss.shape) != (B,):
        raise _lib.GwwError("det_eval_accumulate: targets must be [B, C] and row_loss [B]")
    for t, dt, name in ((correct, torch.int64, "correct"), (loss_sum, torch.float64, "loss_sum"), (n, torch.int64, "n"),
                        (batches, torch.int64, "batches")):
        _state(t, dt, (1,), "det_eval_accumulate", name)
    with torch.cuda.device(probs.device):
        check(lib().gww_det_eval_accumulate(probs.data_ptr(), targets.data_ptr(), row_loss.data_ptr(), B, C, correct.data_ptr(),
                                            loss_sum.data_ptr(), n.data_ptr(), batches.data_ptr(), _stream()),
              "gww_det_eval_accumulate")


def score_thresholds(scores, ranks, ws=None):
    """thr fp32 [F] with ``thr[f] = sort(scores)[N - ranks[f]]`` (rank 0: the smallest score, the reference's
    ``noise_outputs[-0]``), selected on the device (``gww_score_thresholds_f32``, no sort, no host sync).  scores fp32 [N],
    ranks int64 [F] on the GPU, F <= 8, every rank in 0..N (the caller's contract: they are device values)."""
    scores = _dev(scores, torch.float32, "scores")
    ranks = _dev(ranks, torch.int64, "ranks")
    if scores.dim() != 1 or ranks.dim() != 1 or scores.numel() < 1 or not 1 <= ranks.numel() <= MAX_FAPS:
        raise _lib.GwwError(f"score_thresholds: scores must be [N >= 1] and ranks [1..{MAX_FAPS}]")
    need = lib().gww_score_thresholds_workspace_bytes()
    if ws is None:
        ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=scores.device)
    if not ws.is_cuda or not ws.is_contiguous():
        raise _lib.GwwError("score_thresholds: ws must be a contiguous GPU tensor")
    thr = torch.empty((ranks.numel(),), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        check(lib().gww_score_thresholds_f32(scores.data_ptr(), scores.numel(), ranks.data_ptr(), ranks.numel(), thr.data_ptr(),
                                             ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
              "gww_score_thresholds_f32")
    return thr


def detection_counts(scores, thr, counts):
    """``counts[f] += #{scores > thr[f]}`` in place (``gww_detection_counts_f32``, one launch, no host sync): scores fp32
    [n], thr fp32 [F], counts a contiguous int64 [F] GPU view, such as one row of an [S, F] table."""
    scores = _dev(scores, torch.float32, "scores")
    thr = _dev(thr, torch.float32, "thr")
    F = thr.numel()
    if scores.dim() != 1 or scores.numel() < 1 or thr.dim() != 1 or not 1 <= F <= MAX_FAPS:
        raise _lib.GwwError(f"detection_counts: scores must be [n >= 1] and thr [1..{MAX_FAPS}]")
    _state(counts, torch.int64, (F,), "detection_counts", "counts")
    with torch.cuda.device(scores.device):
        check(lib().gww_detection_counts_f32(scores.data_ptr(), scores.numel(), thr.data_ptr(), F, counts.data_ptr(), _stream()),
              "gww_detection_counts_f32")


# ---- signal-vs-noise evaluation: ROC curve, AUC, bootstrap band (csrc/roc.hip) ----------------------------------------
ROC_TILE = 16384        # include/gww.h GWW_ROC_TILE: sorted positions of one LDS tile of the bootstrap kernel
ROC_MAX_N = 1 << 24
ROC_MAX_Q = 1024


def _roc_ws(ws, need, device, who):
    if ws is None:
        ws = torch.empty((need,), dtype=torch.uint8, device=device)
    if not ws.is_cuda or not ws.is_contiguous():
        raise _lib.GwwError(f"{who}: ws must be a contiguous GPU tensor")
    return ws


def roc_sort(scores, labels, ws=None):
    """Stable descending sort of the scores on the device (``gww_roc_sort_f32``, no host sync).  scores, labels fp32 [N],
    2 <= N <= 2^24; a label is positive iff it is > 0.5.  Returns (order int32 [N], rank int32 [N], pos uint8 [N],
    gend int32 [N] of which the first G entries are written, G int32 [1], n_nan int32 [1])."""
    scores = _dev(scores, torch.float32, "scores")
    labels = _dev(labels, torch.float32, "labels")
    N = scores.numel()
    if scores.dim() != 1 or tuple(labels.shape) != (N,) or not 2 <= N <= ROC_MAX_N:
        raise _lib.GwwError("roc_sort: scores and labels must be [N] with 2 <= N <= 2^24")
    dev = scores.device
    ws = _roc_ws(ws, lib().gww_roc_sort_workspace_bytes(N), dev, "roc_sort")
    order = torch.empty((N,), dtype=torch.int32, device=dev)
    rank = torch.empty((N,), dtype=torch.int32, device=dev)
    pos = torch.empty((N,), dtype=torch.uint8, device=dev)
    gend = torch.empty((N,), dtype=torch.int32, device=dev)
    G = torch.empty((1,), dtype=torch.int32, device=dev)
    n_nan = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_roc_sort_f32(scores.data_ptr(), labels.data_ptr(), N, order.data_ptr(), rank.data_ptr(), pos.data_ptr(),
                                     gend.data_ptr(), G.data_ptr(), n_nan.data_ptr(), ws.data_ptr(),
                                     ws.numel() * ws.element_size(), _stream()), "gww_roc_sort_f32")
    return order, rank, pos, gend, G, n_nan


def roc_curve(pos, gend, G, ws=None):
    """``sklearn.metrics.roc_curve(drop_intermediate=False)`` and the AUC from the sort's pos / gend / G
    (``gww_roc_curve_f64``, one launch, no host sync).  Returns (fps int64 [N + 1], tps int64 [N + 1], fpr fp64 [N + 1],
    tpr fp64 [N + 1] -- G + 1 entries of each are written --, counts int64 [2] = (P, Nneg), auc fp64 [1])."""
    pos = _dev(pos, torch.uint8, "pos")
    gend = _dev(gend, torch.int32, "gend")
    N = pos.numel()
    if pos.dim() != 1 or tuple(gend.shape) != (N,) or not 2 <= N <= ROC_MAX_N:
        raise _lib.GwwError("roc_curve: pos and gend must be [N] with 2 <= N <= 2^24")
    _state(G, torch.int32, (1,), "roc_curve", "G")
    dev = pos.device
    ws = _roc_ws(ws, lib().gww_roc_curve_workspace_bytes(N), dev, "roc_curve")
    fps = torch.empty((N + 1,), dtype=torch.int64, device=dev)
    tps = torch.empty((N + 1,), dtype=torch.int64, device=dev)
    fpr = torch.empty((N + 1,), dtype=torch.float64, device=dev)
    tpr = torch.empty((N + 1,), dtype=torch.float64, device=dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    auc = torch.empty((1,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_roc_curve_f64(pos.data_ptr(), gend.data_ptr(), G.data_ptr(), N, fps.data_ptr(), tps.data_ptr(),
                                      fpr.data_ptr(), tpr.data_ptr(), counts.data_ptr(), auc.data_ptr(), ws.data_ptr(),
                                      ws.numel() * ws.element_size(), _stream()), "gww_roc_curve_f64")
    return fps, tps, fpr, tpr, counts, auc


def roc_bootstrap_tpr(rank, pos, gend, G, idx, grid, ws=None):
    """The bootstrap replicates' TPR at the grid's FPRs (``gww_roc_bootstrap_tpr_f64``, one workgroup per replicate, no
    host sync): idx int32 [Rc, N] draws from 0..N-1, grid fp64 [Q] ascending in (0, 1], Q <= 1024.  Returns (tpr fp64
    [Rc, Q], valid uint8 [Rc]); a replicate without positives or negatives has valid = 0 and a row of NaN."""
    rank = _dev(rank, torch.int32, "rank")
    pos = _dev(pos, torch.uint8, "pos")
    gend = _dev(gend, torch.int32, "gend")
    idx = _dev(idx, torch.int32, "idx")
    grid = _dev(grid, torch.float64, "grid")
    N = rank.numel()
    if rank.dim() != 1 or tuple(pos.shape) != (N,) or tuple(gend.shape) != (N,) or not 2 <= N <= ROC_MAX_N:
        raise _lib.GwwError("roc_bootstrap_tpr: rank, pos and gend must be [N] with 2 <= N <= 2^24")
    if idx.dim() != 2 or idx.shape[1] != N or not 1 <= idx.shape[0] <= 65535:
        raise _lib.GwwError(f"roc_bootstrap_tpr: idx must be [Rc, N = {N}] with 1 <= Rc <= 65535")
    if grid.dim() != 1 or not 1 <= grid.numel() <= ROC_MAX_Q:
        raise _lib.GwwError(f"roc_bootstrap_tpr: grid must be [Q] with 1 <= Q <= {ROC_MAX_Q}")
    _state(G, torch.int32, (1,), "roc_bootstrap_tpr", "G")
    Rc, Q, dev = idx.shape[0], grid.numel(), rank.device
    ws = _roc_ws(ws, lib().gww_roc_bootstrap_workspace_bytes(Rc, N), dev, "roc_bootstrap_tpr")
    tpr = torch.empty((Rc, Q), dtype=torch.float64, device=dev)
    valid = torch.empty((Rc,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_roc_bootstrap_tpr_f64(rank.data_ptr(), pos.data_ptr(), gend.data_ptr(), G.data_ptr(), idx.data_ptr(), Rc,
                                              N, grid.data_ptr(), Q, tpr.data_ptr(), valid.data_ptr(), ws.data_ptr(),
                                              ws.numel() * ws.element_size(), _stream()), "gww_roc_bootstrap_tpr_f64")
    return tpr, valid


def roc_band(tpr, valid):
    """(mean fp64 [Q], std fp64 [Q], n_valid int32 [1]) of tpr [R, Q] over the rows with valid != 0, summed in row order as
    ``np.mean(axis=0)`` / ``np.std(axis=0)`` do (``gww_roc_band_f64``, one launch, no host sync)."""
    tpr = _dev(tpr, torch.float64, "tpr")
    valid = _dev(valid, torch.uint8, "valid")
    if tpr.dim() != 2 or tpr.shape[0] < 1 or tuple(valid.shape) != (tpr.shape[0],) or not 1 <= tpr.shape[1] <= ROC_MAX_Q:
        raise _lib.GwwError(f"roc_band: tpr must be [R >= 1, Q <= {ROC_MAX_Q}] and valid [R]")
    R, Q = tpr.shape
    mean = torch.empty((Q,), dtype=torch.float64, device=tpr.device)
    std = torch.empty((Q,), dtype=torch.float64, device=tpr.device)
    n_valid = torch.empty((1,), dtype=torch.int32, device=tpr.device)
    with torch.cuda.device(tpr.device):
        check(lib().gww_roc_band_f64(tpr.data_ptr(), valid.data_ptr(), R, Q, mean.data_ptr(), std.data_ptr(), n_valid.data_ptr(),
                                     _stream()), "gww_roc_band_f64")
    return mean, std, n_valid


def binary_eval_accumulate(logits, labels, scores, offset: int, loss_sum, batches, confusion):
    """One batch into the device-resident state of a binary evaluation (``gww_binary_eval_accumulate``, one launch, no
    host sync): ``scores[offset : offset + B] = sigmoid(logits)``, loss_sum fp64 [1] += the batch-mean
    BCEWithLogitsLoss, batches int64 [1] += 1, confusion int64 [2, 2] (rows = the label) += the rows by
    ``torch.round(sigmoid)``."""
    logits = _dev(logits, torch.float32, "logits").reshape(-1)
    labels = _dev(labels, torch.float32, "labels").reshape(-1)
    B = logits.numel()
    if labels.numel() != B or B < 1:
        raise _lib.GwwError("binary_eval_accumulate: logits and labels must hold the same B >= 1 elements")
    if not scores.is_cuda or scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous():
        raise _lib.GwwError("binary_eval_accumulate: scores must be a contiguous GPU torch.float32 tensor [n]")
    if not 0 <= int(offset) <= scores.numel() - B:
        raise _lib.GwwError(f"binary_eval_accumulate: offset={offset} + B={B} exceeds the {scores.numel()} scores")
    _state(loss_sum, torch.float64, (1,), "binary_eval_accumulate", "loss_sum")
    _state(batches, torch.int64, (1,), "binary_eval_accumulate", "batches")
    _state(confusion, torch.int64, (2, 2), "binary_eval_accumulate", "confusion")
    with torch.cuda.device(logits.device):
        check(lib().gww_binary_eval_accumulate(logits.data_ptr(), labels.data_ptr(), B, scores.data_ptr(), int(offset),
                                               scores.numel(), loss_sum.data_ptr(), batches.data_ptr(), confusion.data_ptr(),
                                               _stream()), "gww_binary_eval_accumulate")


# ---- scoring a search: false-alarm rate and sensitive volume (csrc/score.hip) -------------------------------------------
SCORE_MAX_N = 1 << 27


def _score_count(n_dev, who):
    if n_dev is None:
        return 0
    _state(n_dev, torch.int32, (1,), who, "the device count")
    return n_dev.data_ptr()


def score_sort(keys, n_dev=None, ws=None):
    """Stable ascending sort of fp64 keys [n], 1 <= n <= 2^27, on the device (``gww_score_sort_f64``, no host sync).
    ``n_dev`` int32 [1] on the device: sort the first ``n_dev[0]`` keys only.  Returns (order int32 [n] =
    ``np.argsort(keys, kind="stable")``, sorted fp64 [n], n_nan int32 [1])."""
    keys = _dev(keys, torch.float64, "keys")
    n = keys.numel()
    if keys.dim() != 1 or not 1 <= n <= SCORE_MAX_N:
        raise _lib.GwwError(f"score_sort: keys must be [n] with 1 <= n <= 2^27, got {tuple(keys.shape)}")
    dev = keys.device
    cnt = _score_count(n_dev, "score_sort")
    ws = _roc_ws(ws, lib().gww_score_sort_workspace_bytes(n), dev, "score_sort")
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    n_nan = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_score_sort_f64(keys.data_ptr(), n, cnt, out.data_ptr(), order.data_ptr(), n_nan.data_ptr(),
                                       ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), "gww_score_sort_f64")
    return order, out, n_nan


def score_closest(tc, t):
    """``find_closest_index`` of the values t fp64 [n] in the ascending tc fp64 [N] (``gww_score_closest_f64``, one launch,
    no host sync).  Returns (idx int32 [n], diff fp64 [n] = |tc[idx] - t|)."""
    tc = _dev(tc, torch.float64, "tc")
    t = _dev(t, torch.float64, "t")
    if tc.dim() != 1 or t.dim() != 1 or not 1 <= tc.numel() <= SCORE_MAX_N or not 1 <= t.numel() <= SCORE_MAX_N:
        raise _lib.GwwError("score_closest: tc must be [N] and t [n] with 1 <= N, n <= 2^27")
    idx = torch.empty((t.numel(),), dtype=torch.int32, device=t.device)
    diff = torch.empty((t.numel(),), dtype=torch.float64, device=t.device)
    with torch.cuda.device(t.device):
        check(lib().gww_score_closest_f64(tc.data_ptr(), tc.numel(), t.data_ptr(), t.numel(), idx.data_ptr(), diff.data_ptr(),
                                          _stream()), "gww_score_closest_f64")
    return idx, diff


def score_match(events, order, tc, ws=None):
    """Events against injections (``gww_score_match_f64``, no host sync): events fp64 [3, E] (time, stat, var), order int32
    [E] from ``score_sort(events[0])``, tc fp64 [N] ascending.  Returns a dict of device tensors: ``fg_sorted`` [3, E],
    ``found_idx`` [E], ``tp_idx`` / ``fp_idx`` [E], ``tp_diff`` / ``fp_diff`` [E], ``tp_events`` / ``fp_events`` [3, E],
    ``found_inj`` / ``found_stat`` / ``missed`` [N] and ``counts`` int32 [5] = (true positives, false positives, found,
    missed, events with a NaN): the leading ``counts`` entries (columns) of the compacted buffers are written."""
    events = _dev(events, torch.float64, "events")
    order = _dev(order, torch.int32, "order")
    tc = _dev(tc, torch.float64, "tc")
    if events.dim() != 2 or events.shape[0] != 3 or not 1 <= events.shape[1] <= SCORE_MAX_N:
        raise _lib.GwwError(f"score_match: events must be [3, E] with 1 <= E <= 2^27, got {tuple(events.shape)}")
    E, N = events.shape[1], tc.numel()
    if tuple(order.shape) != (E,) or tc.dim() != 1 or not 1 <= N <= SCORE_MAX_N:
        raise _lib.GwwError(f"score_match: order must be [E = {E}] and tc [N] with 1 <= N <= 2^27")
    dev = events.device
    ws = _roc_ws(ws, lib().gww_score_match_workspace_bytes(E, N), dev, "score_match")
    f64, i32 = torch.float64, torch.int32
    r = {"fg_sorted": torch.empty((3, E), dtype=f64, device=dev), "found_idx": torch.empty((E,), dtype=i32, device=dev),
         "tp_idx": torch.empty((E,), dtype=i32, device=dev), "fp_idx": torch.empty((E,), dtype=i32, device=dev),
         "tp_diff": torch.empty((E,), dtype=f64, device=dev), "fp_diff": torch.empty((E,), dtype=f64, device=dev),
         "tp_events": torch.empty((3, E), dtype=f64, device=dev), "fp_events": torch.empty((3, E), dtype=f64, device=dev),
         "found_inj": torch.empty((N,), dtype=i32, device=dev), "found_stat": torch.empty((N,), dtype=f64, device=dev),
         "missed": torch.empty((N,), dtype=i32, device=dev), "counts": torch.empty((5,), dtype=i32, device=dev)}
    with torch.cuda.device(dev):
        check(lib().gww_score_match_f64(events.data_ptr(), order.data_ptr(), E, tc.data_ptr(), N, r["fg_sorted"].data_ptr(),
                                        r["found_idx"].data_ptr(), r["tp_idx"].data_ptr(), r["fp_idx"].data_ptr(),
                                        r["tp_diff"].data_ptr(), r["fp_diff"].data_ptr(), r["tp_events"].data_ptr(),
                                        r["fp_events"].data_ptr(), r["found_inj"].data_ptr(), r["found_stat"].data_ptr(),
                                        r["missed"].data_ptr(), r["counts"].data_ptr(), ws.data_ptr(),
                                        ws.numel() * ws.element_size(), _stream()), "gww_score_match_f64")
    return r


def score_far(n: int, duration: float, device, n_dev=None):
    """far fp64 [n] with far[k] = (m - k - 1) / duration for k < m (``gww_score_far_f64``, one launch, no host sync); m = n,
    or the device's count ``n_dev`` int32 [1] (then m entries are written)."""
    if not 1 <= int(n) <= SCORE_MAX_N:
        raise _lib.GwwError(f"score_far: n={n} must be 1..2^27")
    cnt = _score_count(n_dev, "score_far")
    far = torch.empty((int(n),), dtype=torch.float64, device=device)
    with torch.cuda.device(far.device):
        check(lib().gww_score_far_f64(cnt, int(n), float(duration), far.data_ptr(), _stream()), "gww_score_far_f64")
    return far


def score_suffix(w1, w2, found_inj, order, F):
    """Suffix sums of the per-injection weights w1, w2 fp64 [N] gathered in found-statistic order
    (``gww_score_suffix_f64``, one workgroup, no host sync): found_inj, order int32 [N], F int32 [1] on the device.
    Returns (cs1, cs2) fp64 [N + 1] of which F + 1 entries are written, cs[F] = 0."""
    w1 = _dev(w1, torch.float64, "w1")
    w2 = _dev(w2, torch.float64, "w2")
    found_inj = _dev(found_inj, torch.int32, "found_inj")
    order = _dev(order, torch.int32, "order")
    N = w1.numel()
    if w1.dim() != 1 or not 1 <= N <= SCORE_MAX_N or any(tuple(t.shape) != (N,) for t in (w2, found_inj, order)):
        raise _lib.GwwError("score_suffix: w1, w2, found_inj and order must be [N] with 1 <= N <= 2^27")
    _state(F, torch.int32, (1,), "score_suffix", "F")
    cs1 = torch.empty((N + 1,), dtype=torch.float64, device=w1.device)
    cs2 = torch.empty((N + 1,), dtype=torch.float64, device=w1.device)
    with torch.cuda.device(w1.device):
        check(lib().gww_score_suffix_f64(w1.data_ptr(), w2.data_ptr(), N, found_inj.data_ptr(), order.data_ptr(), F.data_ptr(),
                                         cs1.data_ptr(), cs2.data_ptr(), _stream()), "gww_score_suffix_f64")
    return cs1, cs2


def score_volume(found_sorted, F, noise_sorted, n_inj: float, prefactor: float, cs1=None, cs2=None):
    """Per ascending background statistic (``gww_score_volume_f64``, one launch, no host sync): found_sorted fp64 [N] of
    which F (int32 [1], device) entries count, noise_sorted fp64 [B].  Returns (nfound int64 [B], fraction, volume,
    volume_err fp64 [B]); with cs1, cs2 from ``score_suffix`` the chirp-mass-weighted form."""
    found_sorted = _dev(found_sorted, torch.float64, "found_sorted")
    noise_sorted = _dev(noise_sorted, torch.float64, "noise_sorted")
    N, B = found_sorted.numel(), noise_sorted.numel()
    if found_sorted.dim() != 1 or noise_sorted.dim() != 1 or not 1 <= N <= SCORE_MAX_N or not 1 <= B <= SCORE_MAX_N:
        raise _lib.GwwError("score_volume: found_sorted must be [N] and noise_sorted [B] with 1 <= N, B <= 2^27")
    _state(F, torch.int32, (1,), "score_volume", "F")
    if (cs1 is None) != (cs2 is None):
        raise _lib.GwwError("score_volume: cs1 and cs2 come together")
    if cs1 is not None:
        _state(cs1, torch.float64, (N + 1,), "score_volume", "cs1")
        _state(cs2, torch.float64, (N + 1,), "score_volume", "cs2")
    dev = noise_sorted.device
    nfound = torch.empty((B,), dtype=torch.int64, device=dev)
    frac = torch.empty((B,), dtype=torch.float64, device=dev)
    vol = torch.empty((B,), dtype=torch.float64, device=dev)
    err = torch.empty((B,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_score_volume_f64(found_sorted.data_ptr(), F.data_ptr(), N, noise_sorted.data_ptr(), B, float(n_inj),
                                         float(prefactor), 0 if cs1 is None else cs1.data_ptr(),
                                         0 if cs2 is None else cs2.data_ptr(), nfound.data_ptr(), frac.data_ptr(),
                                         vol.data_ptr(), err.data_ptr(), _stream()), "gww_score_volume_f64")
    return nfound, frac, vol, err


# ---- the efficiency study's test stage: triggers, events, ranking steps (csrc/trigger_stats.hip) -------------------------
TRIG_MAX_N = 1 << 27


def _trig_vec(t, n, who, name):
    t = _dev(t, torch.float64, name)
    if tuple(t.shape) != (n,):
        raise _lib.GwwError(f"{who}: {name} must be fp64 [{n}], got {tuple(t.shape)}")
    return t


def trig_triggers(series, delta_t: float, epoch: float, threshold: float, cap=None, ws=None):
    """The samples of ``series`` (fp32 or fp64 [n], 1 <= n <= 2^27) above ``threshold``, in order
    (``gww_trig_triggers_f64``, 4 launches, no host sync).  Returns (times fp64 [cap], values fp64 [cap], counts int32 [2] =
    (triggers, NaN samples)): the first min(counts[0], cap) entries are written; cap defaults to n."""
    if not series.is_cuda:
        raise _lib.GwwError(f"trig_triggers: series must live on the GPU (got {series.device}); gw_whisper_amd has no CPU path")
    if series.dtype not in (torch.float32, torch.float64):
        raise _lib.GwwError(f"trig_triggers: series must be torch.float32 or torch.float64, got {series.dtype}")
    series = series.contiguous()
    n = series.numel()
    if series.dim() != 1 or not 1 <= n <= TRIG_MAX_N:
        raise _lib.GwwError(f"trig_triggers: series must be [n] with 1 <= n <= 2^27, got {tuple(series.shape)}")
    cap = n if cap is None else int(cap)
    if not 1 <= cap <= n:
        raise _lib.GwwError(f"trig_triggers: cap={cap} must be 1..n = {n}")
    dev = series.device
    ws = _roc_ws(ws, lib().gww_trig_triggers_workspace_bytes(n), dev, "trig_triggers")
    times = torch.empty((cap,), dtype=torch.float64, device=dev)
    values = torch.empty((cap,), dtype=torch.float64, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_trig_triggers_f64(series.data_ptr(), int(series.dtype == torch.float64), n, cap, float(delta_t),
                                          float(epoch), float(threshold), times.data_ptr(), values.data_ptr(),
                                          counts.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
              "gww_trig_triggers_f64")
    return times, values, counts


def trig_events(times, values, tolerance: float, n_dev=None, ws=None):
    """Clusters of the ascending trigger times (a gap >= ``tolerance`` opens one) and per cluster the time and value of its
    first maximum (``gww_trig_events_f64``, 4 launches, no host sync).  times, values fp64 [cap]; ``n_dev`` int32 [1]: the
    device's trigger count.  Returns (ev_times [cap], ev_values [cap], counts int32 [2] = (events, NaN values))."""
    times = _dev(times, torch.float64, "times")
    cap = times.numel()
    if times.dim() != 1 or not 1 <= cap <= TRIG_MAX_N:
        raise _lib.GwwError(f"trig_events: times must be [cap] with 1 <= cap <= 2^27, got {tuple(times.shape)}")
    values = _trig_vec(values, cap, "trig_events", "values")
    cnt = _score_count(n_dev, "trig_events")
    dev = times.device
    ws = _roc_ws(ws, lib().gww_trig_events_workspace_bytes(cap), dev, "trig_events")
    ev_t = torch.empty((cap,), dtype=torch.float64, device=dev)
    ev_v = torch.empty((cap,), dtype=torch.float64, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_trig_events_f64(times.data_ptr(), values.data_ptr(), cnt, cap, float(tolerance), ev_t.data_ptr(),
                                        ev_v.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                                        _stream()), "gww_trig_events_f64")
    return ev_t, ev_v, counts


def trig_split(values, diff, tolerance: float, n_dev=None, ws=None):
    """The event values split by ``diff <= tolerance`` (``gww_trig_split_f64``, 4 launches, no host sync): values, diff fp64
    [cap].  Returns (tp_values [cap], fp_values [cap], counts int32 [3] = (true positives, false positives, NaN values))."""
    values = _dev(values, torch.float64, "values")
    cap = values.numel()
    if values.dim() != 1 or not 1 <= cap <= TRIG_MAX_N:
        raise _lib.GwwError(f"trig_split: values must be [cap] with 1 <= cap <= 2^27, got {tuple(values.shape)}")
    diff = _trig_vec(diff, cap, "trig_split", "diff")
    cnt = _score_count(n_dev, "trig_split")
    dev = values.device
    ws = _roc_ws(ws, lib().gww_trig_split_workspace_bytes(cap), dev, "trig_split")
    tp = torch.empty((cap,), dtype=torch.float64, device=dev)
    fp = torch.empty((cap,), dtype=torch.float64, device=dev)
    counts = torch.empty((3,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_trig_split_f64(values.data_ptr(), diff.data_ptr(), cnt, cap, float(tolerance), tp.data_ptr(),
                                       fp.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                                       _stream()), "gww_trig_split_f64")
    return tp, fp, counts


def trig_steps(fp_sorted, n_fp, tp_sorted, n_tp, duration: float, prefactor: float, n_inj: float, ws=None):
    """The ranking steps over the ascending false-positive values (``gww_trig_steps_f64``, 4 launches, no host sync):
    fp_sorted fp64 [cap] of which n_fp (int32 [1], device) count, tp_sorted fp64 [cap_tp] of which n_tp count.  Returns
    (ranking, far, sens_frac, sens_vol, sens_vol_err fp64 [cap], n_steps int32 [1])."""
    fp_sorted = _dev(fp_sorted, torch.float64, "fp_sorted")
    tp_sorted = _dev(tp_sorted, torch.float64, "tp_sorted")
    cap, cap_tp = fp_sorted.numel(), tp_sorted.numel()
    if fp_sorted.dim() != 1 or tp_sorted.dim() != 1 or not 1 <= cap <= TRIG_MAX_N or not 1 <= cap_tp <= TRIG_MAX_N:
        raise _lib.GwwError("trig_steps: fp_sorted must be [cap] and tp_sorted [cap_tp] with 1 <= cap, cap_tp <= 2^27")
    _state(n_fp, torch.int32, (1,), "trig_steps", "n_fp")
    _state(n_tp, torch.int32, (1,), "trig_steps", "n_tp")
    dev = fp_sorted.device
    ws = _roc_ws(ws, lib().gww_trig_steps_workspace_bytes(cap), dev, "trig_steps")
    outs = [torch.empty((cap,), dtype=torch.float64, device=dev) for _ in range(5)]
    n_steps = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_trig_steps_f64(fp_sorted.data_ptr(), n_fp.data_ptr(), cap, tp_sorted.data_ptr(), n_tp.data_ptr(), cap_tp,
                                       float(duration), float(prefactor), float(n_inj), *[o.data_ptr() for o in outs],
                                       n_steps.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
              "gww_trig_steps_f64")
    return (*outs, n_steps)


# ---- coincidences of two detectors' events at zero lag and under time slides (csrc/coinc.hip) ----------------------------
COINC_MAX_N, COINC_MAX_S = 1 << 27, 65535


def _coinc_events(t, v, n, who, g):
    """(t, v, capacity, address of the device's count or 0) of detector g's event list"""
    t = _dev(t, torch.float64, f"t{g}")
    v = _dev(v, torch.float32, f"v{g}")
    if t.dim() != 1 or v.shape != t.shape or t.numel() > COINC_MAX_N:
        raise _lib.GwwError(f"{who}: t{g} must be fp64 [cap <= 2^27] and v{g} fp32 of the same shape, got {tuple(t.shape)} and "
                            f"{tuple(v.shape)}")
    if torch.is_tensor(n):
        _state(n, torch.int32, (1,), who, f"the device count n{g}")
        return t, v, t.numel(), n.data_ptr()
    n = int(n)
    if not 0 <= n <= t.numel():
        raise _lib.GwwError(f"{who}: n{g}={n} must be 0..{t.numel()}, the length of t{g}")
    return t, v, n, 0


def coinc_slides(t0, v0, n0, t1, v1, n1, shifts, window: float, cap_total: int | None = None):
    """Coincidences of detector 0's events (``t0`` fp64 ascending, ``v0`` fp32) with detector 1's under every shift of
    ``shifts`` fp64 [S] (seconds added to ``t1``; 0.0 is zero lag): ``gww_coinc_count_f64``, ``gww_coinc_offsets``,
    ``gww_coinc_emit_f64``, three launches.  ``n0`` / ``n1``: python ints (the first n events count) or int32 [1] tensors on
    the device (the count is read there, clamped to the length).  Events i, j are coincident iff
    ``fabs((t1[j] + shift) - t0[i]) <= window``; i's partner is the coincident j of the largest ``v1``, then the smallest
    ``fabs(dt)``, then the smallest j.  Returns a dict of device tensors: ``offsets`` int64 [S + 1] (slide s owns entries
    ``offsets[s] .. offsets[s + 1] - 1``, in ascending i) and ``time`` = t0[i], ``stat`` = double(v0[i]) + double(v1[j]),
    ``dt`` fp64, ``idx0`` = i, ``idx1`` = j int32.
    ``cap_total=None``: the 8-byte total ``offsets[S]`` is read back -- ONE host synchronisation -- and the result has exactly
    that many entries.  With ``cap_total`` nothing is read: the buffers have ``cap_total`` entries, the first
    ``min(offsets[S], cap_total)`` are written, and ``offsets`` holds the true totals whether or not the list was cut."""
    who = "coinc_slides"
    t0, v0, cap0, n0_dev = _coinc_events(t0, v0, n0, who, 0)
    t1, v1, cap1, n1_dev = _coinc_events(t1, v1, n1, who, 1)
    shifts = _dev(shifts, torch.float64, "shifts")
    S = shifts.numel()
    if shifts.dim() != 1 or not 1 <= S <= COINC_MAX_S:
        raise _lib.GwwError(f"{who}: shifts must be fp64 [S] with 1 <= S <= {COINC_MAX_S}, got {tuple(shifts.shape)}")
    window = float(window)
    if not window >= 0.0:
        raise _lib.GwwError(f"{who}: window={window} must not be negative")
    if cap_total is not None and int(cap_total) < 0:
        raise _lib.GwwError(f"{who}: cap_total={cap_total} must not be negative")
    dev = t0.device
    nb = int(lib().gww_coinc_blocks(cap0))
    partner = torch.empty((S, cap0), dtype=torch.int32, device=dev)
    blocks = torch.empty((S * nb,), dtype=torch.int64, device=dev)
    offsets = torch.empty((S + 1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gww_coinc_count_f64(t0.data_ptr(), n0_dev, cap0, t1.data_ptr(), v1.data_ptr(), n1_dev, cap1,
                                        shifts.data_ptr(), S, window, partner.data_ptr(), blocks.data_ptr(), _stream()),
              "gww_coinc_count_f64")
        check(lib().gww_coinc_offsets(blocks.data_ptr(), cap0, S, offsets.data_ptr(), _stream()), "gww_coinc_offsets")
        cap = int(offsets[S].item()) if cap_total is None else int(cap_total)     # the one host read
        f64, i32 = torch.float64, torch.int32
        r = {"time": torch.empty((cap,), dtype=f64, device=dev), "stat": torch.empty((cap,), dtype=f64, device=dev),
             "dt": torch.empty((cap,), dtype=f64, device=dev), "idx0": torch.empty((cap,), dtype=i32, device=dev),
             "idx1": torch.empty((cap,), dtype=i32, device=dev), "offsets": offsets}
        check(lib().gww_coinc_emit_f64(t0.data_ptr(), v0.data_ptr(), n0_dev, cap0, t1.data_ptr(), v1.data_ptr(), n1_dev, cap1,
                                       shifts.data_ptr(), S, partner.data_ptr(), blocks.data_ptr(), cap, r["time"].data_ptr(),
                                       r["stat"].data_ptr(), r["dt"].data_ptr(), r["idx0"].data_ptr(), r["idx1"].data_ptr(),
                                       _stream()), "gww_coinc_emit_f64")
    return r
