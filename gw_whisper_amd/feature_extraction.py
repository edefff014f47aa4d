"""``WhisperFeatureExtractor``-compatible callable backed by the HIP log-mel kernel.

Mirrors the call surface the reference uses:

    fe = WhisperFeatureExtractor.from_pretrained(f"openai/whisper-{enc}")     # src/dataset.py:12
    x = fe(audio, sampling_rate=16000, return_tensors="pt").input_features    # src/dataset.py:20-21
    x = fe([a0, a1, ...], sampling_rate=16000, return_tensors="pt")           # Efficiency_test/src/tools.py:125

Same argument meaning and error behaviour as HF
(``HF:models/whisper/feature_extraction_whisper.py:193-346``): ``ValueError`` when
``sampling_rate`` differs from the configured rate (16000 by default), zero-pad / truncate to ``chunk_length`` seconds
(30 by default), always returns a batch.

Two entry points of libgww.so do the arithmetic, chosen by ``device`` (constructor or call):

* ``"cpu"`` -- the default, and what HF itself is: ``gww_logmel_host_f32``, plain C++ with no HIP call.  It is
  fork-safe, so the reference's ``dataset.py`` works unchanged inside its forked ``DataLoader`` workers
  (``Signal_vs_Noise/src/train.py:224-225``, ``--num_workers 12``);
* ``"cuda"`` (or a CUDA tensor as input) -- the HIP kernels (``gww_logmel_f32``), the batched variant SURVEY.md
  section 8b calls the additional entry point; ``return_device="cuda"`` keeps the features on the GPU and skips
  the PCIe round trip.

Neither is a fallback of the other and neither is torch / numpy: a missing ``libgww.so`` raises ``GwwError``.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


class BatchFeature(dict):
    """Minimal stand-in for ``transformers.BatchFeature``: dict + attribute access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class WhisperFeatureExtractor:
    """HF's constructor: ``feature_size`` mel bins, ``sampling_rate`` Hz, an ``n_fft``-point window every ``hop_length``
    samples, chunks of ``chunk_length`` seconds.  The defaults are Whisper's published configuration, which runs the
    kernels written for it; every other supported configuration (include/gww.h: ``gww_frontend_cfg``) runs the general
    ones.  ``min_frequency`` / ``max_frequency`` are the band of the mel filterbank: HF fixes 0 .. 8000 Hz, which at a
    low sampling rate leaves the filters above the Nyquist frequency empty -- pass ``max_frequency=sampling_rate / 2``."""
    model_input_names = ["input_features"]

    def __init__(self, feature_size=80, sampling_rate=16000, hop_length=160, chunk_length=30, n_fft=400,
                 padding_value=0.0, device="cpu", min_frequency=0.0, max_frequency=8000.0, **kwargs):
        for name, v in (("feature_size", feature_size), ("sampling_rate", sampling_rate), ("hop_length", hop_length),
                        ("chunk_length", chunk_length), ("n_fft", n_fft)):
            if int(v) != v:
                raise ValueError(f"WhisperFeatureExtractor: {name}={v!r} must be an integer")
        if chunk_length < 1:
            raise ValueError(f"WhisperFeatureExtractor: chunk_length={chunk_length} must be at least 1")
        self.feature_size = int(feature_size)
        self.sampling_rate = int(sampling_rate)
        self.hop_length = int(hop_length)
        self.chunk_length = int(chunk_length)
        self.n_fft = int(n_fft)
        self.min_frequency = float(min_frequency)
        self.max_frequency = float(max_frequency)
        self.n_samples = self.chunk_length * self.sampling_rate
        config = ops.FrontendConfig(self.feature_size, self.sampling_rate, self.n_fft, self.hop_length, self.n_samples,
                                    self.min_frequency, self.max_frequency)
        try:
            ops.frontend_validate(config)
        except _lib.GwwError as e:
            # the library's names (n_mels, n_samples = chunk_length * sampling_rate, n_frames = n_samples // hop_length)
            raise ValueError(f"WhisperFeatureExtractor: unsupported configuration: {e}") from None
        self.nb_max_frames = self.n_samples // self.hop_length
        self.padding_value = padding_value
        self.device = device
        # the published configuration keeps the entry points (and handles) it always had
        self._config = None if config.is_published else config

    @property
    def frontend_config(self):
        """What ``ops.logmel`` / ``ops.logmel_host`` take as ``config`` to compute this extractor's features: an
        ``ops.FrontendConfig``, or ``None`` for Whisper's published configuration (the entry points without one)."""
        return self._config

    @property
    def mel_filters(self) -> np.ndarray:
        """HF's attribute: float32 ``[n_fft // 2 + 1, feature_size]``, the filterbank both twins multiply with."""
        c = self._config or ops.FrontendConfig(n_mels=self.feature_size)
        return np.ascontiguousarray(ops.mel_filters(c).T)

    _HF_KEYS = ("feature_size", "sampling_rate", "hop_length", "chunk_length", "n_fft", "padding_value")
    _OWN_KEYS = ("min_frequency", "max_frequency")

    def to_dict(self) -> dict:
        """The fields of a ``preprocessor_config.json``: HF's keys as HF writes them, and the two frequency keys."""
        d = {k: getattr(self, k) for k in self._HF_KEYS + self._OWN_KEYS}
        d.update(n_samples=self.n_samples, nb_max_frames=self.nb_max_frames, padding_side="right",
                 return_attention_mask=False, feature_extractor_type="WhisperFeatureExtractor")
        return d

    def save_pretrained(self, save_directory: str):
        """Write ``preprocessor_config.json``: ``transformers.WhisperFeatureExtractor.from_pretrained`` of the directory
        gives the same HF fields (the frequency keys are extra attributes there)."""
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        path = os.path.join(save_directory, "preprocessor_config.json")
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)
            f.write("\n")
        return [path]

    @classmethod
    def from_pretrained(cls, name_or_path=None, **kwargs):
        """Every published ``openai/whisper-*`` preprocessor_config.json is this class's default except those of
        large-v3 and large-v3-turbo, which set ``feature_size`` 128.  A local directory's (or file's)
        ``preprocessor_config.json`` is read for every field of the constructor.  Nothing is downloaded; keyword
        arguments override, as in HF."""
        import json
        import os
        if name_or_path is not None:
            path = os.fspath(name_or_path)
            cfg = os.path.join(path, "preprocessor_config.json") if os.path.isdir(path) else path
            if os.path.isfile(cfg):
                with open(cfg) as f:
                    j = json.load(f)
                for k in cls._HF_KEYS + cls._OWN_KEYS:
                    if k in j and k not in kwargs:
                        kwargs[k] = j[k]
            elif "feature_size" not in kwargs and \
                    path.rstrip("/").split("/")[-1] in ("whisper-large-v3", "whisper-large-v3-turbo"):
                kwargs["feature_size"] = 128
        return cls(**kwargs)

    def __call__(self, raw_speech, truncation=True, pad_to_multiple_of=None, return_tensors=None,
                 return_attention_mask=None, padding="max_length", max_length=None, sampling_rate=None,
                 do_normalize=None, device=None, return_device="cpu", **kwargs):
        if sampling_rate is not None and sampling_rate != self.sampling_rate:
            raise ValueError(
                f"The model corresponding to this feature extractor: {self.__class__.__name__} was trained using a"
                f" sampling rate of {self.sampling_rate}. Please make sure that the provided `raw_speech` input"
                f" was sampled with {self.sampling_rate} and not {sampling_rate}.")
        if do_normalize or return_attention_mask or padding != "max_length" or max_length is not None:
            raise NotImplementedError("only the default padding='max_length' path the reference uses is implemented")
        if device is None:
            device = raw_speech.device if isinstance(raw_speech, torch.Tensor) and raw_speech.is_cuda else self.device
        dev = torch.device(device)
        if isinstance(raw_speech, torch.Tensor):
            wave = raw_speech.to(dev, torch.float32)
            if wave.dim() == 1:
                wave = wave[None]
        else:
            is_batched_numpy = isinstance(raw_speech, np.ndarray) and raw_speech.ndim > 1
            if is_batched_numpy and raw_speech.ndim > 2:
                raise ValueError(f"Only mono-channel audio is supported for input to {self}")
            is_batched = is_batched_numpy or (isinstance(raw_speech, (list, tuple))
                                              and isinstance(raw_speech[0], (np.ndarray, tuple, list)))
            if is_batched:
                rows = [np.asarray(r, dtype=np.float32).reshape(-1) for r in raw_speech]
            else:
                rows = [np.asarray(raw_speech, dtype=np.float32).reshape(-1)]
            n = min(max(len(r) for r in rows), self.n_samples)      # HF truncates at chunk_length
            host = np.zeros((len(rows), max(n, 1)), dtype=np.float32)   # ragged rows: zero fill == HF's padding
            for i, r in enumerate(rows):
                m = min(len(r), n)
                host[i, :m] = r[:m]
            wave = torch.from_numpy(host).to(dev)
        feats = (ops.logmel(wave, n_mels=self.feature_size, config=self._config) if dev.type == "cuda"
                 else ops.logmel_host(wave, n_mels=self.feature_size, config=self._config))
        if return_device == "cpu":
            feats = feats.cpu()
        if return_tensors == "np":
            feats = feats.cpu().numpy()
        elif return_tensors not in (None, "pt"):
            raise ValueError(f"unsupported return_tensors={return_tensors!r}")
        elif return_tensors is None:
            feats = [f for f in feats.cpu().numpy()]
        elif return_device != "cpu":
            feats = feats.to(return_device)
        return BatchFeature({"input_features": feats})
