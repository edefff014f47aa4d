#!/usr/bin/env python3
"""Golden vectors of the configurable front end and of a short-context encoder, from HuggingFace ``transformers``.

    python tools/make_golden_frontend.py     # writes tests/golden/frontend_configs.npz and short_context_hf.npz

Runs on the CPU; nothing is downloaded; only OUTPUTS, filterbanks and the seeds that regenerate the inputs are stored.

``frontend_configs.npz`` -- per configuration ``i`` of ``CONFIGS`` (mels, rate, hop, chunk, n_fft, input samples, fmax):
  cfg<i>        the seven numbers
  hf<i>         ``WhisperFeatureExtractor(feature_size, sampling_rate, hop_length, chunk_length, n_fft)``'s
                ``_np_extract_fbank_features`` of the zero-padded input, frames [0, keep) as float32 [N_SEG, mels, keep]:
                keep = min(n_frames, live + 3); every later frame of a row equals ...
  pad<i>        ... this value, float32 [N_SEG] (checked here before it is relied on)
  fb<i>         the filterbank HF multiplies with, float64 [n_fft // 2 + 1, mels]: the extractor's own, or
                ``transformers.audio_utils.mel_filter_bank(..., max_frequency=fmax, ...)`` set as its ``mel_filters``
                where fmax is not HF's 8000 Hz
  near<i>       how many live elements lie within 0.01 (log10) of the ``max - 8`` floor (0 for these seeds)
The input is ``waves(i)``: seeded white noise, which the tests regenerate.

``short_context_hf.npz`` -- HF's ``WhisperEncoder`` in float64 with ``max_source_positions`` 100 (d 128, 2 layers,
2 heads, ffn 512) on ``gw_whisper_amd.synth`` weights (rows 0 .. 99 of the position table) and a seeded input:
``last_hidden_state`` float64 [2, 100, 128] and ``config`` (d, L, H, F, T, weight seed, input seed).
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLD = os.path.join(ROOT, "tests", "golden")
N_SEG = 2
# (mels, rate, hop, chunk, n_fft, input samples, fmax)
CONFIGS = (
    (80, 2048, 16, 2, 128, 2048, 8000),      # 52 of 80 filters above the Nyquist frequency: empty
    (80, 2048, 16, 2, 128, 2048, 1024),
    (80, 16000, 160, 2, 400, 16000, 8000),   # Whisper's window on a 2 s chunk
    (80, 16000, 160, 1, 400, 16000, 8000),   # no dead frame at all
    (128, 4000, 25, 1, 250, 3000, 2000),     # n_fft no multiple of 4, a ragged input shorter than the chunk
    (80, 4096, 256, 4, 1024, 5000, 2048),    # the largest n_fft
    (80, 2048, 8, 1, 64, 2048, 1024),        # 18 empty filters (narrower than a bin)
)
ENCODER = (128, 2, 2, 512, 100, 41, 43)      # d, L, H, F, T, weight seed, input seed


def waves(i: int) -> np.ndarray:
    """float32 [N_SEG, samples]: the input of configuration i."""
    return np.random.default_rng(1000 + i).standard_normal((N_SEG, CONFIGS[i][5])).astype(np.float32)


def live_frames(n: int, n_samples: int, n_fft: int, hop: int) -> int:
    frames = n_samples // hop
    return frames if n >= n_samples - n_fft else min(frames, -(-(n + n_fft // 2) // hop))


def encoder_input(seed: int, T: int, batch: int = 2) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((batch, 80, 2 * T)) * 0.5, -1.5, 1.5).astype(np.float32)


def make_frontend():
    from transformers import WhisperFeatureExtractor
    from transformers.audio_utils import mel_filter_bank
    out = {}
    for i, (mels, rate, hop, chunk, n_fft, n, fmax) in enumerate(CONFIGS):
        fe = WhisperFeatureExtractor(feature_size=mels, sampling_rate=rate, hop_length=hop, chunk_length=chunk, n_fft=n_fft)
        if fmax != 8000:
            fe.mel_filters = mel_filter_bank(num_frequency_bins=1 + n_fft // 2, num_mel_filters=mels, min_frequency=0.0,
                                             max_frequency=float(fmax), sampling_rate=rate, norm="slaney", mel_scale="slaney")
        w = waves(i)
        padded = np.zeros((N_SEG, fe.n_samples), np.float32)
        padded[:, :min(n, fe.n_samples)] = w[:, :fe.n_samples]
        feats = np.asarray(fe._np_extract_fbank_features(padded, "cpu"))
        frames = fe.n_samples // hop
        assert feats.shape == (N_SEG, mels, frames), feats.shape
        live = live_frames(n, fe.n_samples, n_fft, hop)
        keep = min(frames, live + 3)
        f32 = feats.astype(np.float32)
        pad = f32[:, 0, frames - 1].copy()
        assert np.all(f32[:, :, live:] == pad[:, None, None]) or live == frames, "dead frames are not one constant"
        raw = feats.astype(np.float64) * 4.0 - 4.0
        floor = raw.reshape(N_SEG, -1).max(axis=1)[:, None, None] - 8.0
        # (clamped elements sit exactly on the floor: only the ones strictly above it can be near it)
        near = int(((raw[:, :, :live] > floor) & (raw[:, :, :live] < floor + 0.01)).sum())
        out[f"cfg{i}"] = np.array([mels, rate, hop, chunk, n_fft, n, fmax])
        out[f"hf{i}"] = f32[:, :, :keep]
        out[f"pad{i}"] = pad
        out[f"fb{i}"] = np.asarray(fe.mel_filters, np.float64)
        out[f"near{i}"] = np.array(near)
        print(i, CONFIGS[i], "frames", frames, "live", live, "empty filters", int((out[f"fb{i}"].sum(axis=0) == 0).sum()),
              "near the floor", near)
    path = os.path.join(GOLD, "frontend_configs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def make_encoder():
    import torch
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder

    from gw_whisper_amd import synth
    d, L, H, F, T, wseed, iseed = ENCODER
    sd = synth.encoder_state_dict(d, L, H, F, seed=wseed)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:T]
    cfg = WhisperConfig(d_model=d, encoder_layers=L, encoder_attention_heads=H, encoder_ffn_dim=F, num_mel_bins=80,
                        max_source_positions=T, decoder_layers=1, decoder_attention_heads=H, decoder_ffn_dim=F,
                        attn_implementation="eager")
    enc = WhisperEncoder(cfg).double()
    res = enc.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    enc.eval()
    with torch.no_grad():
        o = enc(torch.from_numpy(encoder_input(iseed, T)).double()).last_hidden_state
    assert o.shape == (2, T, d) and o.dtype == torch.float64
    path = os.path.join(GOLD, "short_context_hf.npz")
    np.savez_compressed(path, last_hidden_state=o.numpy(), config=np.array(ENCODER))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make_frontend()
    make_encoder()
