#!/usr/bin/env python3
"""Golden vectors for the wide encoders (medium, large, large-v3) and the 128-bin front end.

Runs HuggingFace ``transformers`` on the CPU -- ``WhisperFeatureExtractor(feature_size=128)`` (what
``WhisperFeatureExtractor.from_pretrained("openai/whisper-large-v3")`` builds) and ``WhisperEncoder`` -- with
seeded ``gw_whisper_amd.synth`` weights and inputs.  Nothing is downloaded and only OUTPUTS are stored; each
fixture is well under 1 MB.  ``tools/make_golden.py`` and its fixtures are not touched.

    python tools/make_golden_large.py                 # writes the four files below into tests/golden/
    python tools/make_golden_large.py logmel128       # one of them

  logmel128.npz               128-bin log-mel: 1 s segments, ragged lengths, 30 s / truncated, constant collapse
  encoder_medium_reduced.npz  d 1024, H 16, F 4096, 80 mels, 2 layers, B 2
  encoder_large_reduced.npz   d 1280, H 20, F 5120, 128 mels, 2 layers, B 2
  large_v3_last_token.npz     the full 32-layer large-v3 geometry, B 1: last token and mean |x| only
"""

from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transformers import WhisperConfig, WhisperFeatureExtractor  # noqa: E402
from transformers.models.whisper.modeling_whisper import WhisperEncoder  # noqa: E402

from gw_whisper_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ROWS = np.array([0, 1, 2, 49, 50, 51, 52, 53, 700, 1498, 1499])
# (name, d, layers, heads, ffn, n_mels, weight seed): the reduced two-layer encoders of the parity tests
REDUCED = {
    "encoder_medium_reduced": (1024, 2, 16, 4096, 80, 13),
    "encoder_large_reduced": (1280, 2, 20, 5120, 128, 17),
}
LARGE_V3_SEED = 19
INPUT_SEED = 21   # synth.strain_segments(2, seed=21): the input of every encoder fixture (B = 1 takes the first row)


def hf_encoder(d, L, H, ffn, n_mels, sd):
    cfg = WhisperConfig(d_model=d, encoder_layers=L, encoder_attention_heads=H, encoder_ffn_dim=ffn, num_mel_bins=n_mels,
                        decoder_layers=1, decoder_attention_heads=H, decoder_ffn_dim=ffn, attn_implementation="eager")
    enc = WhisperEncoder(cfg)
    res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return enc.eval()


def features(n_mels, n_seg):
    fe = WhisperFeatureExtractor(feature_size=n_mels)
    seg = synth.strain_segments(2, seed=INPUT_SEED)[:n_seg]
    return fe([s for s in seg], sampling_rate=16000, return_tensors="pt").input_features


def make_logmel128():
    fe = WhisperFeatureExtractor(feature_size=128)
    out = {}
    seg = synth.strain_segments(4, seed=11)
    f = fe([s for s in seg], sampling_rate=16000, return_tensors="np").input_features
    assert f.shape == (4, 128, 3000)
    out["seg16000_frames0_112"] = f[:, :, :112].astype(np.float32)
    out["seg16000_pad_value"] = f[:, 0, 2999].astype(np.float32)
    assert np.all(f[:, :, 103:] == f[:, :1, 2999:3000]), "frames >= 103 must be one constant"
    for n in (1, 159, 12345, 40000):
        w = synth.strain_segments(1, seed=100 + n, n_samples=n)[0]
        g = fe(w, sampling_rate=16000, return_tensors="np").input_features[0]
        live = min(3000, -(-(n + 200) // 160))
        out[f"len{n}_frames"] = g[:, :live + 2].astype(np.float32)
        out[f"len{n}_pad_value"] = g[0, 2999].astype(np.float32)
    for n in (480000, 480321):
        w = synth.strain_segments(1, seed=200 + n, n_samples=n)[0]
        g = fe(w, sampling_rate=16000, return_tensors="np").input_features[0]
        cols = np.concatenate([np.arange(0, 3000, 37), np.arange(2990, 3000)])
        out[f"len{n}_cols"] = cols
        out[f"len{n}_frames"] = g[:, cols].astype(np.float32)
    z = fe(np.zeros(16000, np.float32), sampling_rate=16000, return_tensors="np").input_features[0]
    out["zeros_value"] = np.array([z.min(), z.max()], np.float32)
    r = fe((synth.strain_segments(1, seed=5)[0] * 1e-21).astype(np.float32), sampling_rate=16000,
           return_tensors="np").input_features[0]
    out["raw1e21_value"] = np.array([r.min(), r.max()], np.float32)
    np.savez_compressed(os.path.join(GOLD, "logmel128.npz"), **out)
    print("logmel128.npz", {k: v.shape for k, v in out.items()})


def make_reduced(name):
    d, L, H, ffn, n_mels, seed = REDUCED[name]
    sd = synth.encoder_state_dict(d, L, H, ffn, seed=seed, n_mels=n_mels)
    enc = hf_encoder(d, L, H, ffn, n_mels, sd)
    with torch.no_grad():
        final = enc(features(n_mels, 2)).last_hidden_state.numpy()
    out = {"rows": ROWS, "final": final[:, ROWS], "last": final[:, -1], "final_mean_abs": np.abs(final).mean(axis=(1, 2)),
           "config": np.array([d, L, H, ffn, n_mels, seed])}
    np.savez_compressed(os.path.join(GOLD, f"{name}.npz"), **out)
    print(f"{name}.npz", {k: v.shape for k, v in out.items()})


def make_large_v3_last_token():
    d, L, H, ffn = synth.ENCODER_SIZES["large-v3"]
    n_mels = synth.encoder_mels("large-v3")
    t0 = time.time()
    sd = synth.encoder_state_dict(d, L, H, ffn, seed=LARGE_V3_SEED, n_mels=n_mels)
    enc = hf_encoder(d, L, H, ffn, n_mels, sd)
    del sd
    with torch.no_grad():
        final = enc(features(n_mels, 1)).last_hidden_state.numpy()
    out = {"last": final[:, -1], "final_mean_abs": np.abs(final).mean(axis=(1, 2)),
           "config": np.array([d, L, H, ffn, n_mels, LARGE_V3_SEED])}
    np.savez_compressed(os.path.join(GOLD, "large_v3_last_token.npz"), **out)
    print("large_v3_last_token.npz", {k: v.shape for k, v in out.items()}, f"{time.time() - t0:.0f} s")


MAKERS = {
    "logmel128": make_logmel128,
    "encoder_medium_reduced": lambda: make_reduced("encoder_medium_reduced"),
    "encoder_large_reduced": lambda: make_reduced("encoder_large_reduced"),
    "large_v3_last_token": make_large_v3_last_token,
}

if __name__ == "__main__":
    torch.manual_seed(0)
    for k in sys.argv[1:] or list(MAKERS):
        MAKERS[k]()
