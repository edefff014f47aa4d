#!/usr/bin/env python3
"""Golden vectors of the encoder's per-layer outputs (``output_hidden_states`` / ``output_attentions``).

Runs HuggingFace ``transformers``' ``WhisperEncoder`` on the CPU with ``attn_implementation="eager"`` (the
implementation that returns the attention probabilities) on seeded ``gw_whisper_amd.synth`` weights and a seeded
input-feature tensor.  Nothing is downloaded and only OUTPUTS (and the seeds that regenerate the inputs) are stored.
``tools/make_golden.py``, ``tools/make_golden_large.py`` and their fixtures are not touched.

    python tools/make_golden_outputs.py      # writes tests/golden/encoder_outputs.npz

Two reduced 2-layer encoders at B = 2: ``tiny`` geometry (d 384, H 6, F 1536: the fused whisper-tiny path) and
``base`` geometry (d 512, H 8, F 2048: the generic path).  Per encoder ``<name>``:

  <name>_hidden<i>   hidden_states[i][:, ROWS]            for i = 0 .. L     [2, len(ROWS), d]
  <name>_attn<l>     attentions[l][0, :, QROWS, :]        for l = 0 .. L-1   [H, len(QROWS), 1500]
  <name>_config      d, L, H, F, weight seed, input seed
plus ``rows`` (= ROWS) and ``qrows`` (= QROWS).
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transformers import WhisperConfig  # noqa: E402
from transformers.models.whisper.modeling_whisper import WhisperEncoder  # noqa: E402

from gw_whisper_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ROWS = np.array([0, 1, 2, 49, 50, 51, 52, 53, 700, 1498, 1499])   # the convention of tools/make_golden_large.py
QROWS = np.array([0, 50, 777, 1499])
# name -> (d, layers, heads, ffn, weight seed, input seed)
ENCODERS = {
    "tiny": (384, 2, 6, 1536, 23, 31),
    "base": (512, 2, 8, 2048, 29, 37),
}


def input_features(seed: int, batch: int = 2) -> np.ndarray:
    """Seeded stand-in for log-mel features, [batch, 80, 3000] fp32, in the range Whisper's normalised log-mel
    takes (about -1.5 .. 1.5).  The GPU test regenerates it from the stored seed."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((batch, 80, 3000)) * 0.5, -1.5, 1.5).astype(np.float32)


def make():
    out = {"rows": ROWS, "qrows": QROWS}
    for name, (d, L, H, ffn, wseed, iseed) in ENCODERS.items():
        sd = synth.encoder_state_dict(d, L, H, ffn, seed=wseed)
        cfg = WhisperConfig(d_model=d, encoder_layers=L, encoder_attention_heads=H, encoder_ffn_dim=ffn, num_mel_bins=80,
                            decoder_layers=1, decoder_attention_heads=H, decoder_ffn_dim=ffn, attn_implementation="eager")
        enc = WhisperEncoder(cfg)
        res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        enc.eval()
        with torch.no_grad():
            o = enc(torch.from_numpy(input_features(iseed)), output_hidden_states=True, output_attentions=True)
        assert len(o.hidden_states) == L + 1 and len(o.attentions) == L
        assert torch.equal(o.hidden_states[-1], o.last_hidden_state)
        for i, hs in enumerate(o.hidden_states):
            out[f"{name}_hidden{i}"] = hs.numpy()[:, ROWS].astype(np.float32)
        for l, at in enumerate(o.attentions):
            assert at.shape == (2, H, 1500, 1500)
            out[f"{name}_attn{l}"] = at.numpy()[0][:, QROWS, :].astype(np.float32)
        out[f"{name}_config"] = np.array([d, L, H, ffn, wseed, iseed])
    path = os.path.join(GOLD, "encoder_outputs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    make()
