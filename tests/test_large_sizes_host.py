"""The wide encoder sizes (medium, large, large-v2, large-v3, large-v3-turbo) and large-v3's 128-bin front end, on
the host: the C++ twin of the log-mel kernel against HF ``WhisperFeatureExtractor(feature_size=128)``
(tools/make_golden_large.py), the named configurations, the extractor's name -> feature_size mapping, the
``num_mel_bins`` round trip through ``save_pretrained``, and the seeded weights of the existing sizes.  CPU only."""

import hashlib
import json

import numpy as np
import pytest
import torch

from gw_whisper_amd import GwwError, ops, synth
from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor

TOL = 1e-5   # the 80-bin host twin's tolerance (test_logmel_host.py)


def test_seg16000_128_matches_hf(golden):
    g = golden("logmel128.npz")
    seg = synth.strain_segments(4, seed=11)
    out = ops.logmel_host(seg, n_mels=128).numpy()
    assert out.shape == (4, 128, 3000) and out.dtype == np.float32
    np.testing.assert_allclose(out[:, :, :112], g["seg16000_frames0_112"], atol=TOL, rtol=0)
    for i in range(4):
        assert np.all(out[i, :, 103:] == out[i, 0, 2999])
        assert abs(out[i, 0, 2999] - g["seg16000_pad_value"][i]) < TOL


@pytest.mark.parametrize("n", [1, 159, 12345, 40000])
def test_ragged_lengths_128(golden, n):
    g = golden("logmel128.npz")
    w = synth.strain_segments(1, seed=100 + n, n_samples=n)[0]
    out = ops.logmel_host(w, n_mels=128).numpy()[0]
    ref = g[f"len{n}_frames"]
    np.testing.assert_allclose(out[:, :ref.shape[1]], ref, atol=TOL, rtol=0)
    assert abs(out[0, 2999] - g[f"len{n}_pad_value"]) < TOL


@pytest.mark.parametrize("n", [480000, 480321])
def test_full_and_truncated_128(golden, n):
    g = golden("logmel128.npz")
    w = synth.strain_segments(1, seed=200 + n, n_samples=n)[0]
    out = ops.logmel_host(w, n_mels=128).numpy()[0]
    np.testing.assert_allclose(out[:, g[f"len{n}_cols"]], g[f"len{n}_frames"], atol=TOL, rtol=0)


def test_constant_collapse_128(golden):
    g = golden("logmel128.npz")
    z = ops.logmel_host(np.zeros(16000, np.float32), n_mels=128).numpy()[0]
    assert z.min() == g["zeros_value"][0] and z.max() == g["zeros_value"][1] == -1.5
    r = ops.logmel_host((synth.strain_segments(1, seed=5)[0] * 1e-21).astype(np.float32), n_mels=128).numpy()[0]
    assert r.min() == g["raw1e21_value"][0] and r.max() == g["raw1e21_value"][1]


def test_80_bins_unchanged_by_the_n_mels_entry(golden):
    seg = synth.strain_segments(2, seed=11)
    assert torch.equal(ops.logmel_host(seg), ops.logmel_host(seg, n_mels=80))
    with pytest.raises(GwwError, match="n_mels"):
        ops.logmel_host(seg, n_mels=64)


@pytest.mark.parametrize("name, geometry, n_mels", [
    ("medium", (1024, 24, 16, 4096), 80),
    ("large", (1280, 32, 20, 5120), 80),
    ("large-v2", (1280, 32, 20, 5120), 80),
    ("large-v3", (1280, 32, 20, 5120), 128),
    ("large-v3-turbo", (1280, 32, 20, 5120), 128),
])
def test_named_configs(name, geometry, n_mels):
    c = WhisperConfig.named(name)
    assert (c.d_model, c.encoder_layers, c.encoder_attention_heads, c.encoder_ffn_dim) == geometry
    assert c.num_mel_bins == n_mels == synth.encoder_mels(name)
    assert c.max_source_positions == 1500
    assert synth.ENCODER_SIZES[name] == geometry


def test_existing_named_configs_keep_80_mels():
    for name in ("tiny", "base", "small", "micro"):
        assert WhisperConfig.named(name).num_mel_bins == 80
    with pytest.raises(KeyError):
        WhisperConfig.named("huge")


@pytest.mark.parametrize("name, feature_size", [
    ("openai/whisper-tiny", 80), ("openai/whisper-base", 80), ("openai/whisper-small", 80),
    ("openai/whisper-medium", 80), ("openai/whisper-large", 80), ("openai/whisper-large-v2", 80),
    ("openai/whisper-large-v3", 128), ("openai/whisper-large-v3-turbo", 128),
])
def test_feature_extractor_from_pretrained(name, feature_size):
    fe = WhisperFeatureExtractor.from_pretrained(name)
    assert fe.feature_size == feature_size
    assert WhisperFeatureExtractor.from_pretrained(name, feature_size=80).feature_size == 80


def test_feature_extractor_128_on_host(tmp_path):
    with open(tmp_path / "preprocessor_config.json", "w") as f:
        json.dump({"feature_size": 128, "sampling_rate": 16000}, f)
    fe = WhisperFeatureExtractor.from_pretrained(str(tmp_path))
    assert fe.feature_size == 128
    seg = synth.strain_segments(2, seed=11)
    out = fe([seg[0], seg[1]], sampling_rate=16000, return_tensors="pt").input_features
    assert out.shape == (2, 128, 3000)
    assert torch.equal(out, ops.logmel_host(seg, n_mels=128))
    with pytest.raises(ValueError):
        WhisperFeatureExtractor(feature_size=64)


def test_save_pretrained_carries_num_mel_bins(tmp_path):
    cfg = WhisperConfig(128, 1, 2, 512, num_mel_bins=128)
    enc = WhisperEncoder(cfg)
    sd = synth.encoder_state_dict(128, 1, 2, 512, seed=4, n_mels=128)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    enc.save_pretrained(str(tmp_path))
    with open(tmp_path / "config.json") as f:
        assert json.load(f)["num_mel_bins"] == 128
    back = WhisperEncoder.from_pretrained(str(tmp_path))
    assert back.config == cfg
    assert tuple(back.conv1.weight.shape) == (128, 128, 3)
    assert torch.equal(back.conv1.weight, torch.from_numpy(sd["conv1.weight"]))


# sha256 (first 16 hex digits) of conv1.weight and of the last layer's fc2.weight drawn by
# synth.named_encoder_state_dict(name, seed=0) before the wide sizes were added
_WEIGHT_HASHES = {
    "tiny": ("90725e3b25c87d89", "b1b3a3a9b8bfeaea"),
    "base": ("773714e9ddd5bb03", "ea070af98b96ffd4"),
    "small": ("70d327f24f8dcef7", "5b372cdf507d3fa5"),
    "micro": ("8aaa5abc1962e7d0", "4dabd930fdb6c451"),
}


@pytest.mark.parametrize("name", sorted(_WEIGHT_HASHES))
def test_existing_sizes_draw_the_same_weights(name):
    sd = synth.named_encoder_state_dict(name, seed=0)
    L = synth.ENCODER_SIZES[name][1]
    got = tuple(hashlib.sha256(np.ascontiguousarray(sd[k]).tobytes()).hexdigest()[:16]
                for k in ("conv1.weight", f"layers.{L - 1}.fc2.weight"))
    assert got == _WEIGHT_HASHES[name]
