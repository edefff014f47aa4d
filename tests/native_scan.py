"""Seeded cases shared by tests/test_gpu_native_scan.py and tools/make_golden_scan.py, which records its fixture (a plain
module, deterministic per seed): the catalogue-event scan on Whisper's published front end, whose output on this input is recorded in
tests/golden/scan_events_default.npz, and short-context networks on a native-rate front end."""

import numpy as np

from gw_whisper_amd import synth

SCAN_N = 2048 + 2 * 204            # three windows of 2048 every 204 per event
SCAN_BATCH = 4                     # six windows in all: one full batch and a ragged one that crosses the events
GAIN = 200.0                       # tests/test_gpu_real_events.py: lets a seeded encoder's logits respond at O(0.1)


def scan_strain(n_events=2, n=SCAN_N, seed=7):
    """[E, 2, n] float32: unit noise plus a chirp that depends on event and detector."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 2048.0
    out = rng.standard_normal((n_events, 2, n))
    for e in range(n_events):
        for k in range(2):
            f0, tc = 40.0 + 30.0 * e + 50.0 * k, 0.3 + 0.3 * e + 0.25 * k
            out[e, k] += (3.0 - 5.0 * k) * np.sin(2 * np.pi * (f0 + 90.0 * t) * t) * np.exp(-((t - tc) / 0.2) ** 2)
    return out.astype(np.float32)


def default_scan_model(T, strain):
    """The two-detector MLP model on a seeded micro encoder (bf16, Whisper's own context), its first layer scaled by GAIN and
    its last bias moved so that window 0 of event 0 sits at logit 0."""
    from gw_whisper_amd import models, ops
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.inference import resample
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc = WhisperEncoder.from_numpy_state_dict(synth.encoder_state_dict(d, L, H, F, seed=42), WhisperConfig.named("micro"),
                                               precision="bf16")
    T.manual_seed(3)
    model = models.two_channel_ligo_binary_classifier(enc, num_classes=1).cuda().eval()
    with T.no_grad():
        mel = ops.logmel(resample(T.from_numpy(strain[0, :, :2048].copy()).cuda()))
        model.classifier[0].weight.mul_(GAIN)
        model.classifier[-1].bias.sub_(model(mel[0:1], mel[1:2]).reshape(-1))
    return model
