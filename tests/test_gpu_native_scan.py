"""The sliding-window consumers on a native-rate front end: ``inference.evaluate_slices`` with ``NativeMelAdapter`` and
``real_events.scan_events(frontend=...)``.  Short-context encoders (T 16 at d 128, T 32 at d 384) on windows of 128 (256)
samples every 8 (16): the shared route of ``ops.logmel_windows`` gives the features of ``ops.logmel`` on the cut windows bit
for bit (tests/test_gpu_logmel_windows.py), so everything behind it -- scores, triggers, tokens -- is compared with
``torch.equal`` / ``==`` and no tolerance is introduced.  The default scan (no ``frontend``) is held to its output at the
commit before this feature, tests/golden/scan_events_default.npz (recorded by ``tests/native_scan.py``'s model and strain)."""

import os

import numpy as np
import pytest

from gw_whisper_amd import synth
from tests import native_scan as ns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# d -> (encoder sizes, context T, front end (n_fft, hop, L), step)
NETS = {128: ((128, 1, 2, 512), 16, (16, 4, 128), 8), 384: ((384, 1, 6, 1536), 32, (16, 4, 256), 16)}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def frontend(d):
    from gw_whisper_amd import ops
    n_fft, hop, L = NETS[d][2]
    return ops.FrontendConfig(80, 2048, n_fft, hop, L, 0.0, 1024.0)


def encoder(T, d):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    (dd, L, H, F), Tn = NETS[d][0], NETS[d][1]
    sd = synth.encoder_state_dict(dd, L, H, F, seed=11)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:Tn].copy()
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(dd, L, H, F, max_source_positions=Tn), precision="bf16").cuda()


def classifier(T, d, route=None, adapter=None):
    """A seeded ``GWWhisperClassifier`` on the short encoder; the first layer of its head is scaled so that the scores move
    with the strain (tests/test_gpu_real_events.py)."""
    from gw_whisper_amd.inference import GWWhisperClassifier, NativeMelAdapter
    T.manual_seed(5)
    net = GWWhisperClassifier(encoder(T, d), adapter=adapter or NativeMelAdapter(frontend(d), route=route)).cuda().eval()
    with T.no_grad():
        net.classifier[0].weight.mul_(ns.GAIN)
    return net


def segment(d, n_windows=11, seed=3):
    """[2, N] float32 two-detector strain holding ``n_windows`` windows: noise plus one loud transient."""
    L, step = NETS[d][2][2], NETS[d][3]
    x = np.random.default_rng(seed).standard_normal((2, L + (n_windows - 1) * step + 3)).astype(np.float32)
    x[:, L + step + 2:L + step + 5] += np.float32(300.0)
    return x


@pytest.mark.parametrize("d", sorted(NETS))
def test_evaluate_slices_shared_route_equals_the_per_window_route(T, gww, d):
    """Batches of 4 cut the 11 windows into 4 + 4 + 3: scores, triggers and returned tokens of the shared route are those
    of the forced per-window route, and those of the materialising path through ``forward``."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer, evaluate_slices
    L, step = NETS[d][2][2], NETS[d][3]
    slicer = DeviceSegmentSlicer(segment(d), delta_t=1.0 / 2048, step_size=step / 2048.0, slice_length=L)
    assert len(slicer) == 11 and slicer.index_step_size == step
    # a threshold between the 5th and the 6th score, so that the trigger list is neither empty nor everything
    first = np.sort(np.concatenate(evaluate_slices(slicer, classifier(T, d), batch_size=4)[1]))
    assert first[4] < first[5], f"two equal scores in the middle: {first}"
    thr = 0.5 * (float(first[4]) + float(first[5]))
    runs = {}
    for route in (None, "per_window"):
        net = classifier(T, d, route)
        trig, vals, tok = evaluate_slices(slicer, net, batch_size=4, trigger_threshold=thr, return_tokens=True)
        plain = evaluate_slices(slicer, net, batch_size=4, trigger_threshold=thr)
        assert ops.last_logmel_windows_route() == ("shared" if route is None else "per_window")
        assert plain[0] == trig and all(np.array_equal(a, b) for a, b in zip(plain[1], vals))
        runs[route] = (trig, vals, tok)
    (trig, vals, tok), (trig_p, vals_p, tok_p) = runs[None], runs["per_window"]
    assert [len(v) for v in vals] == [4, 4, 3] and tok.shape == (11, 2, d)
    assert T.equal(tok, tok_p)
    assert all(np.array_equal(a, b) for a, b in zip(vals, vals_p)) and trig == trig_p
    scores = np.concatenate(vals)
    assert len(trig) == 6 and [t[1] for t in trig] == [float(v) for v in scores if v > thr]
    # ... and the same network on the cut windows (its forward: adapter -> encoder -> head), in the same batches
    net = classifier(T, d)
    with T.no_grad():
        direct = T.cat([net(slicer.windows(i, min(i + 4, 11)).contiguous())[:, 0] for i in range(0, 11, 4)])
    assert np.array_equal(direct.float().cpu().numpy(), scores)


def test_a_resampling_network_still_materialises(T, gww, monkeypatch):
    """A network with ``ResampleMelAdapter`` takes the path it took: ``from_series`` is not reached (there is none on its
    adapter, and ``ops.logmel_windows`` is not called) and the recorded route does not change."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.inference import DeviceSegmentSlicer, GWWhisperClassifier, NativeMelAdapter, ResampleMelAdapter, evaluate_slices
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc = WhisperEncoder.from_numpy_state_dict(synth.encoder_state_dict(d, L, H, F, seed=42), WhisperConfig.named("micro"),
                                               precision="bf16").cuda()
    T.manual_seed(5)
    net = GWWhisperClassifier(enc).cuda().eval()
    assert isinstance(net.adapter, ResampleMelAdapter) and not hasattr(net.adapter, "from_series")
    ops.logmel_windows(T.zeros(1, 136, device="cuda"), frontend(128), 8)          # leaves a route on record
    before = ops.last_logmel_windows_route()
    assert before == "shared"

    def unreachable(*a, **k):
        raise AssertionError("the materialising path must not reach the series front end")
    monkeypatch.setattr(ops, "logmel_windows", unreachable)
    monkeypatch.setattr(NativeMelAdapter, "from_series", unreachable)
    x = np.random.default_rng(1).standard_normal((2, 2048 + 2 * 204)).astype(np.float32)
    slicer = DeviceSegmentSlicer(x, step_size=204 / 2048.0)
    trig, vals = evaluate_slices(slicer, net, batch_size=2)
    assert [len(v) for v in vals] == [2, 1] and ops.last_logmel_windows_route() == before
    with T.no_grad():
        want = T.cat([net(slicer.windows(0, 2).contiguous()), net(slicer.windows(2, 3).contiguous())])[:, 0]
    assert np.array_equal(np.concatenate(vals), want.float().cpu().numpy())


@pytest.mark.parametrize("batch_size", [4, 16, 256])
def test_scan_events_native_equals_the_window_loop(T, gww, batch_size):
    """[E = 2, 2, N] with 11 windows per event: ``scan_events(frontend=cfg)`` against a loop that cuts each window, runs
    ``ops.logmel(config=cfg)`` on it, and runs the model on the same groups of windows, bit for bit -- in batches smaller than
    an event, of one event and of both.  (One window at a time through the model is printed: the head's GEMM is PyTorch's,
    whose bits may depend on the batch; the front end's and the encoder's do not.)"""
    from gw_whisper_amd import GwwError, models, ops, real_events
    d = 128
    cfg, (L, step) = frontend(d), (NETS[d][2][2], NETS[d][3])
    T.manual_seed(9)
    model = models.two_channel_ligo_binary_classifier(encoder(T, d), num_classes=1).cuda().eval()
    with T.no_grad():
        model.classifier[0].weight.mul_(ns.GAIN)
    strain = np.stack([segment(d, seed=3), segment(d, seed=4)])
    got = real_events.scan_events(model, strain, batch_size=batch_size, window_size=L, step_size=step, frontend=cfg)
    assert ops.last_logmel_windows_route() == "shared"
    dev = T.from_numpy(strain).cuda()
    want, single = T.zeros((2, 11), device="cuda"), T.zeros((2, 11), device="cuda")
    mel = T.empty((2, 11, 2, 80, cfg.n_frames), device="cuda")
    if batch_size <= 11:
        groups = [(e, e + 1, j, min(j + batch_size, 11)) for e in range(2) for j in range(0, 11, batch_size)]
    else:
        groups = [(e, min(e + batch_size // 11, 2), 0, 11) for e in range(0, 2, batch_size // 11)]
    with T.no_grad():
        for e in range(2):
            for j in range(11):
                mel[e, j] = ops.logmel(dev[e, :, j * step:j * step + L].contiguous(), config=cfg)
                single[e, j] = T.sigmoid(model(mel[e, j, 0:1], mel[e, j, 1:2]).float()).reshape(())
        for e0, e1, j0, j1 in groups:
            m = mel[e0:e1, j0:j1]
            h1, l1 = (m[:, :, k].reshape(-1, 80, cfg.n_frames) for k in (0, 1))
            want[e0:e1, j0:j1] = T.sigmoid(model(h1, l1).float()).reshape(e1 - e0, j1 - j0)
    want, single = want.cpu().numpy(), single.cpu().numpy()
    print(f"batch {batch_size}: max |scan - one window at a time| = {np.abs(got - single).max():.3e}")
    assert got.shape == (2, 11) and got.dtype == np.float32
    assert np.array_equal(got, want), f"max |scan - loop| = {np.abs(got - want).max():.3e}"
    assert np.ptp(got) > 1e-3
    with pytest.raises(GwwError, match=r"frontend.n_samples is 128 but window_size is 64"):
        real_events.scan_events(model, strain, window_size=64, frontend=cfg)


def test_scan_events_default_is_what_it_was(T, gww):
    """No ``frontend``: resample + published log-mel, the output of the commit before the native front end on the same
    seeded model and strain (ragged batches of 4 across the events), element for element."""
    from gw_whisper_amd import real_events
    with np.load(os.path.join(ROOT, "tests", "golden", "scan_events_default.npz")) as z:
        want = z["model_output"]
    strain = ns.scan_strain()
    got = real_events.scan_events(ns.default_scan_model(T, strain), strain, batch_size=ns.SCAN_BATCH)
    print("max |scan - recorded| =", float(np.abs(got - want).max()), "span", float(want.min()), float(want.max()))
    assert got.shape == want.shape == (2, 3) and got.dtype == want.dtype
    assert np.array_equal(got, want)
    assert np.ptp(want) > 1e-3
