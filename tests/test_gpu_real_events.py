"""The catalogue-event scan on the device (``real_events.scan_events``, ``harness/run_real_events.py``) against the same
windows scored one at a time, at batch 1, through the public pieces (``inference.resample``, ``ops.logmel``, the model).
1e-3 on the logit is the project's bf16 logit tolerance.  Needs an MI355X."""

import os
import sys

import numpy as np
import pytest

from gw_whisper_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harness"))

KEYS = ["GW150914-v3", "GW170817-v2", "GW190521_074359-v1"]
N = 2660                      # 4 windows of 2048 every 204
TOL = 1e-3
SEED = 42
GAIN = 200.0
LAST_GAIN = {"mlp": 1.0, "cnn": 50.0}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_strain():
    """[3, 2, N]: unit noise plus a chirp whose band, centre and sign depend on event and detector, so that every window
    and both detectors differ at O(1)."""
    rng = np.random.default_rng(5)
    t = np.arange(N) / 2048.0
    out = rng.standard_normal((len(KEYS), 2, N))
    for e in range(len(KEYS)):
        for k in range(2):
            f0, tc = 30.0 + 25.0 * e + 60.0 * k, 0.35 + 0.25 * e + 0.3 * k
            out[e, k] += (3.0 - 5.0 * k) * np.sin(2 * np.pi * (f0 + 90.0 * t) * t) * np.exp(-((t - tc) / 0.2) ** 2)
    return out.astype(np.float32)


def make_peft(T):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=SEED)
    enc = WhisperEncoder(WhisperConfig.named("micro"), precision="bf16")
    enc.load_state_dict({k: T.from_numpy(v) for k, v in sd.items()})
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj", "v_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    g = T.Generator(device="cuda").manual_seed(2)
    with T.no_grad():
        for n, p in peft.named_parameters():
            if "lora_B" in n:
                p.copy_(0.02 * T.randn(p.shape, generator=g, device="cuda"))
    return peft


@pytest.fixture(scope="module")
def setup(T):
    """The two models on one adapted micro encoder, the strain, and the single-window logits [head][E, W] (computed once)."""
    from gw_whisper_amd import models, ops, real_events
    from gw_whisper_amd.inference import resample
    peft = make_peft(T)
    T.manual_seed(3)
    ms = {"mlp": models.two_channel_ligo_binary_classifier(peft, num_classes=1).cuda().eval(),
          "cnn": models.TwoChannelLIGOBinaryClassifierCNN(peft, num_classes=1).cuda().eval()}
    strain = make_strain()
    starts = list(real_events.window_starts(N))
    assert len(starts) == 4
    dev = T.from_numpy(strain).cuda()
    # a seeded encoder under a default-init head answers an O(1) change of the strain with a change of the logit near 1e-3,
    # the tolerance itself (the CNN head, which averages over the length, with less): the first layer of each head, and the
    # CNN's last, are scaled so that the logits respond at O(0.1), and the last bias is moved so that window (0, 0) sits at
    # logit 0, in the middle of the sigmoid
    with T.no_grad():
        mel = ops.logmel(resample(dev[0, :, :2048].contiguous()))
        for h, m in ms.items():
            m.classifier[0].weight.mul_(GAIN)
            m.classifier[-1].weight.mul_(LAST_GAIN[h])
            m.classifier[-1].bias.sub_(m(mel[0:1], mel[1:2]).reshape(-1))
    single = {h: np.zeros((len(KEYS), len(starts))) for h in ms}
    with T.no_grad():
        for e in range(len(KEYS)):
            for j, s in enumerate(starts):
                mel = ops.logmel(resample(dev[e, :, s:s + 2048].contiguous()))         # [2, 80, 3000]: H1, L1
                for h, m in ms.items():
                    single[h][e, j] = float(m(mel[0:1], mel[1:2]))
    return ms, peft, strain, single


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


@pytest.mark.parametrize("head", ["mlp", "cnn"])
def test_scan_equals_the_single_windows_at_batch_1(T, gww, setup, head):
    from gw_whisper_amd import real_events
    ms, _, strain, single = setup
    for bs in (256, 5):                                    # one pass over all events; ragged batches across events
        out = real_events.scan_events(ms[head], strain, batch_size=bs)
        assert out.shape == single[head].shape and out.dtype == np.float32
        err = np.abs(_logit(out) - single[head]).max()
        print(f"[{head}, batch {bs}] max|logit(scan) - logit(single window)| = {err:.3e}; logits span "
              f"{single[head].min():.3f} .. {single[head].max():.3f}")
        assert err <= TOL
        np.testing.assert_allclose(out, 1.0 / (1.0 + np.exp(-single[head])), atol=TOL)


@pytest.mark.parametrize("head", ["mlp", "cnn"])
def test_detector_order(T, gww, setup, head):
    """H1 is the model's first argument: swapping the detectors in the input moves the output by far more than 1e-3."""
    from gw_whisper_amd import real_events
    ms, _, strain, single = setup
    swapped = real_events.scan_events(ms[head], strain[:, ::-1].copy())
    diff = np.abs(_logit(swapped) - single[head])
    print(f"[{head}] |logit(swapped) - logit| : min {diff.min():.3e}, median {np.median(diff):.3e}, max {diff.max():.3e}")
    assert np.median(diff) > 10 * TOL


def test_harness_end_to_end_on_the_twin(T, gww, setup, tmp_path):
    """Both --head values on the .npz twin: both datasets written, names cut at the first '-', --event_name order kept,
    --first-window-only equal to column 0; a head file of the other kind is refused."""
    import run_real_events
    from gw_whisper_amd import GwwError, real_events
    ms, peft, strain, _ = setup
    data = str(tmp_path / "events.npz")
    np.savez(data, **{f"{k}/{d}_strain": strain[e, i] for e, k in enumerate(KEYS) for i, d in enumerate(("h1", "l1"))})
    lora = str(tmp_path / "best_lora_weights_8_32")
    peft.save_pretrained(lora)
    have_h5 = real_events._have_h5py()
    for head in ("mlp", "cnn"):
        dense = str(tmp_path / f"dense_{head}.pth")
        T.save(ms[head].classifier.state_dict(), dense)
        want = real_events.scan_events(ms[head], strain)
        base = ["--timeseries_data_test", data, "--encoder", "micro", "--seed", str(SEED), "--lora_weights_file", lora,
                "--dense_layers_file", dense, "--head", head]

        def run(name, *extra):
            path = str(tmp_path / name)
            run_real_events.main(run_real_events.build_parser().parse_args(base + ["--output_path", path, *extra]))
            if have_h5:
                import h5py
                with h5py.File(path, "r") as f:
                    return f["model_output"][()], [n.decode() if isinstance(n, bytes) else n for n in f["event_names"][()]]
            with np.load(path + ".npz") as z:
                return z["model_output"], list(z["event_names"])
        out, names = run(f"all_{head}.hdf")
        assert names == ["GW150914", "GW170817", "GW190521_074359"]
        assert out.shape == (3, 4) and np.abs(_logit(out) - _logit(want)).max() <= TOL
        first, _ = run(f"first_{head}.hdf", "--first-window-only")
        assert first.shape == (3, 1) and np.abs(_logit(first[:, 0]) - _logit(out[:, 0])).max() <= TOL
        sel, names = run(f"sel_{head}.hdf", "--event_name", KEYS[2], KEYS[0])
        assert names == ["GW190521_074359", "GW150914"] and np.abs(_logit(sel) - _logit(out[[2, 0]])).max() <= TOL
    with pytest.raises(GwwError, match="--head cnn needs a rank-3"):
        run_real_events.main(run_real_events.build_parser().parse_args(
            ["--timeseries_data_test", data, "--encoder", "micro", "--lora_weights_file", lora, "--dense_layers_file",
             str(tmp_path / "dense_mlp.pth"), "--head", "cnn", "--output_path", str(tmp_path / "x.hdf")]))
